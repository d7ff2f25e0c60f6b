"""Times of the YOLOv3 pieces on one MI355X, bf16, B = 32 at 640 x 640: every mgdt_maxpool2d_fwd / mgdt_maxpool2d_bwd shape of yolov3-tiny, the ZeroPad2d +
MaxPool2d(2, 1) pair (forward: zero fill + copy + pool; reverse: pool adjoint, the pad's is a view), mgdt_spp_pool_bwd at yolov3-spp's P5 map, each beside
mgdt_copy_fwd moving the same number of bytes (the floor of a kernel that is pure traffic); the three graphs' forward + decode and + NMS, and the training
step of yolov3-tiny, each as one captured graph.

    python tools/yolov3_bench.py [--rounds 5] [--steps 20] [--reps 10] [--warmup 5] [--batch 32] [--size 640] [--no-train] [--no-full]

Protocol of tools/yolov6_bench.py: every piece is captured once (torch.cuda.graph) and replayed; one measurement is `reps` back-to-back replays between two
HIP events, divided by `reps`; the pieces alternate measurement by measurement in one process; a round's figure is the median of `steps` measurements and
the spread of a piece is (max - min) / median over the rounds' medians.  `MB` = the bytes a piece must move (each tensor once), `TB_per_s` = MB over its
time, `copy_us` = ops.copy of a dense bf16 map of MB / 2 bytes (read + write = MB).  Also printed, for a later decision and without building them: the bytes
a Conv + BN + SiLU + MaxPool2d(2, 2) epilogue would save on tiny's first two rows (the maps between the convolutions and their pools are then neither
written nor read) and what a fused pad + pool would save (the padded map).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.models import get_config  # noqa: E402
from mgdt_yolo_amd.nn.modules import MaxPool2d, ZeroPad2d  # noqa: E402
from mgdt_yolo_amd.nn.tasks import DetectionModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images, seeded_labels  # noqa: E402
from tools.yolov6_bench import Captured, Stepper, timed  # noqa: E402

DEV = 'cuda:0'
med = statistics.median
# (name, channels, input map side at 640 / this, stride): rows 1, 3, 5, 7, 9 of yolov3-tiny, then row 12 on the padded P5 map
POOLS = [('l1', 16, 1, 2), ('l3', 32, 2, 2), ('l5', 64, 4, 2), ('l7', 128, 8, 2), ('l9', 256, 16, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--no-full', action='store_true', help='leave out the two full-width darknet53 graphs')
    a = ap.parse_args()
    B, S, bf = a.batch, a.size, torch.bfloat16
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(bf).to(DEV).contiguous(memory_format=torch.channels_last)
    pieces, meta = {}, {}

    def add(key, fn, nbytes, **info):
        pieces[key] = Captured(fn, a.warmup)
        n = max(int(nbytes // 4), 8)                                   # bf16 elements of a map whose copy reads + writes `nbytes`
        src = torch.zeros(1, 8, 1, n // 8, dtype=bf, device=DEV).contiguous(memory_format=torch.channels_last)
        dst = torch.empty_like(src)
        pieces[key + '_copy'] = Captured(lambda: ops.copy(src, dst), a.warmup)
        meta[key] = dict(MB=round(nbytes / 1e6, 2), **info)

    for name, c, red, s in POOLS:
        h = S // red
        x, gy = rnd(B, c, h, h), rnd(B, c, h // 2, h // 2)
        y, gx = ops.maxpool2d(x, 2, s), ops.like(x)
        add(f'maxpool2d_fwd_{name}', lambda x=x, y=y, s=s: ops.maxpool2d(x, 2, s, out=y), (x.numel() + y.numel()) * 2, channels=c, map=h, stride=s)
        add(f'maxpool2d_bwd_{name}', lambda x=x, gy=gy, gx=gx, s=s: ops.maxpool2d_bwd(x, gy, 2, s, gx=gx), (2 * x.numel() + gy.numel()) * 2, channels=c, map=h, stride=s)
    h5 = S // 32
    x5, g5 = rnd(B, 512, h5, h5), rnd(B, 512, h5, h5)
    pad, pool = ZeroPad2d((0, 1, 0, 1)), MaxPool2d(2, 1, 0)
    xp = pad(x5)
    add('maxpool2d_fwd_l12', lambda: ops.maxpool2d(xp, 2, 1), (xp.numel() + x5.numel()) * 2, channels=512, map=h5 + 1, stride=1)
    add('maxpool2d_bwd_l12', lambda: ops.maxpool2d_bwd(xp, g5, 2, 1), (2 * xp.numel() + g5.numel()) * 2, channels=512, map=h5 + 1, stride=1)
    add('pad_pool_fwd_l11_l12', lambda: pool(pad(x5)), (2 * x5.numel() + 3 * xp.numel()) * 2, channels=512, map=h5, launches='fill + copy + pool')
    # SPP(1024, 512) at full width: c_ = 512 channels per slot of the concat buffer, on the P5 map of yolov3-spp
    cat, gcat = rnd(B, 4 * 512, h5, h5), rnd(B, 4 * 512, h5, h5)
    sl = lambda t, i: t[:, i * 512:(i + 1) * 512]
    add('spp_pool_bwd_p5', lambda: ops.spp_pool_bwd(sl(cat, 0), sl(gcat, 1), sl(gcat, 2), sl(gcat, 3)), B * 512 * h5 * h5 * (4 * 2 + 4 + 4 + 2), channels=512, map=h5)
    img = (seeded_images(B, S, S, seed=2) * 255).to(torch.uint8).to(DEV)
    graphs = ['yolov3-tiny'] + ([] if a.no_full else ['yolov3', 'yolov3-spp'])
    for name in graphs:
        model = seed_state_dict_(DetectionModel(get_config(name, '', 80), verbose=False), 0).eval().to(DEV).set_compute_dtype(bf)
        pieces[f'{name}_forward_decode'] = Captured(lambda model=model: model(img), a.warmup)
        pieces[f'{name}_forward_decode_nms'] = Captured(lambda model=model: ops.nms(model(img)[0], 0.25, 0.7, None, False, False, 300, 30000, 7680), a.warmup)
    if not a.no_train:
        from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
        tm = seed_state_dict_(DetectionModel(get_config('yolov3-tiny', '', 80), verbose=False), 0).to(DEV)
        lab = seeded_labels(B, 80, seed=3, max_boxes=8, min_boxes=2)
        pieces['yolov3-tiny_train_step'] = Stepper(DetectionTrainer(tm, lr0=0.01, amp=True, graph=True, batch_size=B, nb=100, epochs=3), dict(img=img, **lab))
    rounds = {k: [] for k in pieces}
    for _ in range(a.rounds):
        ts = {k: [] for k in pieces}
        for _ in range(a.steps):
            for k, g in pieces.items():
                ts[k].append(timed(g, 1 if k.endswith('train_step') else a.reps))
        for k in pieces:
            rounds[k].append(med(ts[k]))
    out = {'batch': B, 'size': S, 'dtype': 'bf16', 'rounds': a.rounds, 'steps': a.steps, 'reps': a.reps}
    spread = lambda k: (max(rounds[k]) - min(rounds[k])) / med(rounds[k])
    tbs = lambda mb, t: round(mb * 1e6 / (t * 1e-3) / 1e12, 3)
    for key, row in meta.items():
        t, tc = med(rounds[key]), med(rounds[key + '_copy'])
        row.update(us=round(t * 1e3, 2), spread=round(spread(key), 4), TB_per_s=tbs(row['MB'], t), copy_us=round(tc * 1e3, 2), copy_spread=round(spread(key + '_copy'), 4),
                   times_copy=round(t / tc, 2))
        out[key] = row
    for k in pieces:
        if k.startswith('yolov3'):
            t = med(rounds[k])
            out[k] = dict(us=round(t * 1e3, 2), spread=round(spread(k), 4), images_per_s=round(B / (t * 1e-3), 1))
    # not built: what the fusions would save, in bytes the unfused rows move and the fused ones would not (bf16)
    e = lambda c, red: B * c * (S // red) ** 2 * 2
    out['not_built_conv_pool_epilogue_rows_0_to_3'] = dict(saved_MB=round(2 * (e(16, 1) + e(32, 2)) / 1e6, 1),
                                                           note='rows 0-1 and 2-3: the 16- and 32-channel maps between Conv and pool, written once and read once')
    out['not_built_fused_pad_pool'] = dict(saved_MB=round(2 * xp.numel() * 2 / 1e6, 2), note='the padded P5 map: written (fill + copy) and read once')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
