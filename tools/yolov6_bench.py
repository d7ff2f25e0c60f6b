"""Times of the YOLOv6 pieces on one MI355X, bf16, B = 32 at 640 x 640: the ConvTranspose2d layer's data and weight gradients, one launch each
(mgdt_deconv2x2_dgrad / mgdt_deconv2x2_wgrad) against the composed route (four strided-view 1x1 launches per gradient) at the yolov6n and yolov6s shapes;
every repeated 3x3 row of yolov6n on the composed route (the input of a later chain-kernel decision); yolov6n forward + decode, + NMS, and the training
step, each as one captured graph.

    python tools/yolov6_bench.py [--rounds 5] [--steps 20] [--reps 10] [--warmup 5] [--batch 32] [--size 640] [--no-train]

Protocol of tools/c3_bench.py: every piece is captured once (torch.cuda.graph) and replayed; one measurement is `reps` back-to-back replays between two
HIP events, divided by `reps`; the pieces alternate measurement by measurement in one process; a round's figure is the median of `steps` measurements and
the spread of a piece is (max - min) / median over the rounds' medians.  `fused_pays` is true where the fused median is below the composed one by more than
the sum of the two spreads: the rule by which ops.DECONV_DX_FUSED_CLASSES / ops.DECONV_DW_FUSED_CLASSES are filled.  Both routes of both gradients are
timed through the calls the layer makes (ops.deconv2x2_dgrad / ops.deconv2x2_wgrad with ops.DECONV_BWD_FUSED forced); the composed data gradient's four
panels are packed from the weight while the piece is warmed and stay cached, as in a training step, where the batched re-pack refreshes them.  `TB_per_s` = the bytes a piece must move (each tensor once) over its time:
its distance from the HBM floor.  Prints one JSON line."""
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
from mgdt_yolo_amd.nn.modules import Repeat  # noqa: E402
from mgdt_yolo_amd.nn.tasks import DetectionModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images, seeded_labels  # noqa: E402

DEV = 'cuda:0'
med = statistics.median
# (name, channels, input map side at 640 / this): layers 11 and 16 of yolov6n, then of yolov6s
DECONVS = [('n_l11', 64, 32), ('n_l16', 32, 16), ('s_l11', 128, 32), ('s_l16', 64, 16)]


class Captured:
    """One piece captured into a graph; the object owns everything the graph reads and writes for as long as it can be replayed (tools/c3_bench.py)."""

    def __init__(self, fn, warmup):
        self.fn = fn
        with torch.no_grad():
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = fn()
        self.graph.replay()
        torch.cuda.synchronize()

    def replay(self):
        self.graph.replay()


class Stepper:
    """The trainer's captured step as a piece: replay() is one DetectionTrainer.step on the same batch."""

    def __init__(self, tr, batch):
        self.tr, self.batch = tr, batch
        for _ in range(3):
            tr.step(batch)
        torch.cuda.synchronize()

    def replay(self):
        self.tr.step(self.batch)


def timed(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--no-train', action='store_true')
    a = ap.parse_args()
    B, S, bf = a.batch, a.size, torch.bfloat16
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV).to(bf).contiguous(memory_format=torch.channels_last)
    pieces, meta = {}, {}
    shipped = ops.DECONV_BWD_FUSED
    for name, c, red in DECONVS:
        h = S // red
        x, dy, dx = rnd(B, c, h, h), rnd(B, c, 2 * h, 2 * h), rnd(B, c, h, h)
        w = (torch.randn(c, c, 2, 2, generator=gen) / c ** 0.5).to(DEV)
        dw = torch.empty_like(w)
        for route in ('composed', 'fused'):
            ops.DECONV_BWD_FUSED = route == 'fused'                     # the route is chosen while the piece is warmed and captured
            try:
                pieces[f'deconv_{name}_dx_{route}'] = Captured(lambda dy=dy, w=w, dx=dx: ops.deconv2x2_dgrad(dy, w, dx), a.warmup)
                pieces[f'deconv_{name}_dw_{route}'] = Captured(lambda x=x, dy=dy, dw=dw: ops.deconv2x2_wgrad(x, dy, dw), a.warmup)
            finally:
                ops.DECONV_BWD_FUSED = shipped
        meta[f'deconv_{name}_dx'] = dict(channels=c, map=h, MB=round((dy.numel() + dx.numel()) * 2 / 1e6 + w.numel() * 4 / 1e6, 2))
        meta[f'deconv_{name}_dw'] = dict(channels=c, map=h, MB=round((dy.numel() + x.numel()) * 2 / 1e6, 2))
    model = seed_state_dict_(DetectionModel(get_config('yolov6', 'n', 80), verbose=False), 0).eval().to(DEV).set_compute_dtype(bf)
    for l in model.model:
        if isinstance(l, Repeat):
            c, h = l[0].conv.in_channels, int(S // model._reductions[l.i])
            x = rnd(B, c, h, h)
            pieces[f'row{l.i}'] = Captured(lambda l=l, x=x: l(x), a.warmup)
            meta[f'row{l.i}'] = dict(n=len(l), channels=c, map=h, MB=round(len(l) * 2 * x.numel() * 2 / 1e6, 2))        # each conv reads and writes one map
    img = (seeded_images(B, S, S, seed=2) * 255).to(torch.uint8).to(DEV)
    pieces['yolov6n_forward_decode'] = Captured(lambda: model(img), a.warmup)
    pieces['yolov6n_forward_decode_nms'] = Captured(lambda: ops.nms(model(img)[0], 0.25, 0.7, None, False, False, 300, 30000, 7680), a.warmup)
    if not a.no_train:
        from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
        tm = seed_state_dict_(DetectionModel(get_config('yolov6', 'n', 80), verbose=False), 0).to(DEV)
        lab = seeded_labels(B, 80, seed=3, max_boxes=8, min_boxes=2)
        pieces['yolov6n_train_step'] = Stepper(DetectionTrainer(tm, lr0=0.01, amp=True, graph=True, batch_size=B, nb=100, epochs=3), dict(img=img, **lab))
    rounds = {k: [] for k in pieces}
    for _ in range(a.rounds):
        ts = {k: [] for k in pieces}
        for _ in range(a.steps):
            for k, g in pieces.items():
                ts[k].append(timed(g, 1 if k.endswith('train_step') else a.reps))
        for k in pieces:
            rounds[k].append(med(ts[k]))
    out = {'batch': B, 'size': S, 'dtype': 'bf16', 'rounds': a.rounds, 'steps': a.steps, 'reps': a.reps, 'DECONV_BWD_FUSED': shipped,
           'DECONV_DX_FUSED_CLASSES': [list(c) for c in ops.DECONV_DX_FUSED_CLASSES], 'DECONV_DW_FUSED_CLASSES': [list(c) for c in ops.DECONV_DW_FUSED_CLASSES]}
    spread = lambda k: (max(rounds[k]) - min(rounds[k])) / med(rounds[k])
    tbs = lambda mb, t: round(mb * 1e6 / (t * 1e-3) / 1e12, 3)
    for key, row in meta.items():
        if key.startswith('deconv_'):
            tc, tf = med(rounds[key + '_composed']), med(rounds[key + '_fused'])
            row.update(composed_us=round(tc * 1e3, 2), composed_spread=round(spread(key + '_composed'), 4), fused_us=round(tf * 1e3, 2),
                       fused_spread=round(spread(key + '_fused'), 4), fused_TB_per_s=tbs(row['MB'], tf), composed_TB_per_s=tbs(row['MB'], tc),
                       fused_pays=bool(tf < tc * (1 - spread(key + '_composed') - spread(key + '_fused'))))
        else:
            t = med(rounds[key])
            row.update(us=round(t * 1e3, 2), spread=round(spread(key), 4), us_per_conv=round(t * 1e3 / row['n'], 2), TB_per_s=tbs(row['MB'], t))
        out[key] = row
    for k in pieces:
        if k.startswith('yolov6n'):
            t = med(rounds[k])
            out[k] = dict(us=round(t * 1e3, 2), spread=round(spread(k), 4), images_per_s=round(B / (t * 1e-3), 1))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
