"""Times of the YOLOv5 pieces on one MI355X, bf16, B = 32 at 640 x 640: the one-launch C3 route (merged [cv1 | cv2] launch + mode CSP_C3 of
mgdt_csp_block_fwd) against the composed route for the yolov5n blocks the kernel covers (layers 2, 4, 13, 17, 20), the stem route (space-to-depth launch, then the 3x3 convolution over its map), and yolov5n forward + decode + NMS per batch as
one captured graph.

    python tools/c3_bench.py [--rounds 7] [--steps 30] [--reps 10] [--warmup 5] [--batch 32] [--size 640]

Every piece is captured once (torch.cuda.graph) and replayed; one measurement is `reps` back-to-back replays between two HIP events, divided by `reps`;
the pieces alternate measurement by measurement; a round's figure is the median of `steps` measurements and the spread of a piece is (max - min) / median
over the rounds' medians.  A block's `fused_pays` is true where the fused median is below the composed one by more than the sum of the two spreads: the rule
by which ops.C3_FUSED_CLASSES is filled.  The model rows run with ops.C3_FUSED_CLASSES as the library ships it.  Prints one JSON line."""
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
from mgdt_yolo_amd.nn.modules import C3, Conv  # noqa: E402
from mgdt_yolo_amd.nn.tasks import DetectionModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402

DEV = 'cuda:0'
med = statistics.median
# (layer of yolov5n, c1, c2, map side at 640 / this, n, shortcut)
BLOCKS = [(2, 32, 32, 4, 1, True), (4, 64, 64, 8, 2, True), (13, 256, 128, 16, 1, False), (17, 128, 64, 8, 1, False), (20, 128, 128, 16, 1, False)]


class Captured:
    """One piece captured into a graph.  The object owns everything its graph reads and writes - the callable (and through it the module, its packed
    panels and the input tensors) and the outputs of the captured call - for as long as the graph can be replayed: torch.cuda.graph() empties the caching
    allocator when the NEXT capture begins, so memory that only a dead closure owned would be returned to the driver under a live graph."""

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


def captured(fn, warmup):
    return Captured(fn, warmup)


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
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    a = ap.parse_args()
    B, S, bf = a.batch, a.size, torch.bfloat16
    gen = torch.Generator().manual_seed(1)
    pieces, meta = {}, {}
    for layer, c1, c2, red, n, sc in BLOCKS:
        m = seed_state_dict_(C3(c1, c2, n, sc), layer).eval().to(DEV)
        m.apply(lambda s: setattr(s, '_cdtype', bf) if hasattr(s, 'out_dtype') else None)
        x = torch.randn(B, c1, S // red, S // red, generator=gen).to(DEV).to(bf).contiguous(memory_format=torch.channels_last)
        key = f'c3_layer{layer}'
        shipped = ops.C3_FUSED_CLASSES
        for route, classes in (('composed', ()), ('fused', None)):          # the route is chosen while the piece is warmed and captured
            ops.C3_FUSED_CLASSES = classes
            try:
                pieces[f'{key}_{route}'] = captured(lambda m=m, x=x: m(x), a.warmup)
            finally:
                ops.C3_FUSED_CLASSES = shipped
        meta[key] = dict(c1=c1, c2=c2, wd=c2 // 2, map=S // red, n=n, shortcut=sc)
    stem = seed_state_dict_(Conv(3, 16, 6, 2, 2), 0).eval().to(DEV)
    stem._cdtype = bf
    img = (seeded_images(B, S, S, seed=2) * 255).to(torch.uint8).to(DEV)
    sd = ops.space_to_depth2(img, bf)
    pieces['stem_space_to_depth2'] = captured(lambda: ops.space_to_depth2(img, bf, out=sd), a.warmup)
    pieces['stem_conv3x3'] = captured(lambda: ops.conv2d(sd, stem._stem6_packed(bf, False), 1, ops.ACT_SILU), a.warmup)
    meta['stem_space_to_depth2'] = dict(MB=round((img.numel() + sd.numel() * 2) / 1e6, 2))
    model = seed_state_dict_(DetectionModel(get_config('yolov5', 'n', 80), verbose=False), 0).eval().to(DEV).set_compute_dtype(bf)
    pieces['yolov5n_forward_decode'] = captured(lambda: model(img), a.warmup)
    pieces['yolov5n_forward_decode_nms'] = captured(lambda: ops.nms(model(img)[0], 0.25, 0.7, None, False, False, 300, 30000, 7680), a.warmup)
    rounds = {k: [] for k in pieces}
    for _ in range(a.rounds):
        ts = {k: [] for k in pieces}
        for _ in range(a.steps):
            for k, g in pieces.items():
                ts[k].append(timed(g, a.reps))
        for k in pieces:
            rounds[k].append(med(ts[k]))
    out = {'batch': B, 'size': S, 'dtype': 'bf16', 'rounds': a.rounds, 'steps': a.steps, 'reps': a.reps}
    spread = lambda k: (max(rounds[k]) - min(rounds[k])) / med(rounds[k])
    for key, row in meta.items():
        if not key.startswith('c3_'):
            continue
        tc, tf = med(rounds[key + '_composed']), med(rounds[key + '_fused'])
        row.update(composed_us=round(tc * 1e3, 2), composed_spread=round(spread(key + '_composed'), 4), fused_us=round(tf * 1e3, 2),
                   fused_spread=round(spread(key + '_fused'), 4), fused_pays=bool(tf < tc * (1 - spread(key + '_composed') - spread(key + '_fused'))))
        out[key] = row
    out['C3_FUSED_CLASSES'] = None if ops.C3_FUSED_CLASSES is None else [list(c) for c in ops.C3_FUSED_CLASSES]
    for k in pieces:
        if k.startswith('c3_'):
            continue
        t = med(rounds[k])
        row = dict(meta.get(k, {}))
        row['us'] = round(t * 1e3, 2)
        row['spread'] = round(spread(k), 4)
        if 'MB' in row:
            row['TB_per_s'] = round(row['MB'] * 1e6 / (t * 1e-3) / 1e12, 3)
        if k.startswith('yolov5n'):
            row['images_per_s'] = round(B / (t * 1e-3), 1)
        out[k] = row
    print(json.dumps(out))


if __name__ == '__main__':
    main()
