"""Throughput of augmented bf16 inference (model(x, augment=True) + NMS at the predictor's settings) next to the plain forward + NMS on the
same run: B = 32, 640x640, every step a replay of a captured graph, R resident batches cycled through (bench.py's protocol, simplified).

    python tools/tta_bench.py [--models mspa_c2f_gd_yolov8 yolov8] [--batch 32] [--imgsz 640] [--steps 50] [--warmup 5] [--resident 4]

Prints one JSON line per model: images/sec and ms per batch of both forms and their ratio.  --resample: instead, time mgdt_scale_img_fwd
alone (B x 3 x imgsz^2 uint8 -> the flipped 0.83 pass of yolov8's gs = 32, bf16; run it under `rocprofv3 --kernel-trace --stats` for the
kernel's own time) and print its bytes and its share of the HBM peak."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.models import get_config  # noqa: E402
from mgdt_yolo_amd.nn.tasks import DetectionModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402


def timed(model, xs, augment, steps, warmup):
    graphs = []
    for x in xs:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                y = model(x, augment=augment)[0]
                ops.nms(y, 0.25, 0.7, None, False, False, 300, 30000, 7680.0)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            y = model(x, augment=augment)[0]
            out = ops.nms(y, 0.25, 0.7, None, False, False, 300, 30000, 7680.0)
        graphs.append((g, y, out))
    for i in range(warmup):
        graphs[i % len(graphs)][0].replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        graphs[i % len(graphs)][0].replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    anchors = graphs[0][1].shape[-1]
    del graphs
    return ms, anchors


def resample(a):
    dev = torch.device('cuda:0')
    xs = [torch.randint(0, 256, (a.batch, 3, a.imgsz, a.imgsz), dtype=torch.uint8, device=dev) for _ in range(a.resident)]
    hs = int(a.imgsz * 0.83)
    hp = math.ceil(a.imgsz * 0.83 / 32) * 32                  # scale_img's padding (gs = 32)
    for i in range(a.warmup):
        ops.scale_img(xs[i % len(xs)], hs, hs, hp, hp, True, torch.bfloat16)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.steps):
        ops.scale_img(xs[i % len(xs)], hs, hs, hp, hp, True, torch.bfloat16)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.steps * 1e3
    nbytes = a.batch * 3 * (a.imgsz * a.imgsz + 2 * hp * hp)
    print(json.dumps({'kernel': 'scale_img_fwd', 'in': [a.batch, 3, a.imgsz, a.imgsz, 'uint8'], 'out': [a.batch, 3, hp, hp, 'bf16'], 'us_event': round(us, 2),
                      'MB': round(nbytes / 1e6, 1), 'GB_per_s': round(nbytes / us / 1e3, 1), 'hbm_peak_share': round(nbytes / us / 1e3 / 8000.0, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['mspa_c2f_gd_yolov8', 'yolov8'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--resident', type=int, default=4)
    ap.add_argument('--resample', action='store_true')
    a = ap.parse_args()
    if a.resample:
        return resample(a)
    dev = torch.device('cuda:0')
    xs = [seeded_images(a.batch, a.imgsz, a.imgsz, seed=100 + i).to(dev).to(torch.bfloat16) for i in range(a.resident)]
    for name in a.models:
        m = DetectionModel(get_config(name, 'n', 80), verbose=False)
        m = seed_state_dict_(m, 0).eval().to(dev).half()
        ms_plain, a_plain = timed(m, xs, False, a.steps, a.warmup)
        ms_tta, a_tta = timed(m, xs, True, a.steps, a.warmup)
        print(json.dumps({'model': f'{name} n', 'batch': a.batch, 'imgsz': a.imgsz, 'dtype': 'bf16', 'captured': True,
                          'plain': {'ms_per_batch': round(ms_plain, 4), 'images_per_sec': round(a.batch * 1e3 / ms_plain, 1), 'anchors': a_plain},
                          'augment': {'ms_per_batch': round(ms_tta, 4), 'images_per_sec': round(a.batch * 1e3 / ms_tta, 1), 'anchors': a_tta},
                          'augment_over_plain_time': round(ms_tta / ms_plain, 3)}))


if __name__ == '__main__':
    main()
