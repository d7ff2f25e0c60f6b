"""Per-batch times of classification inference with seeded yolov8n-cls weights, bf16: the fused eval head (mgdt_classify_pool_fwd +
mgdt_classify_linear_fwd) against the unfused chain built from the other kernels (1x1 conv, adaptive_avgpool, the linear as a 1x1 conv, softmax) at
B = 32 on the final maps 7x7 (224^2 input) and 20x20 (640^2 input), and the whole forward in images/s at 224^2, B = 64.

    python tools/cls_bench.py [--batch 32] [--steps 30] [--warmup 5] [--nc 1000]

The two head variants run in the same process, alternating launch by launch, on the same seeded head input; every time is a median of HIP-event
intervals around the call (stream-ordered, no host time inside).  Prints one JSON line."""
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
from mgdt_yolo_amd.nn.tasks import ClassificationModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--fwd-batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--nc', type=int, default=1000)
    a = ap.parse_args()
    dev = 'cuda:0'
    m = seed_state_dict_(ClassificationModel(get_config('yolov8-cls', 'n', a.nc), verbose=False), 0).eval().to(dev).fuse().set_compute_dtype(torch.bfloat16)
    head = m.model[-1]
    c1 = head.conv.conv.in_channels
    med = statistics.median
    out = {'model': 'yolov8n-cls', 'nc': a.nc, 'batch': a.batch, 'steps': a.steps, 'dtype': 'bf16'}

    def run_head(x, fused):
        ops.FUSED_CLS_HEAD = fused
        try:
            with torch.no_grad():
                head(x)
        finally:
            ops.FUSED_CLS_HEAD = True

    for hw in (7, 20):
        x = torch.randn(a.batch, c1, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        for _ in range(a.warmup):
            run_head(x, True); run_head(x, False)
        torch.cuda.synchronize()
        tf, tu = [], []
        for _ in range(a.steps):
            tf.append(timed(lambda: run_head(x, True)))
            tu.append(timed(lambda: run_head(x, False)))
        out[f'head_{hw}x{hw}_fused_ms'] = round(med(tf), 4)
        out[f'head_{hw}x{hw}_unfused_ms'] = round(med(tu), 4)
        out[f'head_{hw}x{hw}_unfused_over_fused'] = round(med(tu) / med(tf), 3)
    x = seeded_images(a.fwd_batch, 224, 224, seed=7).to(dev).to(torch.bfloat16)

    def run_model():
        with torch.no_grad():
            m(x)

    for _ in range(a.warmup):
        run_model()
    torch.cuda.synchronize()
    t = med([timed(run_model) for _ in range(a.steps)])
    out.update({'forward_batch': a.fwd_batch, 'forward_224_ms': round(t, 4), 'forward_224_images_per_s': round(a.fwd_batch / (t * 1e-3), 1)})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
