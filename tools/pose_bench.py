"""Per-batch times of pose inference at B = 32, 640x640, bf16, seeded weights: the whole forward, the Pose head alone with its keypoint branch on
the MFMA kernel over zero-padded panels (ops.POSE_PAD_MFMA, the default) and with the branch sent through mgdt_conv2d_direct_fwd, and the two
pose kernels on their own against their byte counts.

    python tools/pose_bench.py [--model yolov8-pose] [--batch 32] [--imgsz 640] [--steps 20] [--warmup 5]

The two head variants run in the same process, alternating step by step, on the same captured head inputs; every time is a median of HIP-event
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
from mgdt_yolo_amd.nn.tasks import PoseModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='yolov8-pose')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = 'cuda:0'
    m = seed_state_dict_(PoseModel(get_config(a.model, 'n'), verbose=False), 0).eval().to(dev).fuse().set_compute_dtype(torch.bfloat16)
    head = m.model[-1]
    x = seeded_images(a.batch, a.imgsz, a.imgsz, seed=7).to(dev).to(torch.bfloat16)
    seen = {}
    hook = head.register_forward_pre_hook(lambda mod, args: seen.__setitem__('x', [t.clone() for t in args[0]]))
    with torch.no_grad():
        pred = m(x)[0]
    hook.remove()
    feats = seen['x']

    def run_head(pad):
        ops.POSE_PAD_MFMA = pad
        try:
            with torch.no_grad():
                head(list(feats))
        finally:
            ops.POSE_PAD_MFMA = True

    def run_model():
        with torch.no_grad():
            m(x)

    for _ in range(a.warmup):
        run_model(); run_head(True); run_head(False)
    torch.cuda.synchronize()
    t_model, t_pad, t_direct = [], [], []
    for _ in range(a.steps):
        t_model.append(timed(run_model))
        t_pad.append(timed(lambda: run_head(True)))
        t_direct.append(timed(lambda: run_head(False)))
    # the two pose kernels alone
    nk, nd = head.nk, head.kpt_shape[1]
    with torch.no_grad():
        kps = [head._kpt_branch(i, feats[i]) for i in range(head.nl)]
    y = pred[:, :4 + head.nc].contiguous()
    strides = [float(s) for s in head.stride.tolist()]
    t_cat = [timed(lambda: ops.pose_concat(y, kps, strides, nk, nd)) for _ in range(a.warmup + a.steps)][a.warmup:]
    b, rows, A = y.shape
    cat_bytes = b * A * (2 * rows * 4 + nk * 8) + sum(t.numel() * t.element_size() for t in kps)
    md = 300
    nrows = torch.rand(b, md, 6 + nk, device=dev) * a.imgsz
    counts = torch.full((b,), md, dtype=torch.int32, device=dev)
    meta = torch.tensor([ops.pose_scale_meta((a.imgsz, a.imgsz), (480, 640))] * b, dtype=torch.float32).to(dev)
    t_scale = [timed(lambda: ops.pose_scale(nrows, counts, meta, nk, nd)) for _ in range(a.warmup + a.steps)][a.warmup:]
    scale_bytes = 2 * nrows.numel() * 4
    med = statistics.median
    print(json.dumps({'model': a.model, 'batch': a.batch, 'imgsz': a.imgsz, 'steps': a.steps, 'dtype': 'bf16',
                      'forward_ms': round(med(t_model), 4), 'head_padded_mfma_ms': round(med(t_pad), 4), 'head_direct_ms': round(med(t_direct), 4),
                      'head_direct_over_padded': round(med(t_direct) / med(t_pad), 3),
                      'pose_concat_ms': round(med(t_cat), 4), 'pose_concat_bytes': cat_bytes,
                      'pose_concat_fraction_of_hbm_peak': round(cat_bytes / (med(t_cat) * 1e-3) / HBM_PEAK, 4),
                      'pose_scale_ms': round(med(t_scale), 4), 'pose_scale_bytes': scale_bytes,
                      'pose_scale_fraction_of_hbm_peak': round(scale_bytes / (med(t_scale) * 1e-3) / HBM_PEAK, 4)}))


if __name__ == '__main__':
    main()
