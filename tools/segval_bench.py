"""Mask IoU of a validation batch: the batch kernel (mgdt_mask_iou_fwd) against the reference's own formulation in torch ops on the same device.

    python tools/segval_bench.py [--batch 32] [--dets 300] [--labels 20] [--sizes 160 640] [--steps 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/segval_bench.py --steps 20 --only kernel      # the kernels' own times

Yardstick (yolo/v8/segment/val.py:141-149 + yolo/utils/metrics.py:131-147, per image as the reference loops): the index map repeated and compared
into (nl, H, W) float masks, the uint8 predictions converted to float, `torch.matmul`, sums, divide.  Both paths run alternately in one process
after warm-up; times are HIP-event medians.  Prints one JSON line per size: both times, their ratio, the predicted-mask bytes and the share of the
8 TB/s HBM peak the kernel's time corresponds to (the whole call: workspace clear + MFMA kernel + final pass).  Seeded random 0 / 1 masks: the
time does not depend on the mask content."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12


def reference_path(masks, idx, nd, nl, eps=1e-7):
    out = []
    for i in range(idx.shape[0]):
        gt = idx[i:i + 1].float()
        index = torch.arange(nl, device=gt.device).view(nl, 1, 1) + 1
        gt = torch.where(gt.repeat(nl, 1, 1) == index, 1.0, 0.0).view(nl, -1)
        pm = masks[i * nd:(i + 1) * nd].float().view(nd, -1)
        inter = torch.matmul(gt, pm.T).clamp_(0)
        union = (gt.sum(1)[:, None] + pm.sum(1)[None]) - inter
        out.append(inter / (union + eps))
    return torch.stack(out)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dets', type=int, default=300)
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--sizes', type=int, nargs='+', default=[160, 640])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=['kernel', 'reference'], default=None, help='one path only (for a run under rocprofv3)')
    a = ap.parse_args()
    dev = 'cuda:0'
    b, nd, nl = a.batch, a.dets, a.labels
    for s in a.sizes:
        g = torch.Generator(device=dev).manual_seed(s)
        masks = (torch.rand(b * nd, s, s, device=dev, generator=g) < 0.3).to(torch.uint8)
        idx = torch.randint(0, nl + 1, (b, s, s), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
        counts = torch.full((b,), nd, dtype=torch.int32, device=dev)
        nlab = torch.full((b,), nl, dtype=torch.int32, device=dev)
        offsets = ops.exclusive_offsets(counts)
        kernel = lambda: ops.mask_iou_batch(masks, counts, offsets, nd, idx, nlab, nl, index_map=True)
        reference = lambda: reference_path(masks, idx, nd, nl)
        paths = [(n, f) for n, f in (('kernel', kernel), ('reference', reference)) if a.only in (None, n)]
        for _ in range(a.warmup):
            res = {n: f() for n, f in paths}
        torch.cuda.synchronize()
        if a.only is None:
            assert torch.equal(res['kernel'], res['reference']), 'the two paths disagree'
        times = {n: [] for n, _ in paths}
        for _ in range(a.steps):
            for n, f in paths:
                times[n].append(timed(f)[0])
        med = {n: statistics.median(v) for n, v in times.items()}
        line = {'batch': b, 'dets': nd, 'labels': nl, 'size': s, 'steps': a.steps, 'ms': {n: round(v, 4) for n, v in med.items()},
                'pred_mask_bytes': masks.numel(), 'gt_bytes': idx.numel()}
        if 'kernel' in med:
            line['kernel_fraction_of_hbm_peak'] = round((masks.numel() + idx.numel()) / (med['kernel'] * 1e-3) / HBM_PEAK, 4)
        if len(med) == 2:
            line['reference_over_kernel'] = round(med['reference'] / med['kernel'], 2)
        print(json.dumps(line), flush=True)
        del masks, idx
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
