"""Confusion matrix + counting metrics of a validation batch (mgdt_val_confusion_fwd, one launch) beside the validation chain that was there before
it: NMS (mgdt_nms_fwd, validator settings) + scale_boxes per image + mgdt_val_match_fwd over the same batch.

    python tools/valstats_bench.py [--batch 32] [--dets 300] [--labels 40] [--anchors 8400] [--steps 200] [--warmup 20]

Times are HIP-event medians over `--steps` calls after warm-up, each call timed on its own, for nc = 2 and nc = 80.  The new launch reads the
NMS output of the same seeded predictions; labels are jittered copies of each image's first `--labels` detections, so both matchings find pairs
(matches cost atomics).  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.yolo.utils import ops as uops  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def one(a, nc):
    dev = 'cuda:0'
    b, nd, nl, A = a.batch, a.dets, a.labels, a.anchors
    H, W = 640, 640
    g = torch.Generator(device=dev).manual_seed(7)
    pred = torch.empty(b, 4 + nc, A, device=dev)
    pred[:, 0] = torch.rand(b, A, device=dev, generator=g) * W
    pred[:, 1] = torch.rand(b, A, device=dev, generator=g) * H
    pred[:, 2:4] = torch.rand(b, 2, A, device=dev, generator=g) * 110 + 10
    expo = math.log(0.001) / math.log(1.0 - min(4000.0 / (A * nc), 0.5))      # about 4000 candidates per image over the validator's conf 0.001
    pred[:, 4:] = torch.rand(b, nc, A, device=dev, generator=g) ** expo
    pred = pred.contiguous()
    nms_fn = lambda: ops.nms(pred, 0.001, 0.7, None, False, True, nd, 30000, 7680.0)
    out, _, counts = nms_fn()
    torch.cuda.synchronize()
    ndet_host = counts.cpu().tolist()
    labels = torch.zeros(b, nl, 5, device=dev)
    labels[:, :, 0] = out[:, :nl, 5]
    labels[:, :, 1:] = out[:, :nl, :4] + torch.randn(b, nl, 4, device=dev, generator=g) * 4
    nlab = torch.full((b,), nl, dtype=torch.int32, device=dev)
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    matrix = torch.zeros(nc + 1, nc + 1, dtype=torch.int32, device=dev)
    slots = torch.zeros(nc, ops.COUNT_SLOTS, dtype=torch.int64, device=dev)

    def scale_fn():
        for i in range(b):
            uops.scale_boxes((H, W), out[i], (H, W), ratio_pad=((1.0, 1.0), (0.0, 0.0)))        # gain 1, no pad: the boxes stay what they are

    match_fn = lambda: ops.val_match(out, counts, labels, nlab, iouv)
    new_fn = lambda: ops.val_confusion(out, counts, labels, nlab, nc, matrix=matrix, counts=slots)
    cm_fn = lambda: ops.val_confusion(out, counts, labels, nlab, nc, matrix=matrix)
    cnt_fn = lambda: ops.val_confusion(out, counts, labels, nlab, nc, counts=slots)
    fns = {'nms': nms_fn, 'scale_boxes': scale_fn, 'val_match': match_fn, 'val_confusion': new_fn, 'val_confusion_matrix_only': cm_fn,
           'val_confusion_counts_only': cnt_fn}
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(a.steps):
        for k, f in fns.items():
            t[k].append(timed(f)[0])
    med = {k: round(statistics.median(v), 4) for k, v in t.items()}
    chain = med['nms'] + med['scale_boxes'] + med['val_match']
    return {'nc': nc, 'ndet_min': min(ndet_host), 'ndet_max': max(ndet_host), 'ms_median': med, 'ms_min': {k: round(min(v), 4) for k, v in t.items()},
            'chain_ms': round(chain, 4), 'val_confusion_over_nms': round(med['val_confusion'] / med['nms'], 4),
            'val_confusion_over_chain': round(med['val_confusion'] / chain, 4), 'matrix_sum': int(matrix.sum()), 'tp_sum': int(slots[:, 7].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dets', type=int, default=300)
    ap.add_argument('--labels', type=int, default=40)
    ap.add_argument('--anchors', type=int, default=8400)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    print(json.dumps({'batch': a.batch, 'dets': a.dets, 'labels': a.labels, 'anchors': a.anchors, 'steps': a.steps,
                      'results': [one(a, nc) for nc in (2, 80)]}), flush=True)


if __name__ == '__main__':
    main()
