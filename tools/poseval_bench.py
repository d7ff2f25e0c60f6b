"""Keypoint matching of a validation batch: the OKS launch (mgdt_kpt_iou_fwd) plus the match launch on its matrix (mgdt_val_match_iou_fwd).

    python tools/poseval_bench.py [--batch 32] [--dets 300] [--labels 20] [--nkpt 17] [--ndim 3] [--steps 200] [--warmup 20]

Times are HIP-event medians over `--steps` calls after warm-up, each call timed on its own and the two launches also as one pair, with the
predictions read in place from NMS-layout rows (stride 6 + nk).  A second figure times `--steps` back-to-back pairs between one pair of events
(the launch gaps overlap there).  Prints one JSON line.  Seeded random keypoints: the time does not depend on their values, except that invisible
label keypoints (a quarter here) are skipped.  There is no earlier path for the same work in this package to compare against."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402


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
    ap.add_argument('--nkpt', type=int, default=17)
    ap.add_argument('--ndim', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    a = ap.parse_args()
    dev = 'cuda:0'
    b, nd, nl, nkpt, ndim = a.batch, a.dets, a.labels, a.nkpt, a.ndim
    g = torch.Generator(device=dev).manual_seed(7)
    rows = torch.rand(b, nd, 6 + nkpt * ndim, device=dev, generator=g) * 200
    rows[:, :, 5] = 0
    gk = torch.rand(b, nl, nkpt, 3, device=dev, generator=g) * 200
    gk[..., 2] = (torch.rand(b, nl, nkpt, device=dev, generator=g) > 0.25).float()
    labels = torch.zeros(b, nl, 5, device=dev)
    area = torch.rand(b, nl, device=dev, generator=g) * 5000 + 100
    sigma = torch.full((nkpt,), 0.05, device=dev)
    counts = torch.full((b,), nd, dtype=torch.int32, device=dev)
    nlab = torch.full((b,), nl, dtype=torch.int32, device=dev)
    iouv = torch.linspace(0.5, 0.95, 10, device=dev)
    oks_fn = lambda: ops.kpt_iou_batch(rows, counts, nd, gk, area, nlab, sigma)
    oks = oks_fn()
    match_fn = lambda: ops.val_match_iou(oks, rows, counts, labels, nlab, iouv)
    pair = lambda: ops.val_match_iou(oks_fn(), rows, counts, labels, nlab, iouv)
    for _ in range(a.warmup):
        pair()
    torch.cuda.synchronize()
    t = {'kpt_iou': [], 'val_match_iou': [], 'pair': []}
    for _ in range(a.steps):
        t['kpt_iou'].append(timed(oks_fn)[0])
        t['val_match_iou'].append(timed(match_fn)[0])
        t['pair'].append(timed(pair)[0])
    stream_ms = timed(lambda: [pair() for _ in range(a.steps)])[0] / a.steps
    out_bytes = b * nl * nd * 4
    print(json.dumps({'batch': b, 'dets': nd, 'labels': nl, 'nkpt': nkpt, 'ndim': ndim, 'steps': a.steps,
                      'ms_median': {k: round(statistics.median(v), 4) for k, v in t.items()}, 'ms_min': {k: round(min(v), 4) for k, v in t.items()},
                      'ms_per_pair_back_to_back': round(stream_ms, 4), 'oks_matrix_bytes': out_bytes,
                      'pred_keypoint_bytes': b * nd * nkpt * ndim * 4}), flush=True)


if __name__ == '__main__':
    main()
