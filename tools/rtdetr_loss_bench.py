"""Times of the RT-DETR criterion and of the validator's post-processing at B = 32, nq = 300, nc = 80, 7 layers (the encoder's outputs + 6 decoder
layers) and about 10 ground truths per image: the match launch (mgdt_detr_match_fwd: costs + exact assignment of every layer and image), the loss
launch with head gradients (mgdt_detr_loss_fwd) and the validator rows (mgdt_rtdetr_val_post_fwd) - and, for scale, the one-batch forward of
`yolov8-rtdetr` n (fp32, one captured graph) measured in the same call, alternating step by step.

    python tools/rtdetr_loss_bench.py [--batch 32] [--steps 50] [--warmup 10] [--no-model]

Every time is a median of HIP-event intervals around the call (stream-ordered, no host time inside the window; the calls are repeated `inner`
times per window so that a window is not a single short launch).  Inputs are seeded (predictions as in tests/rtdetr_loss_ref.py: uniform boxes,
normal logits).  There is no earlier device implementation to compare against: the numbers are a record.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--nq', type=int, default=300)
    ap.add_argument('--nc', type=int, default=80)
    ap.add_argument('--layers', type=int, default=7)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    r = np.random.RandomState(0)
    l, b, nq, nc = a.layers, a.batch, a.nq, a.nc
    groups = r.randint(4, 17, b).tolist()                       # about 10 per image
    g = sum(groups)
    box = lambda *s: np.concatenate([r.uniform(0.1, 0.9, s + (2,)), r.uniform(0.05, 0.4, s + (2,))], -1).astype(np.float32)
    boxes, logits = torch.from_numpy(box(l, b, nq)).to(dev), torch.from_numpy(r.normal(-2, 1.5, (l, b, nq, nc)).astype(np.float32)).to(dev)
    gt_boxes, gt_cls = torch.from_numpy(box(g)).to(dev), torch.from_numpy(r.randint(0, nc, g).astype(np.int32)).to(dev)
    gt_off = torch.from_numpy(np.concatenate([[0], np.cumsum(groups)]).astype(np.int32)).to(dev)
    scores = torch.sigmoid(logits[-1]).contiguous()

    match = lambda: ops.detr_match(boxes, logits, gt_boxes, gt_cls, groups, gt_off=gt_off)
    assign = match()
    loss = lambda: ops.detr_loss(boxes, logits, gt_boxes, gt_cls, assign, g, want_grads=True)
    loss_nograd = lambda: ops.detr_loss(boxes, logits, gt_boxes, gt_cls, assign, g, want_grads=False)
    post = lambda: ops.rtdetr_val_post(boxes[-1], scores)
    calls = {'match_ms': match, 'loss_with_grads_ms': loss, 'loss_ms': loss_nograd, 'val_post_ms': post}

    graph = None
    if not a.no_model:
        from mgdt_yolo_amd.models import get_config
        from mgdt_yolo_amd.nn.tasks import RTDETRDetectionModel
        from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images
        m = seed_state_dict_(RTDETRDetectionModel(get_config('yolov8-rtdetr', 'n'), verbose=False), 0).eval().to(dev).fuse()
        x = seeded_images(b, 640, 640, seed=7).to(dev)
        with torch.no_grad():
            for _ in range(3):
                m(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            m(x)
        graph.replay()
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    tm = []
    for _ in range(a.steps):
        for k, fn in calls.items():
            t[k].append(timed(fn, a.inner))
        if graph is not None:
            tm.append(timed(graph.replay, 1))
    out = {'batch': b, 'nq': nq, 'nc': nc, 'layers': l, 'ground_truths': g, 'steps': a.steps, 'inner': a.inner}
    for k in calls:
        out[k] = round(statistics.median(t[k]), 4)
        out[k.replace('_ms', '_min_max_ms')] = [round(min(t[k]), 4), round(max(t[k]), 4)]
    out['criterion_ms'] = round(out['match_ms'] + out['loss_with_grads_ms'], 4)
    if tm:
        out['model_graph_fp32_ms'] = round(statistics.median(tm), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
