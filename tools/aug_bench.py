"""Time of the training augmentation's two launches (mgdt_aug_warp_fwd, mgdt_aug_labels_fwd) and of TrainAugment.apply as a whole, next to the
bf16 captured training step of the same process that consumes the batch.

    python tools/aug_bench.py [--batch 32] [--imgsz 640] [--pool 256] [--labels 20] [--steps 20] [--warmup 5] [--no-train]

Seeded and synthetic: a pool of `--pool` random-pixel images whose long side is imgsz (short side 0.6 .. 1.0 of it) with `--labels` boxes each,
default hyp (mosaic 1.0, scale 0.5, translate 0.1, HSV on).  Every time is a median of HIP-event intervals around one call (stream-ordered) after
the warm-up calls; `apply` includes the host part of the call (record check, the copy into pinned memory) as far as it delays the stream.  Every
timed call gets freshly drawn parameters.  Bytes: what each launch must move at least - the warp writes B * 3 * S * S bytes and reads four source
pixels of 3 bytes per output pixel from the pool (mostly cache hits between neighbours: not counted), the records and tables are B * 992 bytes.
The reference's cv2 pipeline cannot be timed here (cv2 is not installed), so there is no comparison with it.  Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.yolo.data.augment import ImagePool, TrainAugment  # noqa: E402

DEV = 'cuda:0'


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return dict(ms=statistics.median(ts), ms_min=min(ts), ms_max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--pool', type=int, default=256)
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-train', action='store_true', help='skip the training step (a kernel trace of the two launches alone)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('aug_bench needs the MI355X: there is nothing to time on a CPU')
    B, S, nc = a.batch, a.imgsz, 80
    rng = np.random.default_rng(0)
    images, labels = [], []
    for i in range(a.pool):
        short = int(rng.integers(int(0.6 * S), S + 1))
        h, w = (S, short) if i % 2 else (short, S)
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        labels.append(np.concatenate([rng.integers(0, nc, (a.labels, 1)), rng.uniform(0.1, 0.9, (a.labels, 2)), rng.uniform(0.05, 0.4, (a.labels, 2))], 1).astype(np.float32))
    pool = ImagePool(images, labels, S, DEV)
    aug = TrainAugment(pool, max_labels=4 * a.labels)
    random.seed(0)
    np.random.seed(0)
    draw = lambda: aug.sample(rng.integers(0, a.pool, B))
    n = a.warmup + a.steps
    params = [draw() for _ in range(n)]
    res = dict(batch=B, imgsz=S, pool=a.pool, labels_per_image=a.labels, steps=a.steps, warmup=a.warmup, max_labels=aug.max_labels,
               pool_bytes=pool.pool_bytes)
    t_apply = [timed(lambda: aug.apply(p)) for p in params][a.warmup:]
    res['apply'] = stats(t_apply)
    # the two launches alone, on records that are already on the device
    rb = B * ops.AUG_RECORD.itemsize
    t_warp, t_lab = [], []
    for k, p in enumerate(params):
        aug.load(p)
        aug._dev.copy_(aug._host, non_blocking=True)
        torch.cuda.synchronize()
        tw = timed(lambda: ops.aug_warp(pool.pixels, pool.table_dev, pool.table, aug._dev[:rb], p.records, aug._dev[rb:], B, S))
        tl = timed(lambda: ops.aug_labels(pool.labels, pool.n_labels, pool.table_dev, pool.table, aug._dev[:rb], p.records, B, S, aug.max_labels))
        if k >= a.warmup:
            t_warp.append(tw)
            t_lab.append(tl)
    res['warp'], res['labels'] = stats(t_warp), stats(t_lab)
    out_bytes = B * 3 * S * S
    res['warp_out_bytes'] = out_bytes
    res['warp_out_GBps'] = out_bytes / (res['warp']['ms'] * 1e-3) / 1e9
    res['param_bytes'] = B * (ops.AUG_RECORD.itemsize + 768)
    res['labels_out_bytes'] = B * (2 * aug.max_labels * 5 * 4 + 8)
    batch = aug.apply(params[-1])
    res['boxes_per_image'] = float(batch['nlabels'].float().mean().item())
    res['flags'] = int(batch['flags'].max().item())
    if not a.no_train:
        from mgdt_yolo_amd.models import get_config
        from mgdt_yolo_amd.nn.tasks import DetectionModel
        from mgdt_yolo_amd.seeding import seed_state_dict_
        from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
        m = seed_state_dict_(DetectionModel(get_config('mspa_c2f_gd_yolov8', 'n', nc), verbose=False), 0).to(DEV)
        tr = DetectionTrainer(m, lr0=0.01, amp=True, graph=True)
        for _ in range(a.warmup):
            tr.step(batch)
        res['train_step_bf16_graph'] = stats([timed(lambda: tr.step(batch)) for _ in range(a.steps)])
        res['train_step_captured'] = bool(tr._graphs)
        res['apply_share_of_step'] = res['apply']['ms'] / res['train_step_bf16_graph']['ms']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
