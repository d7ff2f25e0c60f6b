"""Per-frame time of the tracker's one launch (mgdt_bytetrack_update) for a batch of streams, next to the NMS launch that feeds it.

    python tools/track_bench.py [--steps 50] [--warmup 10] [--scene typical|corner]

Two scenes, both seeded and synthetic (boxes on a jittered grid that drift a few pixels per frame, a share of them hidden each frame so that tracks
get lost and found, a few low scores for the second association):
  typical   B = 32 streams, about 60 detections per stream and frame (50 of 52 objects + 10 one-frame boxes that start nothing), about 50 live tracks
  corner    B = 32 streams at the capacity corner: 128 detections per frame and 128 slots, all in use
and the solver alone (mgdt_track_assign) on 32 dense uniform 128 x 128 matrices, the worst case of its serial phase.
The NMS time is `ops.nms` on a seeded B = 32 x (4 + 80) x 8400 prediction with about 60 kept rows per image, in the same process.

Every time is a median of HIP-event intervals around one call (stream-ordered, no host time inside) after the warm-up frames; the frames of the timed
window are consecutive frames of the scene, so every call does the work of a real frame.  Prints one JSON line."""
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
from mgdt_yolo_amd.tracker import BYTETracker, get_tracker_cfg  # noqa: E402

DEV = 'cuda:0'


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def scene(streams, objects, frames, hidden, spurious, seed, size=1920):
    """-> rows (frames, streams, objects, 6) fp32, counts (frames, streams) int32: `objects` boxes per stream, a share `hidden` of them absent per frame, plus
    `spurious` one-frame boxes per frame with a score between track_high_thresh and new_track_thresh (columns of the first association that start nothing)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(objects)))
    pitch = size / side
    gy, gx = np.divmod(np.arange(objects), side)
    c0 = np.stack([(gx + 0.5) * pitch, (gy + 0.5) * pitch], -1)[None] + rng.uniform(-0.1, 0.1, (streams, objects, 2)) * pitch
    wh = rng.uniform(0.5, 0.8, (streams, objects, 2)) * pitch
    v = rng.uniform(-2, 2, (streams, objects, 2))
    rows = np.zeros((frames, streams, objects + spurious, 6), np.float32)
    counts = np.zeros((frames, streams), np.int32)
    for f in range(frames):
        c = c0 + v * f + rng.uniform(-1, 1, c0.shape)
        score = np.where(rng.random((streams, objects)) < 0.1, rng.uniform(0.15, 0.45, (streams, objects)), rng.uniform(0.65, 0.95, (streams, objects)))
        r = np.concatenate([c - wh / 2, c + wh / 2, score[..., None], rng.integers(0, 2, (streams, objects, 1))], -1).astype(np.float32)
        keep = rng.random((streams, objects)) >= hidden if f else np.ones((streams, objects), bool)
        for b in range(streams):
            sc = rng.uniform(40, size - 40, (spurious, 2))
            sp = np.concatenate([sc - 15, sc + 15, rng.uniform(0.52, 0.58, (spurious, 1)), np.zeros((spurious, 1))], -1).astype(np.float32)
            k = np.concatenate([r[b][keep[b]], sp])
            k = k[np.argsort(-k[:, 4], kind='stable')]
            rows[f, b, :len(k)] = k
            counts[f, b] = len(k)
    return torch.from_numpy(rows).to(DEV), torch.from_numpy(counts).to(DEV)


def run_scene(streams, objects, hidden, spurious, capacity, steps, warmup, seed):
    rows, counts = scene(streams, objects, warmup + steps, hidden, spurious, seed)
    trk = BYTETracker(get_tracker_cfg(), streams=streams, device=DEV, capacity=capacity)
    times, flags = [], 0
    for f in range(warmup + steps):
        r, c = rows[f].contiguous(), counts[f].contiguous()
        if f < warmup:
            out = trk.update_batch(r, c)
        else:
            times.append(timed(lambda: trk.update_batch(r, c)))
            out = trk._last
        flags |= int(out[2].max().item())
    if flags:
        raise SystemExit(f'track_bench: a frame did not fit (flags {flags}): the scene is not what this tool means to time')
    live = [len(trk.state(b)['id']) for b in range(min(streams, 4))]
    return dict(ms=statistics.median(times), ms_min=min(times), ms_max=max(times), detections=float(counts[warmup:].float().mean().item()),
                live_tracks=live, rows_out=float(out[1].float().mean().item()), flags=flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--scene', choices=('all', 'typical', 'corner'), default='all', help='one scene alone and nothing else: for a kernel trace')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_bench needs the MI355X: there is nothing to time on a CPU')
    res = dict(streams=a.streams, steps=a.steps, warmup=a.warmup)
    if a.scene in ('all', 'typical'):
        res['typical'] = run_scene(a.streams, 52, 0.04, 10, ops.TRACK_CAP, a.steps, a.warmup, 1)
    if a.scene in ('all', 'corner'):
        res['corner'] = run_scene(a.streams, 128, 0.0, 0, ops.TRACK_CAP, a.steps, a.warmup, 2)
    if a.scene != 'all':
        print(json.dumps(res))
        return
    rng = np.random.default_rng(3)
    cost = torch.from_numpy(rng.uniform(0, 1, (a.streams, 128, 128)).astype(np.float32)).to(DEV)
    n = torch.full((a.streams,), 128, dtype=torch.int32, device=DEV)
    for _ in range(a.warmup):
        ops.track_assign(cost, n, n, 0.8)
    res['assign_128x128_ms'] = statistics.median(timed(lambda: ops.track_assign(cost, n, n, 0.8)) for _ in range(a.steps))
    # the NMS launch of the same batch: about 60 anchors per image carry a score above conf, far apart
    pred = torch.zeros(a.streams, 84, 8400)
    pred[:, 4:] = torch.from_numpy(rng.uniform(0, 0.2, (a.streams, 80, 8400)).astype(np.float32))
    for b in range(a.streams):
        idx = rng.choice(8400, 60, replace=False)
        pred[b, 0, idx] = torch.from_numpy(rng.uniform(50, 600, 60).astype(np.float32))
        pred[b, 1, idx] = torch.from_numpy(rng.uniform(50, 600, 60).astype(np.float32))
        pred[b, 2, idx], pred[b, 3, idx] = 20., 20.
        pred[b, 4 + rng.integers(0, 80, 60), idx] = torch.from_numpy(rng.uniform(0.5, 0.9, 60).astype(np.float32))
    pred = pred.to(DEV).contiguous()
    nms = lambda: ops.nms(pred, 0.25, 0.7, None, False, False, 128, 30000, 7680)
    for _ in range(a.warmup):
        kept = nms()
    res['nms_ms'] = statistics.median(timed(nms) for _ in range(a.steps))
    res['nms_kept'] = float(kept[2].float().mean().item())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
