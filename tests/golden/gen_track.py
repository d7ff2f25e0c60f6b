"""Generate tests/golden/track_NN.npz and track_solver.npz from the reference's own BYTETracker (build container only).

The reference's tracker/utils/matching.py imports `lap` and, when it is missing, calls check_requirements('lap'), which would try to install a
package: a stand-in module `lap` is therefore installed BEFORE anything of ultralytics.tracker is imported.  lapjv(cost, extend_cost=True,
cost_limit=t) is scipy's linear_sum_assignment on lap's own extended matrix: (n+m)^2, filled with t/2, the lower-right block 0, the top-left block
the cost; x[i] = j for real-real pairs, otherwise -1.

Run:  python tests/golden/gen_track.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

STREAMS, FRAMES, MAX_OBJ, MAX_DET, SIZE = 4, 60, 12, 16, 640
MARGIN, NOISE, RERUNS = 1e-3, 1e-4, 5
EVENTS = ('reactivated', 'removed_then_new_id', 'second_match', 'high_below_new_thresh', 'unconfirmed_removed', 'duplicate_removed', 'empty_frame')


def extended(cost, t):
    n, m = cost.shape
    e = np.full((n + m, n + m), t / 2.0, np.float64)
    e[n:, m:] = 0
    e[:n, :m] = cost
    return e


def lapjv(cost, extend_cost=True, cost_limit=np.inf):
    from scipy.optimize import linear_sum_assignment
    assert extend_cost and np.isfinite(cost_limit)
    cost = np.asarray(cost, np.float64)
    n, m = cost.shape
    e = extended(cost, cost_limit)
    r, c = linear_sum_assignment(e)
    x, y = np.full(n, -1, np.int64), np.full(m, -1, np.int64)
    for i, j in zip(r, c):
        if i < n and j < m:
            x[i], y[j] = j, i
    return float(e[r, c].sum()), x, y


def install():
    ref_import.install()
    lap = types.ModuleType('lap')
    lap.__version__ = '0.4.0'
    lap.lapjv = lapjv
    sys.modules['lap'] = lap
    for name, sub in (('ultralytics.tracker', 'tracker'), ('ultralytics.tracker.trackers', 'tracker/trackers')):      # shell packages: no bot_sort / cv2 GMC import
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref_import.REF, sub)]
        sys.modules[name] = m
    import importlib
    bt = importlib.import_module('ultralytics.tracker.trackers.byte_tracker')
    return bt, importlib.import_module('ultralytics.tracker.utils.matching')


# ---- synthetic scenes ---------------------------------------------------------------------------------------------------------------
def make_stream(rng, long_gaps, empty_at=None):
    """-> rows (FRAMES, MAX_DET, 6) fp32 sorted by descending score, counts (FRAMES,)."""
    objs = []
    for k in range(int(rng.integers(5, 9))):
        w, h = rng.uniform(40, 110, 2)
        start = 0 if k < 4 else int(rng.integers(1, 30))
        o = dict(c=rng.uniform(80, SIZE - 80, 2), v=rng.uniform(-3.5, 3.5, 2), w=w, h=h, start=start, end=int(rng.integers(start + 25, FRAMES + 1)),
                 cls=float(rng.integers(0, 2)), score=rng.uniform(0.72, 0.93), gone=set(), low=set())
        for _ in range(int(rng.integers(0, 3))):
            g0 = int(rng.integers(o['start'] + 4, FRAMES - 4))
            o['gone'] |= set(range(g0, g0 + int(rng.integers(7, 12) if long_gaps and rng.random() < 0.5 else rng.integers(2, 5))))
        for _ in range(int(rng.integers(0, 3))):
            l0 = int(rng.integers(o['start'] + 3, FRAMES - 3))
            o['low'] |= set(range(l0, l0 + int(rng.integers(1, 4))))
        objs.append(o)
    # a crossing: B walks over the standing A and is hidden while near it, so B's lost track drifts over A's box (a duplicate)
    ca = rng.uniform(200, 440, 2)
    t0 = int(rng.integers(5, 15))
    objs.append(dict(c=ca, v=np.zeros(2), w=90., h=90., start=0, end=FRAMES, cls=0., score=0.9, gone=set(), low=set()))
    objs.append(dict(c=ca - np.array([4. * (t0 + 16), 0.]), v=np.array([4., 0.]), w=90., h=90., start=0, end=FRAMES, cls=1., score=0.85,
                     gone=set(range(t0, t0 + 34)), low=set()))
    objs = objs[-MAX_OBJ:]
    rows = np.zeros((FRAMES, MAX_DET, 6), np.float32)
    counts = np.zeros(FRAMES, np.int32)
    for f in range(FRAMES):
        det = []
        if f != empty_at:
            for o in objs:
                if not (o['start'] <= f < o['end']) or f in o['gone']:
                    continue
                c = o['c'] + o['v'] * f + rng.uniform(-1, 1, 2)
                w, h = o['w'] + rng.uniform(-1, 1), o['h'] + rng.uniform(-1, 1)
                s = rng.uniform(0.15, 0.45) if f in o['low'] else min(0.97, o['score'] + rng.uniform(-0.05, 0.05))
                det.append([c[0] - w / 2, c[1] - h / 2, c[0] + w / 2, c[1] + h / 2, s, o['cls']])
            if f > 0 and rng.random() < 0.15:      # a one-frame detection: below new_track_thresh (starts nothing) or above (an unconfirmed track, removed)
                c, w, h = rng.uniform(60, SIZE - 60, 2), rng.uniform(30, 70), rng.uniform(30, 70)
                s = rng.uniform(0.52, 0.58) if rng.random() < 0.5 else rng.uniform(0.65, 0.9)
                det.append([c[0] - w / 2, c[1] - h / 2, c[0] + w / 2, c[1] + h / 2, s, float(rng.integers(0, 2))])
        det = np.array(sorted(det, key=lambda r: -r[4]), np.float32).reshape(-1, 6)[:MAX_DET]
        rows[f, :len(det)] = det
        counts[f] = len(det)
    return rows, counts


# ---- one run of the reference, instrumented ---------------------------------------------------------------------------------------------
class Run:
    def __init__(self, bt, matching, cfg, rows, counts, noise_seed=None):
        self.events = set()
        self.min_margin = np.inf
        calls = []
        orig_la, orig_dup = matching.linear_assignment, bt.BYTETracker.remove_duplicate_stracks
        nrng = np.random.default_rng(noise_seed) if noise_seed is not None else None

        def la(cost, thresh, use_lap=True):
            cost = np.asarray(cost)
            if cost.size:
                self.min_margin = min(self.min_margin, float(np.abs(cost.astype(np.float64) - thresh).min()))
                if nrng is not None:
                    cost = cost + nrng.uniform(-NOISE, NOISE, cost.shape)
            out = orig_la(cost, thresh, use_lap)
            calls.append((cost.shape, len(out[0]), len(out[1]), len(out[2])))
            return out

        def dup(a, b):
            pd = matching.iou_distance(a, b)
            if pd.size:
                self.min_margin = min(self.min_margin, float(np.abs(pd.astype(np.float64) - 0.15).min()))
            ra, rb = orig_dup(a, b)
            if len(ra) < len(a) or len(rb) < len(b):
                self.events.add('duplicate_removed')
            return ra, rb

        matching.linear_assignment = la
        bt.BYTETracker.remove_duplicate_stracks = staticmethod(dup)
        try:
            args = types.SimpleNamespace(**cfg)
            self.out, self.snaps = [], []
            for b in range(rows.shape[0]):
                trk = bt.BYTETracker(args, frame_rate=30)          # resets the process-global id counter: each stream runs alone
                outs, snaps = [], []
                for f in range(rows.shape[1]):
                    r = rows[b, f, :counts[b, f]]
                    if len(r) == 0:
                        self.events.add('empty_frame')
                    for thr in (cfg['track_high_thresh'], cfg['track_low_thresh'], cfg['new_track_thresh']):
                        if len(r):
                            self.min_margin = min(self.min_margin, float(np.abs(r[:, 4].astype(np.float64) - thr).min()))
                    lost_before = {t.track_id for t in trk.lost_stracks}
                    count_before, removed_before = bt.BaseTrack._count, len(trk.removed_stracks)
                    del calls[:]
                    o = trk.update(types.SimpleNamespace(conf=r[:, 4].copy(), xyxy=r[:, :4].copy(), cls=r[:, 5].copy()))
                    o = np.asarray(o, np.float32).reshape(-1, 8)
                    outs.append(o[np.argsort(o[:, 4], kind='stable')])
                    if lost_before & {t.track_id for t in trk.tracked_stracks}:
                        self.events.add('reactivated')
                    if calls[1][1] > 0:
                        self.events.add('second_match')
                    if calls[2][2] > 0:
                        self.events.add('unconfirmed_removed')
                    if calls[2][3] > bt.BaseTrack._count - count_before:
                        self.events.add('high_below_new_thresh')
                    if any(t.is_activated and t.frame_id < trk.frame_id - trk.max_time_lost for t in trk.removed_stracks[removed_before:]):
                        self.buffer_removed = True
                    if getattr(self, 'buffer_removed', False) and bt.BaseTrack._count > count_before:
                        self.events.add('removed_then_new_id')
                    if (f + 1) % 10 == 0:
                        ts = sorted(trk.tracked_stracks + trk.lost_stracks, key=lambda t: t.track_id)
                        snaps.append(dict(id=[t.track_id for t in ts], state=[t.state for t in ts], is_activated=[int(t.is_activated) for t in ts],
                                          frame_id=[t.frame_id for t in ts], start_frame=[t.start_frame for t in ts],
                                          tracklet_len=[t.tracklet_len for t in ts], score=[t.score for t in ts], cls=[t.cls for t in ts],
                                          mean=[np.asarray(t.mean, np.float64) for t in ts], covariance=[np.asarray(t.covariance, np.float64) for t in ts],
                                          tracker_frame_id=trk.frame_id, count=bt.BaseTrack._count))
                self.buffer_removed = False
                self.out.append(outs)
                self.snaps.append(snaps)
        finally:
            matching.linear_assignment = orig_la
            bt.BYTETracker.remove_duplicate_stracks = staticmethod(orig_dup)

    def decisions(self):
        return [[o[:, [4, 6, 7]].tolist() for o in outs] for outs in self.out]


def pack(cfg, rows, counts, run, seed):
    kmax = max(len(o) for outs in run.out for o in outs)
    out = np.zeros((STREAMS, FRAMES, kmax, 8), np.float32)
    nout = np.zeros((STREAMS, FRAMES), np.int32)
    for b, outs in enumerate(run.out):
        for f, o in enumerate(outs):
            out[b, f, :len(o)] = o
            nout[b, f] = len(o)
    nsnap = FRAMES // 10
    smax = max(len(s['id']) for ss in run.snaps for s in ss)
    d = dict(rows=rows, counts=counts, out=out, nout=nout, seed=np.int64(seed), snap_frames=np.arange(1, nsnap + 1) * 10,
             snap_n=np.zeros((STREAMS, nsnap), np.int32), snap_tracker_frame_id=np.zeros((STREAMS, nsnap), np.int32),
             snap_count=np.zeros((STREAMS, nsnap), np.int32), snap_mean=np.zeros((STREAMS, nsnap, smax, 8)),
             snap_covariance=np.zeros((STREAMS, nsnap, smax, 8, 8)), snap_score=np.zeros((STREAMS, nsnap, smax), np.float32),
             snap_cls=np.zeros((STREAMS, nsnap, smax), np.float32))
    for k in ('id', 'state', 'is_activated', 'frame_id', 'start_frame', 'tracklet_len'):
        d['snap_' + k] = np.zeros((STREAMS, nsnap, smax), np.int32)
    for b, ss in enumerate(run.snaps):
        for i, s in enumerate(ss):
            n = len(s['id'])
            d['snap_n'][b, i], d['snap_tracker_frame_id'][b, i], d['snap_count'][b, i] = n, s['tracker_frame_id'], s['count']
            for k in ('id', 'state', 'is_activated', 'frame_id', 'start_frame', 'tracklet_len', 'score', 'cls', 'mean', 'covariance'):
                if n:
                    d['snap_' + k][b, i, :n] = np.asarray(s[k])
    for k, v in cfg.items():
        d['cfg_' + k] = np.float64(v)
    return d


def sequences(bt, matching):
    base = dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8)
    seen = set()
    for nn, (buffer, seed0) in enumerate(((30, 0), (5, 100))):
        cfg = dict(base, track_buffer=buffer)
        for seed in range(seed0, seed0 + 50):
            rng = np.random.default_rng(seed)
            made = [make_stream(rng, long_gaps=buffer == 5, empty_at=31 if b == 1 else None) for b in range(STREAMS)]
            rows, counts = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
            run = Run(bt, matching, cfg, rows, counts)
            if run.min_margin < MARGIN:
                print(f'track_{nn:02d}: seed {seed} margin {run.min_margin:.2e} - next seed')
                continue
            want = run.decisions()
            if any(Run(bt, matching, cfg, rows, counts, noise_seed=1000 + k).decisions() != want for k in range(RERUNS)):
                print(f'track_{nn:02d}: seed {seed} decisions move under noise - next seed')
                continue
            break
        else:
            raise SystemExit('no seed passed the margins')
        # the blocks decouple: every covariance entry outside (i,i), (i,i+4), (i+4,i), (i+4,i+4) is exactly 0 in the reference
        mask = np.ones((8, 8), bool)
        for i in range(4):
            mask[i, i] = mask[i, i + 4] = mask[i + 4, i] = mask[i + 4, i + 4] = False
        assert all(not np.asarray(s['covariance'])[:, mask].any() for ss in run.snaps for s in ss if len(s['id']))
        d = pack(cfg, rows, counts, run, seed)
        path = os.path.join(HERE, f'track_{nn:02d}.npz')
        np.savez_compressed(path, **d)
        seen |= run.events
        print(f'{path}: seed {seed}, margin {run.min_margin:.2e}, max id {int(d["snap_count"].max())}, events {sorted(run.events)}, '
              f'{os.path.getsize(path)} bytes')
        assert os.path.getsize(path) < 1 << 20
    missing = set(EVENTS) - seen
    assert not missing, f'events that never occurred: {missing}'


def solver_cases():
    thresh = 0.8
    d = {}
    names = []

    def stable(cost):
        tot, x, _ = lapjv(cost, True, thresh) if cost.size else (0.0, np.full(cost.shape[0], -1, np.int64), None)
        if not cost.size:
            tot = (cost.shape[0] + cost.shape[1]) * thresh / 2
        rng = np.random.default_rng(7)
        for _ in range(RERUNS):
            if cost.size and not np.array_equal(lapjv(cost + rng.uniform(-NOISE, NOISE, cost.shape), True, thresh)[1], x):
                return None
        return tot, x

    def add(name, make):
        for seed in range(1000):
            cost = make(np.random.default_rng(seed)).astype(np.float32)
            r = stable(cost)
            if r is not None:
                d[name + '_cost'], d[name + '_x'], d[name + '_total'] = cost, r[1].astype(np.int32), np.float64(r[0])
                names.append(name)
                print(f'solver {name}: seed {seed}, {int((r[1] >= 0).sum())} matched, total {r[0]:.6f}')
                return
        raise SystemExit(f'solver case {name}: no stable seed')

    for n, m in ((0, 5), (5, 0), (1, 1), (7, 13), (13, 7), (64, 64), (65, 63), (128, 128), (128, 1)):
        add(f'u{n}x{m}', lambda rng, n=n, m=m: rng.uniform(0, 1, (n, m)))
    add('above', lambda rng: rng.uniform(0.85, 1, (9, 11)))

    def sparse(rng):      # IoU-like: most entries are exactly 1.0, a few candidates per row
        c = np.ones((40, 48))
        for i in range(40):
            for j in rng.choice(48, int(rng.integers(0, 4)), replace=False):
                c[i, j] = rng.uniform(0.05, 0.95)
        return c
    add('sparse', sparse)
    d['names'] = np.array(names)
    d['thresh'] = np.float64(thresh)
    path = os.path.join(HERE, 'track_solver.npz')
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


def yaml_fixture():
    import json
    import yaml
    with open(os.path.join(ref_import.REF, 'tracker', 'cfg', 'bytetrack.yaml')) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(HERE, 'bytetrack_yaml.json'), 'w') as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    bt_, matching_ = install()
    yaml_fixture()
    solver_cases()
    sequences(bt_, matching_)
