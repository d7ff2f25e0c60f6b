"""numpy model of the device tracker (mgdt_yolo_amd/csrc/track.hip): ByteTrack as the reference's tracker/trackers/byte_tracker.py:181-295 runs it,
with the 8x8 Kalman filter in its decoupled form (four 2x2 blocks: mean[8] + 12 covariance numbers, fp64), the fp32 cost arithmetic of
tracker/utils/matching.py in its operation order, and an own shortest-augmenting-path solver of the thresholded assignment.  No scipy here: the GPU
tests import this file and scipy may be absent where they run.

Table form, as the kernel keeps it: `cap` slots per stream, state 0 = free, 1 = Tracked, 2 = Lost, 3 = Removed (the reference's TrackState).
A quirk the reference has and this keeps: byte_tracker.py:288 subtracts self.removed_stracks from the lost list BEFORE :290 extends it with this
frame's removals, so a lost track removed after the buffer stays in the lost list for one more frame in state Removed: it is in that frame's duplicate
check and in the next frame's pool, where a match re-activates it.  Its id is in removed_stracks from then on (`rem`), so the next time it is in the lost
list it leaves it at once.  (The reference clips removed_stracks to its last 999 entries; this keeps every id.)
Overflow (more than DET_CAP detections above track_low_thresh, or no free slot for a new track) sets the flag, leaves the state as it was and returns
no rows.
"""
import numpy as np

FREE, TRACKED, LOST, REMOVED = 0, 1, 2, 3
DET_CAP = 128
FLAG_DETS, FLAG_TRACKS = 1, 2
W_POS, W_VEL = 1. / 20, 1. / 160
BIG = 1e300
f32 = np.float32


# ---- the assignment: minimise sum(c_ij - thresh) over a partial matching, pairs with c_ij >= thresh never matched ----------------------
def assign(cost, thresh):
    """cost (n, m) fp32 -> x (n,) int32, -1 = unmatched.  Shortest augmenting paths with fp64 potentials; every row owns a zero-cost dummy column."""
    cost = np.asarray(cost, f32)
    n, m = cost.shape
    x = np.full(n, -1, np.int32)
    if n == 0 or m == 0:
        return x
    red = cost.astype(np.float64) - np.float64(f32(thresh))
    ok = cost < f32(thresh)
    u = np.zeros(n)
    v = np.zeros(m)
    p = np.full(m + 1, -1, np.int64)          # column -> row; column m is the root's
    way = np.zeros(m, np.int64)
    for i in range(n):
        p[m] = i
        j0 = m
        minv = np.full(m, BIG)
        used = np.zeros(m, bool)
        minv_d, way_d = BIG, m
        while True:
            if j0 < m:
                used[j0] = True
            i0 = p[j0]
            if -u[i0] < minv_d:
                minv_d, way_d = -u[i0], j0
            cur = red[i0] - u[i0] - v
            upd = ok[i0] & ~used & (cur < minv)
            minv[upd] = cur[upd]
            way[upd] = j0
            cand = np.where(used, BIG, minv)
            j1 = int(np.argmin(cand))             # first minimum: the lower column on a tie
            best = cand[j1]
            term = not (best < minv_d)
            delta = minv_d if term else best
            rows = np.append(p[:m][used], p[m])
            u[rows] += delta
            v[used] -= delta
            minv[~used] -= delta
            minv_d -= delta
            if term:
                jj = way_d
                break
            j0 = j1
            if p[j0] < 0:
                jj = j0
                break
        while jj != m:
            j1 = way[jj]
            p[jj] = p[j1]
            jj = j1
    for j in range(m):
        if p[j] >= 0:
            x[p[j]] = j
    return x


# ---- fp32 costs (matching.py:199-229 bbox_ious, :89-106 iou_distance, :188-196 fuse_score) ------------------------------------------------
def iou_cost(a, b, scores=None):
    a, b = np.asarray(a, f32).reshape(-1, 4), np.asarray(b, f32).reshape(-1, 4)
    ix = (np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])).clip(0)
    iy = (np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])).clip(0)
    inter = ix * iy
    a1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iou = inter / (a2[None, :] + a1[:, None] - inter + f32(1e-7))
    c = f32(1) - iou
    if scores is not None:
        c = f32(1) - (f32(1) - c) * np.asarray(scores, f32)[None, :]
    return c.astype(f32)


class Stream:
    def __init__(self, cap):
        self.cap = cap
        self.frame_id = 0
        self.count = 0
        self.mean = np.zeros((cap, 8))
        self.cov = np.zeros((cap, 4, 3))          # per coordinate i: P[i,i], P[i,i+4], P[i+4,i+4]
        self.id = np.zeros(cap, np.int32)
        self.state = np.zeros(cap, np.int32)
        self.act = np.zeros(cap, np.int32)
        self.fid = np.zeros(cap, np.int32)
        self.start = np.zeros(cap, np.int32)
        self.tlen = np.zeros(cap, np.int32)
        self.score = np.zeros(cap, f32)
        self.cls = np.zeros(cap, f32)
        self.idx = np.zeros(cap, f32)
        self.rem = np.zeros(cap, np.int32)          # the id is in the reference's removed_stracks

    def copy(self):
        s = Stream(self.cap)
        for k, v in self.__dict__.items():
            setattr(s, k, v.copy() if isinstance(v, np.ndarray) else v)
        return s

    def tlbr(self, t):
        m = self.mean[t]
        w = m[2] * m[3]
        x1, y1 = m[0] - w / 2, m[1] - m[3] / 2
        return np.array([x1, y1, w + x1, m[3] + y1])

    def export(self):
        live = np.nonzero(self.state != FREE)[0]
        live = live[np.argsort(self.id[live])]
        cov = np.zeros((len(live), 8, 8))
        for k, t in enumerate(live):
            for i in range(4):
                cov[k, i, i], cov[k, i, i + 4], cov[k, i + 4, i], cov[k, i + 4, i + 4] = self.cov[t, i, 0], self.cov[t, i, 1], self.cov[t, i, 1], self.cov[t, i, 2]
        return dict(id=self.id[live].copy(), state=self.state[live].copy(), is_activated=self.act[live].copy(), frame_id=self.fid[live].copy(),
                    start_frame=self.start[live].copy(), tracklet_len=self.tlen[live].copy(), score=self.score[live].copy(), cls=self.cls[live].copy(),
                    mean=self.mean[live].copy(), covariance=cov, tracker_frame_id=self.frame_id, count=self.count)


def _q(h, i, pos):
    if i == 2:
        s = 1e-2 if pos else 1e-5
    else:
        s = (W_POS if pos else W_VEL) * h
    return s * s


def _predict(s, t):
    if s.state[t] != TRACKED:
        s.mean[t, 7] = 0
    h = s.mean[t, 3]
    for i in range(4):
        pp, pv, vv = s.cov[t, i]
        s.cov[t, i] = (pp + pv + (pv + vv) + _q(h, i, True), pv + vv, vv + _q(h, i, False))
    s.mean[t, :4] = s.mean[t, :4] + s.mean[t, 4:]


def _measure(row):
    """Detection row -> (tlbr fp32 as STrack keeps it, xyah fp32): _tlwh = float32(tlbr_to_tlwh), tlwh_to_xyah and tlbr in fp32."""
    x1, y1, x2, y2 = (f32(v) for v in row[:4])
    w, h = f32(x2 - x1), f32(y2 - y1)
    return np.array([x1, y1, f32(x1 + w), f32(y1 + h)], f32), np.array([f32(x1 + f32(w / f32(2))), f32(y1 + f32(h / f32(2))), f32(w / h), h], f32)


def _kf_update(s, t, z):
    h = s.mean[t, 3]
    for i in range(4):
        pp, pv, vv = s.cov[t, i]
        r = 1e-1 * 1e-1 if i == 2 else (W_POS * h) * (W_POS * h)
        S = pp + r
        kp, kv = pp / S, pv / S
        inn = float(z[i]) - s.mean[t, i]
        s.mean[t, i] += inn * kp
        s.mean[t, i + 4] += inn * kv
        s.cov[t, i] = (pp - kp * S * kp, pv - kp * S * kv, vv - kv * S * kv)


def _initiate(s, t, z):
    h = float(z[3])
    s.mean[t, :4] = z.astype(np.float64)
    s.mean[t, 4:] = 0
    for i in range(4):
        sp = 1e-2 if i == 2 else 2 * W_POS * h
        sv = 1e-5 if i == 2 else 10 * W_VEL * h
        s.cov[t, i] = (sp * sp, 0.0, sv * sv)


class Tracker:
    def __init__(self, streams=1, cap=128, track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8,
                 frame_rate=30):
        self.s = [Stream(cap) for _ in range(streams)]
        self.high, self.low, self.new, self.match = f32(track_high_thresh), f32(track_low_thresh), f32(new_track_thresh), f32(match_thresh)
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)

    def update(self, b, rows):
        """rows (n, 6) fp32 [x1,y1,x2,y2,conf,cls] -> (tracks (k, 8) fp32 sorted by id, flag).  On a flag the stream is as it was."""
        work = self.s[b].copy()
        out, flag = self._step(work, np.asarray(rows, f32).reshape(-1, 6))
        if flag == 0:
            self.s[b] = work
        return out, flag

    def _step(self, s, rows):
        none = np.zeros((0, 8), f32)
        s.frame_id += 1
        fid = s.frame_id
        conf = rows[:, 4]
        hi = np.nonzero(conf > self.high)[0]
        lo = np.nonzero((conf > self.low) & (conf < self.high))[0]
        if len(hi) + len(lo) > DET_CAP:
            return none, FLAG_DETS
        det = {int(d): _measure(rows[d]) for d in np.concatenate([hi, lo])}
        st0 = s.state.copy()
        pool = np.nonzero(((st0 == TRACKED) & (s.act != 0)) | (st0 == LOST) | (st0 == REMOVED))[0]
        unconf = np.nonzero((st0 == TRACKED) & (s.act == 0))[0]
        for t in pool:
            _predict(s, t)

        def box(ts):
            return np.array([s.tlbr(t) for t in ts], np.float64).reshape(-1, 4).astype(f32)

        def dbox(ds):
            return np.array([det[int(d)][0] for d in ds], f32).reshape(-1, 4)

        def hit(t, d):
            s.tlen[t] = s.tlen[t] + 1 if s.state[t] == TRACKED else 0
            _kf_update(s, t, det[int(d)][1])
            s.state[t], s.act[t], s.fid[t] = TRACKED, 1, fid
            s.score[t], s.cls[t], s.idx[t] = rows[d, 4], rows[d, 5], f32(d)

        # first association: pool x high detections, fused cost
        x = assign(iou_cost(box(pool), dbox(hi), conf[hi]), self.match)
        for r, t in enumerate(pool):
            if x[r] >= 0:
                hit(t, hi[x[r]])
        # second: the unmatched Tracked tracks x low detections, IoU distance, 0.5
        rem = np.array([t for r, t in enumerate(pool) if x[r] < 0 and st0[t] == TRACKED], np.int64)
        x2 = assign(iou_cost(box(rem), dbox(lo)), 0.5)
        for r, t in enumerate(rem):
            if x2[r] >= 0:
                hit(t, lo[x2[r]])
            else:
                s.state[t] = LOST
        # unconfirmed x left-over high detections, fused cost, 0.7
        used = set(int(c) for c in x if c >= 0)
        left = np.array([d for c, d in enumerate(hi) if c not in used], np.int64)
        x3 = assign(iou_cost(box(unconf), dbox(left), conf[left]), 0.7)
        for r, t in enumerate(unconf):
            if x3[r] >= 0:
                hit(t, left[x3[r]])
            else:
                s.state[t] = FREE
        used3 = set(int(c) for c in x3 if c >= 0)
        new = [d for c, d in enumerate(left) if c not in used3 and not conf[d] < self.new]
        free = np.nonzero(s.state == FREE)[0]
        if len(new) > len(free):
            return none, FLAG_TRACKS
        for k, d in enumerate(new):
            t = free[k]
            s.count += 1
            s.id[t] = s.count
            _initiate(s, t, det[int(d)][1])
            s.state[t], s.act[t], s.fid[t], s.start[t], s.tlen[t] = TRACKED, int(fid == 1), fid, fid, 0
            s.score[t], s.cls[t], s.idx[t], s.rem[t] = rows[d, 4], rows[d, 5], f32(d), 0
        # lost for longer than the buffer: Removed, but in the lost list until the end of the next frame; out of it now when the id was removed before
        in_lost = (s.state == LOST) | (s.state == REMOVED)
        marked = in_lost & (st0 != TRACKED) & (fid - s.fid > self.max_time_lost)
        s.state[marked] = REMOVED
        s.state[in_lost & (s.rem != 0)] = FREE
        # duplicates between the tracked and the lost list
        ta, tb = np.nonzero(s.state == TRACKED)[0], np.nonzero((s.state == LOST) | (s.state == REMOVED))[0]
        if len(ta) and len(tb):
            pd = iou_cost(box(ta), box(tb))
            drop = []
            for p_, q_ in zip(*np.nonzero(pd < f32(0.15))):
                a, c = ta[p_], tb[q_]
                drop.append(c if (s.fid[a] - s.start[a]) > (s.fid[c] - s.start[c]) else a)
            s.state[drop] = FREE
        s.rem[marked & (s.state != FREE)] = 1
        live = np.nonzero((s.state == TRACKED) & (s.act != 0))[0]
        live = live[np.argsort(s.id[live])]
        out = np.array([list(s.tlbr(t)) + [s.id[t], s.score[t], s.cls[t], s.idx[t]] for t in live], np.float64).reshape(-1, 8).astype(f32)
        return out, 0
