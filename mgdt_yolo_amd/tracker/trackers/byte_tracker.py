"""reference: tracker/trackers/byte_tracker.py BYTETracker - here one object tracks `streams` independent video streams, the whole update of a frame
(Kalman predict / update, the three associations, track management) in ONE kernel launch for all of them (ops.bytetrack_update).

Differences from the reference, all on purpose:
  * ids count from 1 per stream.  The reference's counter is one class attribute shared by every tracker of the process and reset by every
    constructor; per stream the ids here equal those of a reference tracker that runs alone.
  * capacity: `capacity` (<= 128) slots per stream for tracked + lost + unconfirmed tracks and 128 detections above track_low_thresh per frame.  A
    frame that does not fit sets the stream's flag, leaves its state as it was and yields no rows; reading results on the host then raises.
  * the reference clips its removed_stracks list to the last 999 entries; the device keeps the removed mark of every live track.
"""
import numpy as np
import torch

from ... import ops as hip


def _get(args, name):
    return args[name] if isinstance(args, dict) else getattr(args, name)


class BYTETracker:
    def __init__(self, args, frame_rate=30, streams=1, device='cuda:0', capacity=hip.TRACK_CAP):
        self.args = args
        self.high, self.low, self.new, self.match = (float(_get(args, k)) for k in ('track_high_thresh', 'track_low_thresh', 'new_track_thresh',
                                                                                    'match_thresh'))
        self.max_time_lost = int(frame_rate / 30.0 * _get(args, 'track_buffer'))
        self.streams, self.capacity, self.device = int(streams), int(capacity), torch.device(device)
        if self.streams < 1:
            raise RuntimeError(f'BYTETracker: streams={streams}')
        if not 1 <= self.capacity <= hip.TRACK_CAP:
            raise RuntimeError(f'BYTETracker: capacity {capacity} is outside 1..{hip.TRACK_CAP}')
        self._state = None          # allocated (zeroed) on the device by the first update
        self._last = None

    # ---- device path -----------------------------------------------------------------------------------------------------------------
    def update_batch(self, rows, counts, active=None, out=None):
        """rows (streams, max_det, 6) fp32 + counts (streams,) int32 on the device, as `ops.nms` returns them; active: optional (streams,) bool mask,
        False = the stream skips this frame -> (tracks (streams, capacity, 8), ntracks, flags) on the device.  No host read."""
        if rows.dim() != 3 or rows.shape[0] != self.streams:
            raise RuntimeError(f'BYTETracker: rows {tuple(rows.shape)} do not hold {self.streams} streams')
        if rows.shape[1] > hip.TRACK_CAP:
            raise RuntimeError(f'BYTETracker: max_det={rows.shape[1]} is above the detection capacity {hip.TRACK_CAP} of a stream and frame')
        hip._need_gpu(rows)
        self._last = hip.bytetrack_update(rows, counts, self.state_buffer, self.capacity, self.high, self.low, self.new, self.match, self.max_time_lost,
                                          active=active, out=out)
        return self._last

    def results(self, last=None):
        """One host read: the list of (n_i, 8) float32 arrays of the last update_batch.  Raises when a stream's frame did not fit."""
        tracks, ntracks, flags = last or self._last
        n, f = torch.stack((ntracks, flags)).tolist()
        if any(f):
            raise RuntimeError(f'BYTETracker: frame over capacity, flags {f} (1: more than {hip.TRACK_CAP} detections above track_low_thresh, '
                               f'2: more than {self.capacity} live tracks); the flagged streams kept their previous state')
        t = tracks.cpu().numpy()
        return [t[i, :n[i]] for i in range(self.streams)]

    # ---- the reference's call: one stream, host results ------------------------------------------------------------------------------------
    def update(self, results, img=None):
        """results: an object with .conf / .xyxy / .cls (numpy or tensor) or an (n, 6) tensor [x1,y1,x2,y2,conf,cls] -> np.float32 (k, 8)
        [x1,y1,x2,y2,track_id,score,cls,idx].  An empty frame is processed (the tracker's frame_id advances), as BYTETracker.update does."""
        if self.streams != 1:
            raise RuntimeError('BYTETracker.update is the single-stream call; use update_batch for a batch of streams')
        if torch.is_tensor(results) or isinstance(results, np.ndarray):
            r = torch.as_tensor(results, dtype=torch.float32).reshape(-1, 6)
        else:
            conf, xyxy, cls = (torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=torch.float32)
                               for v in (results.conf, results.xyxy, results.cls))
            r = torch.cat((xyxy.reshape(-1, 4), conf.reshape(-1, 1), cls.reshape(-1, 1)), 1)
        n = r.shape[0]
        if n > hip.TRACK_CAP:
            raise RuntimeError(f'BYTETracker: {n} detections are above the detection capacity {hip.TRACK_CAP} of a frame')
        rows = torch.zeros(1, max(n, 1), 6, dtype=torch.float32, device=self.device)
        rows[0, :n] = r.to(self.device)
        self.update_batch(rows, torch.tensor([n], dtype=torch.int32).to(self.device))
        return self.results()[0]

    def reset(self, stream=None):
        if self._state is not None:
            hip.bytetrack_reset(self._state, self.streams, self.capacity, -1 if stream is None else int(stream))
        self._last = None

    def state(self, stream=0):
        """The live tracks of a stream in ascending id: dict of id, state, is_activated, frame_id, start_frame, tracklet_len, score, cls, mean (n, 8)
        and covariance (n, 8, 8) float64, tracker_frame_id, count."""
        return hip.bytetrack_export(self.state_buffer, self.streams, self.capacity, stream)

    @property
    def state_buffer(self):
        if self._state is None:
            self._state = hip.bytetrack_state(self.streams, self.capacity, self.device)
        return self._state
