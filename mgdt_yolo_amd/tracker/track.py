"""reference: tracker/track.py - the tracker registry, the two predictor hooks, and a predictor that runs them on the device for a whole batch."""
import torch

from ..yolo.engine.predictor import DetectionPredictor
from .cfg import BYTETRACK
from .trackers import BYTETracker


def _botsort(*a, **k):
    raise NotImplementedError("tracker 'botsort' is not built: it needs cv2's global motion compensation and a ReID model; use 'bytetrack'")


class _TrackerMap(dict):
    def __missing__(self, key):
        if key == 'botsort':
            _botsort()
        raise KeyError(key)


TRACKER_MAP = _TrackerMap(bytetrack=BYTETracker)


def get_tracker_cfg(name='bytetrack'):
    """The defaults of the reference's tracker/cfg/<name>.yaml."""
    if name == 'botsort':
        _botsort()
    if name != 'bytetrack':
        raise KeyError(f"unknown tracker '{name}'")
    return dict(BYTETRACK)


def on_predict_start(predictor, persist=False):
    """track.py:15-36: one tracker for the predictor's batch of streams (the reference builds a list of bs single-stream trackers)."""
    if hasattr(predictor, 'trackers') and persist:
        return
    cfg = dict(get_tracker_cfg('bytetrack'), **(getattr(predictor.args, 'tracker_cfg', None) or {}))
    if cfg['tracker_type'] not in ('bytetrack', 'botsort'):
        raise AssertionError(f"Only support 'bytetrack' and 'botsort' for now, but got '{cfg['tracker_type']}'")
    predictor.trackers = TRACKER_MAP[cfg['tracker_type']](args=cfg, frame_rate=30, streams=predictor.args.streams, device=predictor.device)


def on_predict_postprocess_end(predictor):
    """track.py:39-52 for the batch: the NMS rows (already in original-image coordinates) + counts of predictor.nms_out go through update_batch with
    active = counts > 0 (the reference skips the update of a frame without detections, so that stream's frame_id does not advance), then ONE host
    read.  predictor.results[i] = (n, 7) [x1,y1,x2,y2,track_id,conf,cls], the reference's tracks[:, :-1]; predictor.track_idx[i] = the row of
    the detection each track took (tracks[:, -1])."""
    rows, counts = predictor.nms_out
    trk = predictor.trackers
    trk.update_batch(rows, counts, active=counts > 0)
    res = trk.results()
    predictor.results = [torch.from_numpy(r[:, :7].copy()) for r in res]
    predictor.track_idx = [r[:, 7].astype(int) for r in res]


class TrackingPredictor(DetectionPredictor):
    """DetectionPredictor + the two hooks: batched NMS (rows + counts stay on the device), boxes scaled to the original images on the device,
    update_batch, one host read.  Image i of every call is frame t of stream i; `streams` fixes the batch size.  max_det defaults to the tracker's
    detection capacity."""

    def __init__(self, overrides=None, persist=True):
        o = dict(max_det=128, streams=1, tracker='bytetrack', tracker_cfg=None)
        o.update(overrides or {})
        super().__init__(o)
        self.persist = persist
        self.args.mode = 'track'
        if self.args.tracker == 'botsort':
            _botsort()

    def postprocess(self, preds, img, orig_imgs):
        from .. import ops as hip
        from ..yolo.utils import ops
        pred = preds[0] if isinstance(preds, (list, tuple)) else preds
        if pred.shape[0] != self.args.streams:
            raise RuntimeError(f'TrackingPredictor: a batch of {pred.shape[0]} images for {self.args.streams} streams')
        if self.args.classes is not None and len(self.args.classes) == 0:
            raise RuntimeError('TrackingPredictor: an empty class filter leaves nothing to track')
        on_predict_start(self, persist=self.persist)
        pred = pred if (pred.dtype == torch.float32 and pred.is_contiguous()) else pred.float().contiguous()
        rows, _, counts = hip.nms(pred, self.args.conf, self.args.iou, self.args.classes, self.args.agnostic_nms, False, self.args.max_det, 30000, 7680)
        if not isinstance(orig_imgs, torch.Tensor):
            for i in range(rows.shape[0]):      # rows past counts[i] hold nothing the tracker reads
                ops.scale_boxes(img.shape[2:], rows[i], tuple(orig_imgs[i].shape))
        self.nms_out = (rows, counts)
        on_predict_postprocess_end(self)
        return self.results
