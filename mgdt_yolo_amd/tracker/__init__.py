"""Multi-object tracking (reference: tracker/): ByteTrack with the Kalman filter and the association on the device, for a batch of streams."""
from .track import TRACKER_MAP, TrackingPredictor, get_tracker_cfg, on_predict_postprocess_end, on_predict_start
from .trackers import BYTETracker, TrackState

__all__ = ('BYTETracker', 'TrackState', 'TRACKER_MAP', 'TrackingPredictor', 'get_tracker_cfg', 'on_predict_start', 'on_predict_postprocess_end')
