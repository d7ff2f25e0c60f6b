"""Tracker settings (reference: tracker/cfg/*.yaml) as Python dicts, like the model graphs of mgdt_yolo_amd.models."""

BYTETRACK = dict(tracker_type='bytetrack', track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, track_buffer=30, match_thresh=0.8)
