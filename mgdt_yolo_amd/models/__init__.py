"""Model graph configs (the reference's `models/v8/*.yaml` graphs as Python dict builders)."""
from .v8 import CLS_CONFIGS, CONFIGS, POSE_CONFIGS, RTDETR_CONFIGS, SEG_CONFIGS, get_config  # noqa: F401
