"""Model graph configs (the reference's `models/v8/*.yaml` `models/v5/yolov5.yaml`, `models/v6/yolov6.yaml` and `models/v3/*.yaml` graphs as Python dict builders)."""
from .v8 import ALL_CONFIGS, CLS_CONFIGS, CONFIGS, POSE_CONFIGS, RTDETR_CONFIGS, SEG_CONFIGS, V3_CONFIGS, V5_CONFIGS, V6_CONFIGS, get_config  # noqa: F401
