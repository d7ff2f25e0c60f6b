"""reference: yolo/v8/segment/__init__.py (inference side: the predictor; segmentation training / validation are not built)."""
from .predict import SegmentationPredictor

__all__ = ('SegmentationPredictor',)
