"""reference: yolo/v8/segment/__init__.py: the predictor and the validator (mask IoU, matching and mask mAP on the device).  Segmentation
training is not built: the reference's v8SegmentationLoss does not run in this fork."""
from .predict import SegmentationPredictor
from .val import SegmentationValidator

__all__ = ('SegmentationPredictor', 'SegmentationValidator')
