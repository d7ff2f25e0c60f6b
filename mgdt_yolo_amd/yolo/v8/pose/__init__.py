"""reference: yolo/v8/pose/__init__.py: the predictor and the validator (OKS matching on the device, box and pose mAP).  Pose training is not built
(the reference's v8PoseLoss does not run in this fork)."""
from .predict import PosePredictor
from .val import PoseValidator

__all__ = ('PosePredictor', 'PoseValidator')
