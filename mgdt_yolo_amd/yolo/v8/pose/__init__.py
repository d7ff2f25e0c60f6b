"""reference: yolo/v8/pose/__init__.py: the predictor.  Pose training and OKS validation are not built (the reference's v8PoseLoss does not run in
this fork)."""
from .predict import PosePredictor

__all__ = ('PosePredictor',)
