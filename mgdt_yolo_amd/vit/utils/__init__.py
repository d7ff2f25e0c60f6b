"""reference: vit/utils - the RT-DETR criterion: HungarianMatcher (ops.py) and DETRLoss / RTDETRDetectionLoss (loss.py) on the device."""
from .loss import DETRLoss, RTDETRDetectionLoss, loss_and_head_grads
from .ops import HungarianMatcher

__all__ = ('HungarianMatcher', 'DETRLoss', 'RTDETRDetectionLoss', 'loss_and_head_grads')
