"""reference: vit/rtdetr - RT-DETR.  The predictor is built; the model wrapper, the trainer and the validator are not."""
from .predict import RTDETRPredictor

__all__ = ('RTDETRPredictor',)
