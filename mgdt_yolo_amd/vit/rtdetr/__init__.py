"""reference: vit/rtdetr - RT-DETR.  The predictor and the validator are built; the model wrapper and the trainer are not."""
from .predict import RTDETRPredictor
from .val import RTDETRValidator

__all__ = ('RTDETRPredictor', 'RTDETRValidator')
