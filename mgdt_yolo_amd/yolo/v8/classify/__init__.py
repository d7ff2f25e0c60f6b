"""reference: yolo/v8/classify/__init__.py: the predictor and the validator of the classification task.  A ClassificationTrainer (captured step,
gradient clipping, SGD, EMA), torchvision backbones and the dataset classes are not built; one training step runs through
`ClassificationModel(batch)` + `loss.backward()`."""
from .predict import ClassificationPredictor, classify_crop, classify_transforms
from .val import ClassificationValidator

__all__ = ('ClassificationPredictor', 'ClassificationValidator', 'classify_transforms', 'classify_crop')
