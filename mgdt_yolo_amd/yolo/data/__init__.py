"""Device-side pieces of the reference's data path that sit directly in front of the model (reference: yolo/data/augment.py LetterBox, v8_transforms)."""
from .augment import ImagePool, LetterBox, TrainAugment  # noqa: F401
