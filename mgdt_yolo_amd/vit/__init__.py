"""reference: vit/ - the transformer-based models.  RT-DETR inference is built (vit/rtdetr); SAM is not."""
