"""Module registry (reference: nn/modules/__init__.py:27-34 `__all__`): the names `parse_model` resolves from a YAML."""
from .block import (C2f, C3, DFL, IFM, MSPA_C2f, SPP, SPPF, Bottleneck, InjectionMultiSum_Auto_pool, Proto, SimFusion_3in, SimFusion_4in,
                    Upsample, h_sigmoid)
from .conv import Concat, Conv, ConvTranspose2d, DWConv, MaxPool2d, Repeat, ZeroPad2d
from .convnextv2 import ConvNeXtV2_Block
from .head import Classify, Conv_GN, Detect, DyDCNv2, Pose, RTDETRDecoder, Scale, Segment, TaskDecomposition, TOODHead
from .spr_module import SPRModule
from .utils import GRN, LayerNorm

__all__ = ('Conv', 'DWConv', 'Concat', 'DFL', 'SPPF', 'C2f', 'C3', 'MSPA_C2f', 'Bottleneck', 'SPRModule', 'ConvNeXtV2_Block',
           'LayerNorm', 'GRN', 'SimFusion_4in', 'SimFusion_3in', 'IFM', 'h_sigmoid', 'InjectionMultiSum_Auto_pool',
           'Detect', 'Upsample', 'TOODHead', 'DyDCNv2', 'Conv_GN', 'TaskDecomposition', 'Scale', 'Segment', 'Proto', 'Pose', 'Classify', 'RTDETRDecoder',
           'ConvTranspose2d', 'Repeat', 'MaxPool2d', 'ZeroPad2d', 'SPP')
