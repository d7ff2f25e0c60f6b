"""YOLOv8-family model graphs of the MGDT-YOLO fork as cfg dicts.

Same on-disk schema the reference parses (`[from, repeats, module, args]` rows, `scales`, `nc`;
reference: models/v8/{yolov8,mspa_c2f_yolov8,gd_yolov8,mspa_c2f_gd_yolov8}.yaml, consumed by
nn/tasks.py:604-699).  A user YAML in that schema is loaded by `nn.tasks.yaml_model_load`; these
builders exist so the GPU box (which has no copy of the reference) can build the named configs.
"""
from copy import deepcopy

# [depth, width, max_channels]
SCALES = {'n': [0.33, 0.25, 1024], 's': [0.33, 0.50, 1024], 'm': [0.67, 0.75, 768],
          'l': [1.00, 1.00, 512], 'x': [1.00, 1.25, 512]}


def _backbone(block):
    rows = [[-1, 1, 'Conv', [64, 3, 2]], [-1, 1, 'Conv', [128, 3, 2]]]
    for reps, ch in ((3, 128), (6, 256), (6, 512), (3, 1024)):
        rows.append([-1, reps, block, [ch, True]])
        if ch != 1024:
            rows.append([-1, 1, 'Conv', [ch * 2, 3, 2]])
    rows.append([-1, 1, 'SPPF', [1024, 5]])
    return rows


def _pan_head():
    up = [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']]
    return [list(up), [[-1, 6], 1, 'Concat', [1]], [-1, 3, 'C2f', [512]],
            list(up), [[-1, 4], 1, 'Concat', [1]], [-1, 3, 'C2f', [256]],
            [-1, 1, 'Conv', [256, 3, 2]], [[-1, 12], 1, 'Concat', [1]], [-1, 3, 'C2f', [512]],
            [-1, 1, 'Conv', [512, 3, 2]], [[-1, 9], 1, 'Concat', [1]], [-1, 3, 'C2f', [1024]],
            [[15, 18, 21], 1, 'Detect', ['nc']]]


def _gd_head():
    return [[[2, 4, 6, 9], 1, 'SimFusion_4in', []], [-1, 1, 'IFM', [[64, 32]]],
            [6, 1, 'Conv', [256, 1, 1]], [[2, 4, -1], 1, 'SimFusion_3in', [256]],
            [[-1, 11], 1, 'InjectionMultiSum_Auto_pool', [256, [64, 32], 1]], [-1, 3, 'C2f', [256]],
            [[15], 1, 'Detect', ['nc']]]


def _gd_tood_head():
    """models/v8/mspa_c2f_gd_tood_yolov8.yaml: the GD neck with the task-aligned head, `hidc` = 64 unscaled (works at scale n only)."""
    return _gd_head()[:-1] + [[[15], 1, 'TOODHead', ['nc', 64]]]


def _gd_tood_head_s():
    """Our own variant for scale s (SURVEY section 8 row a15 / BASELINE configs[3]): the reference YAML's hidc=64 only fits scale n because
    parse_model leaves it unscaled (tasks.py:664-665 commented out); here hidc = 128 = the s-scale width of the head input."""
    return _gd_head()[:-1] + [[[15], 1, 'TOODHead', ['nc', 128]]]


def _cfg(block, head, nc):
    return {'nc': nc, 'scales': deepcopy(SCALES), 'backbone': _backbone(block), 'head': head()}


CONFIGS = {
    'yolov8': lambda nc=80: _cfg('C2f', _pan_head, nc),
    'mspa_c2f_yolov8': lambda nc=80: _cfg('MSPA_C2f', _pan_head, nc),
    'gd_yolov8': lambda nc=80: _cfg('C2f', _gd_head, nc),
    'mspa_c2f_gd_yolov8': lambda nc=80: _cfg('MSPA_C2f', _gd_head, nc),
    'mspa_c2f_gd_tood_yolov8_hidc128': lambda nc=80: _cfg('MSPA_C2f', _gd_tood_head_s, nc),      # use with scale='s'
    'mspa_c2f_gd_tood_yolov8': lambda nc=2: _cfg('MSPA_C2f', _gd_tood_head, nc),
}


def _seg(head):
    """`head` with its Detect row replaced by Segment [nc, 32, 256] (models/v8/yolov8-seg.yaml:46)."""
    def build():
        rows = head()
        rows[-1] = [rows[-1][0], 1, 'Segment', ['nc', 32, 256]]
        return rows
    return build


# instance-segmentation graphs: `yolov8-seg` is the reference's models/v8/yolov8-seg.yaml; `mspa_c2f_gd_yolov8-seg` is this fork's MSPA-GD graph
# with the same head swap (the reference ships no file for it).  Kept apart from CONFIGS, which lists the detection graphs only.
SEG_CONFIGS = {
    'yolov8-seg': lambda nc=80: _cfg('C2f', _seg(_pan_head), nc),
    'mspa_c2f_gd_yolov8-seg': lambda nc=80: _cfg('MSPA_C2f', _seg(_gd_head), nc),
}


def _pose(head):
    """`head` with its Detect row replaced by Pose [nc, kpt_shape] (models/v8/yolov8-pose.yaml:46)."""
    def build():
        rows = head()
        rows[-1] = [rows[-1][0], 1, 'Pose', ['nc', 'kpt_shape']]
        return rows
    return build


def _pose_cfg(block, head, nc, kpt_shape):
    d = _cfg(block, _pose(head), nc)
    d['kpt_shape'] = list(kpt_shape)
    return d


# pose-estimation graphs: `yolov8-pose` is the reference's models/v8/yolov8-pose.yaml (nc 1, 17 keypoints of (x, y, visibility)); `mspa_c2f_gd_yolov8-pose`
# is this fork's MSPA-GD graph with the same head swap (a one-level head; the reference ships no file for it).
POSE_CONFIGS = {
    'yolov8-pose': lambda nc=1, kpt_shape=(17, 3): _pose_cfg('C2f', _pan_head, nc, kpt_shape),
    'mspa_c2f_gd_yolov8-pose': lambda nc=1, kpt_shape=(17, 3): _pose_cfg('MSPA_C2f', _gd_head, nc, kpt_shape),
}


# [depth, width, max_channels] of models/v8/yolov8-cls.yaml: every scale keeps max_channels 1024 (the detection YAMLs cut m / l / x)
CLS_SCALES = {'n': [0.33, 0.25, 1024], 's': [0.33, 0.50, 1024], 'm': [0.67, 0.75, 1024], 'l': [1.00, 1.00, 1024], 'x': [1.00, 1.25, 1024]}


def _cls_cfg(nc):
    """models/v8/yolov8-cls.yaml: the yolov8 backbone without SPPF, then Classify [nc]."""
    return {'nc': nc, 'scales': deepcopy(CLS_SCALES), 'backbone': _backbone('C2f')[:-1], 'head': [[-1, 1, 'Classify', ['nc']]]}


# image-classification graph: the reference's models/v8/yolov8-cls.yaml (nc 1000)
CLS_CONFIGS = {'yolov8-cls': lambda nc=1000: _cls_cfg(nc)}


def _rtdetr(head):
    """`head` with its Detect row replaced by RTDETRDecoder [nc] (models/v8/yolov8-rtdetr.yaml:46)."""
    def build():
        rows = head()
        rows[-1] = [rows[-1][0], 1, 'RTDETRDecoder', ['nc']]
        return rows
    return build


# RT-DETR graph: the reference's models/v8/yolov8-rtdetr.yaml (the yolov8 backbone and PAN neck, then RTDETRDecoder).  Kept apart from CONFIGS: its
# output is not Detect's (B, 4 + nc, A) map.  The reference's rtdetr-l / rtdetr-x graphs (HGStem, HGBlock, AIFI, RepC3) are not built.
RTDETR_CONFIGS = {'yolov8-rtdetr': lambda nc=80: _cfg('C2f', _rtdetr(_pan_head), nc)}


# [depth, width, max_channels] of models/v5/yolov5.yaml: m / l / x keep max_channels 1024 and x is deeper (1.33) than in the v8 files
V5_SCALES = {'n': [0.33, 0.25, 1024], 's': [0.33, 0.50, 1024], 'm': [0.67, 0.75, 1024], 'l': [1.00, 1.00, 1024], 'x': [1.33, 1.25, 1024]}


def _v5_cfg(nc):
    """models/v5/yolov5.yaml (YOLOv5 v6.0, P3-P5): the 6x6 / stride 2 / padding 2 stem, C3 blocks, SPPF, a PAN head of C3 blocks without shortcuts, Detect."""
    up = [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']]
    backbone = [[-1, 1, 'Conv', [64, 6, 2, 2]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 3, 'C3', [128]], [-1, 1, 'Conv', [256, 3, 2]], [-1, 6, 'C3', [256]],
                [-1, 1, 'Conv', [512, 3, 2]], [-1, 9, 'C3', [512]], [-1, 1, 'Conv', [1024, 3, 2]], [-1, 3, 'C3', [1024]], [-1, 1, 'SPPF', [1024, 5]]]
    head = [[-1, 1, 'Conv', [512, 1, 1]], list(up), [[-1, 6], 1, 'Concat', [1]], [-1, 3, 'C3', [512, False]],
            [-1, 1, 'Conv', [256, 1, 1]], list(up), [[-1, 4], 1, 'Concat', [1]], [-1, 3, 'C3', [256, False]],
            [-1, 1, 'Conv', [256, 3, 2]], [[-1, 14], 1, 'Concat', [1]], [-1, 3, 'C3', [512, False]],
            [-1, 1, 'Conv', [512, 3, 2]], [[-1, 10], 1, 'Concat', [1]], [-1, 3, 'C3', [1024, False]],
            [[17, 20, 23], 1, 'Detect', ['nc']]]
    return {'nc': nc, 'scales': deepcopy(V5_SCALES), 'backbone': backbone, 'head': head}


# YOLOv5 detection graph: the reference's models/v5/yolov5.yaml.  A table of its own: CONFIGS lists the graphs that have a models/v8/ file.
# yolov5-p6 is not built.
V5_CONFIGS = {'yolov5': lambda nc=80: _v5_cfg(nc)}


# [depth, width, max_channels] of models/v6/yolov6.yaml (the v8 table)
V6_SCALES = {'n': [0.33, 0.25, 1024], 's': [0.33, 0.50, 1024], 'm': [0.67, 0.75, 768], 'l': [1.00, 1.00, 512], 'x': [1.00, 1.25, 512]}


def _v6_cfg(nc):
    """models/v6/yolov6.yaml (YOLOv6-3.0, P3-P5), row for row: 3x3 Conv + BN + ReLU throughout (`activation: nn.ReLU()`), repeated plain Conv rows,
    SPPF, nn.ConvTranspose2d(c, c, 2, 2, 0) up-sampling in the head, Detect."""
    backbone = [[-1, 1, 'Conv', [64, 3, 2]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 6, 'Conv', [128, 3, 1]], [-1, 1, 'Conv', [256, 3, 2]],
                [-1, 12, 'Conv', [256, 3, 1]], [-1, 1, 'Conv', [512, 3, 2]], [-1, 18, 'Conv', [512, 3, 1]], [-1, 1, 'Conv', [1024, 3, 2]],
                [-1, 6, 'Conv', [1024, 3, 1]], [-1, 1, 'SPPF', [1024, 5]]]
    head = [[-1, 1, 'Conv', [256, 1, 1]], [-1, 1, 'nn.ConvTranspose2d', [256, 2, 2, 0]], [[-1, 6], 1, 'Concat', [1]], [-1, 1, 'Conv', [256, 3, 1]],
            [-1, 9, 'Conv', [256, 3, 1]],
            [-1, 1, 'Conv', [128, 1, 1]], [-1, 1, 'nn.ConvTranspose2d', [128, 2, 2, 0]], [[-1, 4], 1, 'Concat', [1]], [-1, 1, 'Conv', [128, 3, 1]],
            [-1, 9, 'Conv', [128, 3, 1]],
            [-1, 1, 'Conv', [128, 3, 2]], [[-1, 15], 1, 'Concat', [1]], [-1, 1, 'Conv', [256, 3, 1]], [-1, 9, 'Conv', [256, 3, 1]],
            [-1, 1, 'Conv', [256, 3, 2]], [[-1, 10], 1, 'Concat', [1]], [-1, 1, 'Conv', [512, 3, 1]], [-1, 9, 'Conv', [512, 3, 1]],
            [[19, 23, 27], 1, 'Detect', ['nc']]]
    return {'nc': nc, 'activation': 'nn.ReLU()', 'scales': deepcopy(V6_SCALES), 'backbone': backbone, 'head': head}


# YOLOv6 detection graph: the reference's models/v6/yolov6.yaml.  `activation` holds only for the build (nn.tasks.parse_model restores Conv.default_act).
V6_CONFIGS = {'yolov6': lambda nc=80: _v6_cfg(nc)}


def _v3_darknet53():
    """rows 0-10 of models/v3/yolov3.yaml and yolov3-spp.yaml: the darknet53 backbone (a stride-1 stem, Bottleneck rows with repeats)"""
    return [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'Conv', [64, 3, 2]], [-1, 1, 'Bottleneck', [64]], [-1, 1, 'Conv', [128, 3, 2]], [-1, 2, 'Bottleneck', [128]],
            [-1, 1, 'Conv', [256, 3, 2]], [-1, 8, 'Bottleneck', [256]], [-1, 1, 'Conv', [512, 3, 2]], [-1, 8, 'Bottleneck', [512]],
            [-1, 1, 'Conv', [1024, 3, 2]], [-1, 4, 'Bottleneck', [1024]]]


def _v3_head(row12):
    """the head both full-width files share; they differ in row 12 only (a 1x1 Conv in yolov3, SPP in yolov3-spp).  Rows 16 and 23 read `from = -2`."""
    up = [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']]
    return [[-1, 1, 'Bottleneck', [1024, False]], row12, [-1, 1, 'Conv', [1024, 3, 1]], [-1, 1, 'Conv', [512, 1, 1]], [-1, 1, 'Conv', [1024, 3, 1]],
            [-2, 1, 'Conv', [256, 1, 1]], list(up), [[-1, 8], 1, 'Concat', [1]], [-1, 1, 'Bottleneck', [512, False]], [-1, 1, 'Bottleneck', [512, False]],
            [-1, 1, 'Conv', [256, 1, 1]], [-1, 1, 'Conv', [512, 3, 1]],
            [-2, 1, 'Conv', [128, 1, 1]], list(up), [[-1, 6], 1, 'Concat', [1]], [-1, 1, 'Bottleneck', [256, False]], [-1, 2, 'Bottleneck', [256, False]],
            [[27, 22, 15], 1, 'Detect', ['nc']]]


def _v3_cfg(nc, row12):
    return {'nc': nc, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _v3_darknet53(), 'head': _v3_head(row12)}


def _v3_tiny_cfg(nc):
    """models/v3/yolov3-tiny.yaml, row for row: stride-1 3x3 Convs with nn.MaxPool2d(2, 2, 0) between them, nn.ZeroPad2d((0, 1, 0, 1)) + nn.MaxPool2d(2, 1, 0)
    at P5, a two-level head (P4, P5)."""
    backbone = []
    for c in (16, 32, 64, 128, 256):
        backbone += [[-1, 1, 'Conv', [c, 3, 1]], [-1, 1, 'nn.MaxPool2d', [2, 2, 0]]]
    backbone += [[-1, 1, 'Conv', [512, 3, 1]], [-1, 1, 'nn.ZeroPad2d', [[0, 1, 0, 1]]], [-1, 1, 'nn.MaxPool2d', [2, 1, 0]]]
    head = [[-1, 1, 'Conv', [1024, 3, 1]], [-1, 1, 'Conv', [256, 1, 1]], [-1, 1, 'Conv', [512, 3, 1]],
            [-2, 1, 'Conv', [128, 1, 1]], [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']], [[-1, 8], 1, 'Concat', [1]], [-1, 1, 'Conv', [256, 3, 1]],
            [[19, 15], 1, 'Detect', ['nc']]]
    return {'nc': nc, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': backbone, 'head': head}


# YOLOv3 detection graphs: the reference's models/v3/{yolov3,yolov3-spp,yolov3-tiny}.yaml.  They carry depth_multiple / width_multiple (1.0) and no
# `scales` table, and their names hold no scale letter.
V3_CONFIGS = {
    'yolov3': lambda nc=80: _v3_cfg(nc, [-1, 1, 'Conv', [512, 1, 1]]),
    'yolov3-spp': lambda nc=80: _v3_cfg(nc, [-1, 1, 'SPP', [512, [5, 9, 13]]]),
    'yolov3-tiny': lambda nc=80: _v3_tiny_cfg(nc),
}


# every built-in graph by name (the tables above stay apart: CONFIGS lists the detection graphs that have a models/v8/ file)
ALL_CONFIGS = {**CONFIGS, **SEG_CONFIGS, **POSE_CONFIGS, **CLS_CONFIGS, **RTDETR_CONFIGS, **V5_CONFIGS, **V6_CONFIGS, **V3_CONFIGS}


def get_config(name, scale='n', nc=None):
    """cfg dict for `name` in CONFIGS / SEG_CONFIGS / POSE_CONFIGS / CLS_CONFIGS / RTDETR_CONFIGS / V5_CONFIGS / V6_CONFIGS / V3_CONFIGS at compound-scale letter `scale` (like 'yolov8n.yaml' file stems; the
    YOLOv3 graphs have no `scales` table, so the parser never reads it for them)."""
    build = ALL_CONFIGS[name]
    d = build() if nc is None else build(nc)      # nc=None: the YAML file's own class count
    d['scale'] = scale
    d['yaml_file'] = f'{name}.yaml'
    return d
