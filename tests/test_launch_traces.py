"""The launch sequence of every graph, call form by call form, pinned to tests/launch_traces.json.

A case is one model at scale n, one input and one way of calling it; its trace is the list of kernel names `ops._launch` issues for one call after
a warm call (so no pack launches appear; training traces are the second step's forward + `model.backward`).  Comparison is exact list equality:
host-side work that is meant to leave routing alone must leave every list alone, and work that changes routing re-records the file
(`python tests/test_launch_traces.py` on the GPU), whose diff is then the reviewable statement of what changed.

The two darknet53 graphs (yolov3, yolov3-spp) have no scale table; they run at width_multiple 0.25, the width the YOLOv3 tests use."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.models import get_config  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images, seeded_labels  # noqa: E402

DEV = 'cuda:0'
TRACES = os.path.join(ROOT, 'tests', 'launch_traces.json')
BF16, F32 = torch.bfloat16, torch.float32
FLAGSHIP = 'mspa_c2f_gd_yolov8'
OTHERS = ('yolov8', 'gd_yolov8', 'mspa_c2f_yolov8', 'mspa_c2f_gd_tood_yolov8', 'yolov5', 'yolov6', 'yolov3-spp', 'yolov3-tiny', 'yolov8-seg', 'yolov8-pose',
          'yolov8-cls', 'yolov8-rtdetr')
SIZES = {'yolov5': (160, 224), 'yolov8-cls': (64, 64)}              # everything else: 160 x 160
CASES = ([(FLAGSHIP, form) for form in ('bf16', 'f32', 'u8', 'fused', 'fp8', 'no_side_stream', 'train_f32', 'train_bf16')]
         + [(name, form) for name in OTHERS for form in ('bf16', 'f32')])


def _model(name, dt, nc=None):
    from mgdt_yolo_amd.nn.tasks import model_class_of
    cfg = get_config(name, 'n', nc)
    if name in ('yolov3', 'yolov3-spp'):
        cfg['width_multiple'] = 0.25
    return seed_state_dict_(model_class_of(cfg)(cfg, verbose=False), 0).to(DEV).set_compute_dtype(dt)


def _recorded(fn):
    """names of the launches `fn` issues"""
    names, orig = [], ops._launch
    ops._launch = lambda name, *a, **k: (names.append(name), orig(name, *a, **k))[1]
    try:
        fn()
    finally:
        ops._launch = orig
    return names


def trace(name, form):
    h, w = SIZES.get(name, (160, 160))
    x = seeded_images(2, h, w, seed=7).to(DEV)
    if form.startswith('train'):
        from mgdt_yolo_amd.yolo.utils.loss import loss_and_head_grads, v8DetectionLoss
        m = _model(name, F32 if form == 'train_f32' else BF16, nc=4).train()
        crit, lab = v8DetectionLoss(m), seeded_labels(2, 4, seed=4, max_boxes=4, min_boxes=2)
        names = []
        for _ in range(2):                                   # the second step is the recorded one
            feats = []
            names = _recorded(lambda: feats.extend(m._predict_once(x)))
            hg = loss_and_head_grads(crit, feats, lab)[2]
            names += _recorded(lambda: m.backward(hg))
        return names
    m = _model(name, F32 if form == 'f32' else BF16).eval()
    side = ops.SIDE_STREAM
    try:
        with torch.no_grad():
            if form == 'u8':
                x = (x * 255).round().to(torch.uint8)
            elif form == 'fused':
                m.fuse()
            elif form == 'fp8':
                m.quantize_fp8(seeded_images(2, h, w, seed=8).to(DEV))
            elif form == 'no_side_stream':
                ops.SIDE_STREAM = False
            m(x)
            names = _recorded(lambda: m(x))
    finally:
        ops.SIDE_STREAM = side
    torch.cuda.synchronize()
    return names


@pytest.fixture(scope='module')
def recorded():
    return json.load(open(TRACES))


@pytest.mark.gpu
@pytest.mark.parametrize('name,form', CASES, ids=[f'{n}-{f}' for n, f in CASES])
def test_launch_sequence_equals_the_recorded_one(recorded, name, form):
    want = recorded[f'{name}/{form}']
    got = trace(name, form)
    assert len(want) > 0
    assert got == want, next(f'launch {i}: {g} instead of {w}' for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w)


def test_every_case_is_recorded():
    assert sorted(json.load(open(TRACES))) == sorted(f'{n}/{f}' for n, f in CASES)


if __name__ == '__main__':
    out = {}
    for n, f in CASES:
        out[f'{n}/{f}'] = trace(n, f)
        print(f'{n}/{f}: {len(out[f"{n}/{f}"])} launches', flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else TRACES, 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write('\n')
