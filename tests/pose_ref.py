"""Helpers shared by tests/test_pose.py and tests/golden/gen_pose.py: the fixture loader, the seeded inputs that are re-created instead of stored,
and plain-torch restatements of the reference's keypoint arithmetic (nn/modules/head.py:239-253 kpts_decode, yolo/utils/ops.py:636-666
scale_coords).  No reference import here."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
IMG_SEED = 3
LB_SHAPE = (134, 224)            # original images of the predictor case: letter-box into 160 x 224 by padding 13 rows of 114 above and below
# fixture tag -> (config name, kpt_shape, input shape)
CASES = {'yolov8_pose_n_2x96x160': ('yolov8-pose', (17, 3), (2, 96, 160)),
         'yolov8_pose_n_1x160x224': ('yolov8-pose', (17, 3), (1, 160, 224)),
         'yolov8_pose_k5x2_n_2x96x160': ('yolov8-pose', (5, 2), (2, 96, 160)),
         'mspa_c2f_gd_pose_n_2x96x160': ('mspa_c2f_gd_yolov8-pose', (17, 3), (2, 96, 160))}
FULL = 'yolov8_pose_n_2x96x160'
NMS_CASES = ('pred', 'val', 'agn', 'few')
COORD_CASES = {'wide': (120, 200), 'tall': (200, 120)}       # original shapes letter-boxed into 160 x 224: gain limited by the width / by the height
IN_SHAPE = (160, 224)
QUANTITIES = ('box', 'conf', 'kxy', 'kvis')


def seed_pose_(m, seed=0):
    """seed_state_dict_, then the keypoint branch's closing 1x1 `cv4.N.2.weight` scaled by 0.01, in the spirit of the x 0.05 its name rules give
    Detect's closing 1x1 convolutions (outputs O(1), as a trained head's).  Unscaled, the raw keypoint values reach +-8 on yolov8-pose and +-150
    on the MSPA-GD graph (whose seeded head inputs are about 15x larger), i.e. offsets of tens of cells: a bf16 rounding error of a few percent
    of that is tens of pixels, and no keypoint bound could tell a wrong anchor offset (half a cell) from rounding.  With 0.01 the raw values stay
    within +-1.5 (offsets of at most 3 cells) on both graphs.  The rule cannot move into seeding.py: the Segment fixtures are generated with
    their cv4 unscaled.  In place; returns m."""
    import re
    from mgdt_yolo_amd.seeding import seed_state_dict_
    seed_state_dict_(m, seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if re.search(r'cv4\.\d+\.2\.weight$', name):
                p.mul_(0.01)
    return m


def load_fixture():
    """All arrays of tests/golden/pose_NN.npz as one dict."""
    import glob
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'pose_[0-9][0-9].npz'))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    assert out, 'tests/golden/pose_NN.npz are missing'
    return out


def settings(g, key):
    """A JSON settings record of the fixture (NMS keyword arguments, predictor arguments)."""
    return json.loads(str(g[key]))


def lb_images(shape=LB_SHAPE):
    """The two seeded BGR uint8 images of the predictor case (re-created, not stored)."""
    r = np.random.default_rng([43, 11])
    return [r.integers(0, 256, (*shape, 3), dtype=np.uint8) for _ in range(2)]


def seeded_coords(name, n=48, k=17, ndim=3):
    """(n, k, ndim) float32 keypoints around a 160 x 224 frame, a good part of them outside it, visibility in [0, 1)."""
    r = np.random.default_rng([47, sum(map(ord, name))])
    c = r.uniform(-40.0, 270.0, (n, k, ndim)).astype(np.float32)
    if ndim == 3:
        c[..., 2] = r.random((n, k), dtype=np.float32)
    return c


def split(pred, nc, kpt_shape):
    """(B, 4+nc+nk, A) array -> dict of the four quantities the tolerances are stated for."""
    nd = kpt_shape[1]
    k = pred[:, 4 + nc:]
    idx = np.arange(k.shape[1])
    out = {'box': pred[:, :4], 'conf': pred[:, 4:4 + nc], 'kxy': k[:, idx % nd < 2]}
    out['kvis'] = k[:, idx % nd == 2] if nd == 3 else k[:, :0]
    return out


def max_diffs(a, b, nc, kpt_shape):
    sa, sb = split(a, nc, kpt_shape), split(b, nc, kpt_shape)
    return {q: (float(np.abs(sa[q].astype(np.float64) - sb[q].astype(np.float64)).max()) if sa[q].size else 0.0) for q in QUANTITIES}


def kpts_decode(kpt, level_hw, strides, ndim):
    """head.py:246-252 on a raw (B, nk, A) float32 tensor (any device), with make_anchors' x + 0.5 centres: float32, the reference's operation order."""
    ax, ay, st = [], [], []
    for (h, w), s in zip(level_hw, strides):
        sx = torch.arange(w, device=kpt.device, dtype=torch.float32) + 0.5
        sy = torch.arange(h, device=kpt.device, dtype=torch.float32) + 0.5
        gy, gx = torch.meshgrid(sy, sx, indexing='ij')
        ax.append(gx.reshape(-1)); ay.append(gy.reshape(-1)); st.append(torch.full((h * w,), float(s), device=kpt.device))
    ax, ay, st = torch.cat(ax), torch.cat(ay), torch.cat(st)
    y = kpt.clone()
    if ndim == 3:
        y[:, 2::3] = y[:, 2::3].sigmoid()
    y[:, 0::ndim] = (y[:, 0::ndim] * 2.0 + (ax - 0.5)) * st
    y[:, 1::ndim] = (y[:, 1::ndim] * 2.0 + (ay - 0.5)) * st
    return y
