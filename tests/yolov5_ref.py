"""What the YOLOv5 fixture generator (tests/golden/gen_yolov5.py) and tests/test_yolov5.py share: the seeded cases and inputs, the fixture loader and the
W6 <-> W3 restatement of the stem identity.  No reference code here."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

MODULE_SEED = 31
IMG_SEED = 7
# name -> (C3 constructor arguments (c1, c2, n, shortcut), input shape)
C3_CASES = {
    'c3_odd': ((32, 32, 1, True), (1, 32, 9, 13)),           # odd map
    'c3_n2': ((64, 64, 2, True), (2, 64, 8, 12)),
    'c3_nosc': ((128, 64, 1, False), (1, 128, 8, 12)),        # c1 != c2, no shortcut
    'c3_n3': ((128, 128, 3, True), (1, 128, 6, 10)),          # n = 3
}
STEM_ARGS, STEM_SHAPE = (3, 16, 6, 2, 2), (2, 3, 32, 48)
E2E_SHAPES = {(2, 160, 224): 1, (1, 96, 160): 1, (1, 640, 640): 25}       # shape -> every SUB-th anchor recorded (1: y and the head maps in full)
BF16_QUANTITIES = ('box', 'conf', 'feat')


def case_input(name, shape, seed=MODULE_SEED):
    import zlib
    r = np.random.default_rng([seed, zlib.crc32(name.encode())])
    return torch.from_numpy(r.standard_normal(shape, dtype=np.float32))


def stem_inputs():
    """(float image in [0, 1), uint8 image) of the stem case"""
    r = np.random.default_rng([MODULE_SEED, 66])
    return torch.from_numpy(r.random(STEM_SHAPE, dtype=np.float32)), torch.from_numpy(r.integers(0, 256, STEM_SHAPE, dtype=np.uint8))


def load_fixture():
    """the yolov5_NN.npz shards merged into one dict"""
    out = {}
    paths = sorted(glob.glob(os.path.join(GOLDEN, 'yolov5_[0-9][0-9].npz')))
    assert paths, 'tests/golden/yolov5_NN.npz are missing (python tests/golden/gen_yolov5.py)'
    for p in paths:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def w6_to_w3(w6, cp=None):
    """W3[co, (dy*2+dx)*C + ci, a, b] = W6[co, ci, 2a+dy, 2b+dx], by plain loops (the statement the kernels' index arithmetic is checked against)"""
    co, c = w6.shape[:2]
    w3 = w6.new_zeros(co, cp or 4 * c, 3, 3)
    for dy in range(2):
        for dx in range(2):
            for ci in range(c):
                for a in range(3):
                    for b in range(3):
                        w3[:, (dy * 2 + dx) * c + ci, a, b] = w6[:, ci, 2 * a + dy, 2 * b + dx]
    return w3


def space_to_depth2(x, cp=None):
    """S[b, (dy*2+dx)*C + ci, i, j] = x[b, ci, 2i+dy, 2j+dx] (+ zero channels up to cp), by plain indexing"""
    b, c, h, w = x.shape
    s = x.new_zeros(b, cp or 4 * c, h // 2, w // 2)
    for dy in range(2):
        for dx in range(2):
            s[:, (dy * 2 + dx) * c:(dy * 2 + dx + 1) * c] = x[:, :, dy::2, dx::2]
    return s
