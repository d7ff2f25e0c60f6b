"""What the YOLOv3 fixture generator (tests/golden/gen_yolov3.py), tests/test_yolov3.py and tests/test_pool_kernels.py share: the graphs and their seeded
cases, the fixture loaders, the pooling test inputs and a float64 restatement of SPP's training step.  No reference code here."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from yolov6_ref import BF16_QUANTITIES, INFORMATIVE_COS, NMS_SETTINGS, SCORE_MARGIN, TRAIN_FIGURES, train_figures  # noqa: F401  (shared with the v6 tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

IMG_SEED = 7
E2E_SHAPES = ((2, 64, 96), (1, 96, 160))
FULL_SHAPE = (1, 64, 64)               # the one full-width case (yolov3-spp, 1024-channel layers)
RMS_RANGE = (1e-3, 1e3)                # every row's output rms of the seeded graph must stay inside (else the generator lowers the gain)
NAMES = ('yolov3', 'yolov3-spp', 'yolov3-tiny')
# fixture tag -> (graph name, width_multiple): tiny at full width; the two darknet53 graphs at a quarter of it (both parsers read the key)
GRAPHS = {'tiny': ('yolov3-tiny', 1.0), 'v3_w025': ('yolov3', 0.25), 'spp_w025': ('yolov3-spp', 0.25)}
FULL = ('spp_full', 'yolov3-spp', 1.0)
STRIDES = {'tiny': [16.0, 32.0], 'v3_w025': [8.0, 16.0, 32.0], 'spp_w025': [8.0, 16.0, 32.0], 'spp_full': [8.0, 16.0, 32.0]}
TRAIN = {'tiny': 'train_yolov3_tiny', 'spp_w025': 'train_yolov3_spp_w025'}


def seed_model_(m, seed, gain=1.0):
    """seeding.seed_state_dict_, then every Conv's convolution weight times `gain` (1.0: untouched).  The same call builds the reference's and this project's
    model.  DFL's `dfl.conv.weight` is not a weight but the constant 0 .. reg_max - 1 of the box expectation (requires_grad False; this project's decode
    kernels hold it as a constant): it is left alone, where yolov6_ref.seed_model_ would scale it with the rest (its fixtures use gain 1.0, so it never did)."""
    from mgdt_yolo_amd.seeding import seed_state_dict_
    seed_state_dict_(m, seed)
    if gain != 1.0:
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if k.endswith('.conv.weight') and not k.endswith('dfl.conv.weight'):
                    v.mul_(gain)
    return m


def graph_cfg(name, width=1.0, nc=None):
    """this project's cfg dict of one of the three graphs at `width_multiple` = width"""
    from mgdt_yolo_amd.models import get_config
    d = get_config(name, '', nc)
    d['width_multiple'] = width
    return d


def load_fixture():
    """the yolov3_NN.npz shards merged into one dict (keys `<tag>/<quantity>`)"""
    out = {}
    paths = sorted(glob.glob(os.path.join(GOLDEN, 'yolov3_[0-9][0-9].npz')))
    assert paths, 'tests/golden/yolov3_NN.npz are missing (python tests/golden/gen_yolov3.py)'
    for p in paths:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


class TrainFixture(dict):
    """a training fixture as the dict test_yolov6.check_train_step reads (`files` = its keys)"""

    @property
    def files(self):
        return list(self.keys())


PACKED = ('gst', 'gd64', 'cbf16')      # per-tensor scalars of a training fixture, stored as one array each in the order of `grad_names`


def pack_train(arrs):
    names = str(arrs['grad_names']).split('\n')
    out = {k: v for k, v in arrs.items() if k.split('/')[0] not in PACKED}
    for p in PACKED:
        out[p] = np.stack([np.asarray(arrs[f'{p}/{k}'], np.float64) for k in names])
    return out


def load_train(tag):
    """the training fixture in the per-name layout of train_yolov6_n.npz"""
    with np.load(os.path.join(GOLDEN, TRAIN[tag] + '.npz')) as z:
        g = TrainFixture({k: z[k] for k in z.files if k not in PACKED})
        for p in PACKED:
            for k, v in zip(str(z['grad_names']).split('\n'), z[p]):
                g[f'{p}/{k}'] = v
    return g


# ------------------------------------------------------------------------------------------------ pooling test inputs
def pool_input(gen, B, C, H, W, kind):
    """float64 CPU input of a pooling case.  'quant': three levels, ties everywhere; 'neg': all negative (behind ZeroPad2d every border window's maximum is
    the pad zero); 'zeros': exact zeros and -0.0 mixed with negatives (the scan order decides between a pixel and the pad); 'pool': itself a 5x5 max-pool
    output (plateaus); 'nan': 'quant' with two NaNs; 'rand': untied normal values."""
    if kind == 'rand':
        return torch.randn(B, C, H, W, generator=gen).double()
    if kind == 'pool':
        return F.max_pool2d(torch.randint(0, 4, (B, C, H, W), generator=gen).double(), 5, 1, 2)
    if kind == 'neg':
        return -1.0 - torch.randint(0, 3, (B, C, H, W), generator=gen).double()
    if kind == 'zeros':
        lv = torch.tensor([-1.0, -0.0, 0.0, -0.5], dtype=torch.float64)
        x = lv[torch.randint(0, 4, (B, C, H, W), generator=gen)]
        x[:, :, -1, :] = lv[torch.randint(1, 3, (B, C, W), generator=gen)]            # the border the pad touches: +-0 only
        x[:, :, :, -1] = lv[torch.randint(1, 3, (B, C, H), generator=gen)]
        return x
    x = torch.randint(0, 3, (B, C, H, W), generator=gen).double()
    if kind == 'nan':
        x[0, 1 % C, H // 2, W // 2] = float('nan')
        x[-1, C - 1, 0, 0] = float('nan')
    return x


def spp_step(sd, x, gz, mode, mom, eps=1e-3):
    """One training step of SPP (cv1, the identity and the three DIRECT stride-1 max pools 5 / 9 / 13, cv2) through tests/train_ref.py's Conv restatement:
    mode 'f64' the reference, 'f32' the same in float32 on the CPU, 'bf16' float64 with the two-way bfloat16 rounding hook.  Returns the quantities
    {y0, dx0, g:<key>, rm:<prefix>, rv:<prefix>} as float64 tensors."""
    import train_ref as TR
    dt = torch.float32 if mode == 'f32' else torch.float64
    rnd = TR.round_bf16 if mode == 'bf16' else TR.identity
    rb = (lambda t: t.to(torch.bfloat16).to(t.dtype)) if mode == 'bf16' else (lambda t: t)
    p = {k: v.detach().to(dt).clone().requires_grad_('running' not in k) for k, v in sd.items() if v.dtype.is_floating_point}
    xin = x.detach().to(dt).clone().requires_grad_(True)
    c = TR._Ref(p, rnd, None, mom, eps)
    x0 = c.cba('cv1', rnd(xin))
    y = c.cba('cv2', torch.cat([x0] + [rnd(F.max_pool2d(x0, k, 1, k // 2)) for k in (5, 9, 13)], 1))
    y.backward(rb(gz.detach().to(dt)))
    q = {'y0': y.detach().double(), 'dx0': xin.grad.double()}
    q.update({'g:' + k: v.grad.double() for k, v in p.items() if v.requires_grad})
    for k, (rm, rv) in c.running.items():
        q['rm:' + k], q['rv:' + k] = rm.detach().double(), rv.detach().double()
    return q
