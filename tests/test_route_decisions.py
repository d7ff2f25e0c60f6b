"""Which modules take their fused route, decided on the CPU: every site of DESIGN section 3a x every way a module can stop being what its kernel
computes.  No launch is issued: the `*_supported` queries and `conv_can_mfma` work on CPU tensors, the packed panels are replaced by a stand-in.

EXPECTED was produced by running this table against the commit before the shared predicate (Conv.plain / watched / fp8_claims) existed, with only the
names of the private entry points adapted.  It is that commit's answer in every cell except the dilation / padding cells of the sites that lacked those
tests (listed in NEW_GEOMETRY): there a fused route would have computed dilation 1 / 'same' padding where the composed route raises in
Conv._geometry, and the expected value is "not fused".  A cell that does not apply to a site (padding 0 on a 3x3 where the site has none) is absent."""
import pytest
import torch
import torch.nn as nn

from mgdt_yolo_amd import ops
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.nn.modules import C2f, C3, IFM, SPPF, Classify, Conv, Detect, InjectionMultiSum_Auto_pool, MSPA_C2f, Pose, SimFusion_3in
from mgdt_yolo_amd.nn.modules.convnextv2 import ConvNeXtV2_Block
from mgdt_yolo_amd.yolo.utils.torch_utils import fuse_conv_and_bn

BF16 = torch.bfloat16


def act(c, h=16, w=16):
    return ops.new_act(1, c, h, w, BF16, 'cpu').zero_()


# -- the sites: module (what .train() / a module hook goes on), conv (the convolution that is perturbed), conv3 (a 3x3 one, where the site has one),
#    child / grandchild (hook and _q8 targets), and the inputs of the decision -----------------------------------------------------------------
def _c2f():
    m = C2f(32, 32, 1).eval()
    return dict(module=m, conv=m.cv1, conv3=m.m[0].cv2, child=m.cv1, grandchild=m.m[0].cv1, x=act(32))


def _mspa():
    m = MSPA_C2f(64, 64, 1).eval()
    return dict(module=m, conv=m.convs[0], conv3=m.bottleneck[0].cv2, child=m.convs[0], grandchild=m.bottleneck[0].cv1, x=act(64))


def _c3():
    m = C3(32, 32, 1).eval()
    return dict(module=m, conv=m.cv1, conv3=m.m[0].cv2, child=m.cv1, grandchild=m.m[0].cv1, x=act(32))


def _sppf():
    m = SPPF(64, 64).eval()
    return dict(module=m, conv=m.cv1, child=m.cv1, grandchild=m.cv1.conv, x=act(64))


def _laf():
    m = SimFusion_3in([32, 64, 64], 64).eval()
    return dict(module=m, conv=m.cv1, child=m.cv1, grandchild=m.cv1.conv, pooled0=act(32), cat=act(192), x2=act(64, 8, 8))


def _inject(conv_of):
    def build():
        m = InjectionMultiSum_Auto_pool(64, 256, [32, 32], 0).eval()               # the injection + conv kernel is built for 256 channels
        c = conv_of(m)
        return dict(module=m, conv=c, child=c, grandchild=c.conv, x=[act(64), act(64, 8, 8)], consumer=Conv(256, 64, 1).eval())
    return build


def _ifm():
    m = IFM(64, [32, 32], embed_dim_p=64, fuse_block_num=1).eval()
    tail = m.conv[-1]
    return dict(module=m, conv=tail, child=tail, grandchild=tail.conv)


def _detect(j):
    def build():
        m = Detect(nc=80, ch=(64,)).eval()
        c = m.cv2[0][j]
        return dict(module=m, conv=c, conv3=c, child=c, grandchild=c.conv, x=act(64), tb=act(16), tc=act(80))
    return build


def _pose():
    m = Pose(nc=1, kpt_shape=(17, 3), ch=(64,)).eval()
    c = m.cv4[0][0]
    return dict(module=m, conv=c, conv3=c, child=c, grandchild=c.conv, x=act(64))


def _classify():
    m = Classify(64, 10).eval()
    return dict(module=m, conv=m.conv, child=m.conv, grandchild=m.conv.conv, x=act(64))


def _stem():
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(get_config('yolov8', 'n'), verbose=False).eval().set_compute_dtype(BF16)
    c = m.model[0]
    return dict(module=m, conv=c, conv3=c, child=c, grandchild=c.conv, x=torch.zeros(1, 3, 64, 64, dtype=BF16))


BUILD = {'c2f': _c2f, 'mspa_c2f': _mspa, 'c3': _c3, 'sppf': _sppf, 'laf': _laf, 'inject_global': _inject(lambda m: m.global_act),
         'inject_conv': _inject(lambda m: m.local_embedding), 'cnx_tail': _ifm, 'detect_first': _detect(0), 'detect_box3': _detect(1), 'pose_kpt': _pose,
         'classify': _classify, 'stem': _stem}

# the private entry point of each decision (the only part that was adapted to produce EXPECTED)
DECIDE = {
    'c2f': lambda s: s['module']._fused_route(s['x']) is not None,
    'mspa_c2f': lambda s: s['module']._fused_route(s['x']) is not None,
    'c3': lambda s: s['module']._fused_route(s['x']) is not None,
    'sppf': lambda s: s['module']._fused_route(s['x']) is not None,
    'laf': lambda s: s['module']._laf_route(s['pooled0'], s['cat'][:, 64:128], s['x2'], BF16) is not None,
    'inject_global': lambda s: s['module']._merged_global(s['x'][1][:, :32]) is not None,
    'inject_conv': lambda s: s['module']._into_conv_route(s['x'], s['consumer']) is not None,
    'cnx_tail': lambda s: bool(s['module']._tail_in_block()) and ConvNeXtV2_Block._tail_panel(s['conv'], 64, BF16) is not None,
    'detect_first': lambda s: s['module']._merged_first(0, s['x'], BF16) is not None,
    'detect_box3': lambda s: s['module']._box3_in_tail(0, s['tb'], s['tc'], BF16) is not None,
    'pose_kpt': lambda s: s['module']._kpt_padded(0, s['x']),
    'classify': lambda s: bool(s['module']._fusable(s['x'], BF16)),
    'stem': lambda s: bool(s['module']._stem_fusable(s['x'])),
}


# -- the perturbations --------------------------------------------------------------------------------------------------------------------------------
def _fuse(s):
    for m in s['module'].modules():                        # BaseModel.fuse()
        if isinstance(m, Conv) and hasattr(m, 'bn'):
            m.conv = fuse_conv_and_bn(m.conv, m.bn)
            delattr(m, 'bn')
    for k, v in s.items():                                 # the nn.Conv2d objects were replaced
        if isinstance(v, nn.Conv2d):
            s[k] = s['child'].conv


def _set(name, value):
    return lambda s: setattr(s['conv'].conv, name, value)


def _hook(key):
    return lambda s: s[key].register_forward_hook(lambda *a: None)


PERTURB = {
    'none': lambda s: None,
    'fuse': _fuse,
    'train': lambda s: s['module'].train(),
    'relu': lambda s: setattr(s['conv'], 'act', nn.ReLU()),
    'gelu': lambda s: setattr(s['conv'], 'act', nn.GELU()),
    'stride2': _set('stride', (2, 2)),
    'groups2': _set('groups', 2),
    'dilation2': _set('dilation', (2, 2)),
    'pad0_on_3x3': lambda s: setattr(s['conv3'].conv, 'padding', (0, 0)),
    'hook_module': _hook('module'),
    'hook_child': _hook('child'),
    'hook_grandchild': _hook('grandchild'),
    'q8_child': lambda s: s['child'].__dict__.__setitem__('_q8', {None: 1.0}),
    'q8_calib': lambda s: setattr(ops, 'Q8_CALIB', {}),
}

# one character per perturbation, in PERTURB's order: F fused, . not fused, - does not apply.  PARENT: the commit before Conv.plain, where E marks a
# fused route that was chosen and then raised in Conv._geometry while packing its own panel.
PARENT = {
    'c2f':           'FF.....FFFFFFF',
    'mspa_c2f':      'FF.....FFFFFFF',
    'c3':            'FF......FF....',
    'sppf':          'FF.F...F-..F..',
    'laf':           'FF.F...F-.....',
    'inject_global': 'FFF..F.F-FFFFF',
    'inject_conv':   'FF...F.E-FFF..',
    'cnx_tail':      'FF.FF..F-F.F..',
    'detect_first':  'FFF....FFFFFFF',
    'detect_box3':   'FF.....EEF.F..',
    'pose_kpt':      'FFF......F.FFF',
    'classify':      'FF......-F.FFF',
    'stem':          'FFF..F.F.F.FFF',
}
GEOMETRY = ('dilation2', 'pad0_on_3x3')
EXPECTED = {site: {p: c == 'F' and p not in GEOMETRY for p, c in zip(PERTURB, row) if c != '-'} for site, row in PARENT.items()}
NEW_GEOMETRY = {(site, p) for site, row in PARENT.items() for p, c in zip(PERTURB, row) if p in GEOMETRY and c in 'FE'}


def decide(site, pert):
    s = BUILD[site]()
    PERTURB[pert](s)
    return bool(DECIDE[site](s))


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """panels are never packed (packing launches), every C3 class may fuse, and what a perturbation sets on `ops` is put back"""
    for name in ('PackedConv', 'PackedConvFp8'):
        monkeypatch.setattr(ops, name, lambda *a, **k: object())
    monkeypatch.setattr(ops, 'C3_FUSED_CLASSES', None)
    monkeypatch.setattr(ops, 'Q8_CALIB', None)


CELLS = [(site, pert) for site in BUILD for pert in PERTURB if not (pert == 'pad0_on_3x3' and site not in
                                                                    ('c2f', 'mspa_c2f', 'c3', 'detect_first', 'detect_box3', 'pose_kpt', 'stem'))]


@pytest.mark.parametrize('site,pert', CELLS, ids=[f'{s}-{p}' for s, p in CELLS])
def test_route_decision(site, pert):
    assert decide(site, pert) == EXPECTED[site][pert]


def test_table_covers_every_cell_and_every_unperturbed_module_fuses():
    assert {(s, p) for s in EXPECTED for p in EXPECTED[s]} == set(CELLS) and len(NEW_GEOMETRY) == 15
    assert all(EXPECTED[site]['none'] and EXPECTED[site]['fuse'] for site in BUILD)
