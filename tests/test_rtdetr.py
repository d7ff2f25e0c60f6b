"""RT-DETR inference: the RTDETRDecoder head kernels against the float64 restatements of tests/rtdetr_ref.py, and the model against the reference's
recorded outputs (tests/golden/rtdetr_NN.npz, written by tests/golden/gen_rtdetr.py).

Kernel bounds: fp32 = max(1e-6, 8 x |restatement run in fp32 on the CPU - restatement in float64|), computed here from the restatement alone;
bf16 (the value tensor of the deformable attention) = 3 x |restatement on bf16-rounded inputs and value - float64 restatement on the unrounded ones|.
Model bounds: fp32: the project's 1e-3 px / 1e-4 contract, or 8 x the recorded fp32-vs-fp64 difference where that is larger; bf16: 3 x the recorded
difference of the generator's bf16 emulation, with the recorded query indices forced (the selection is the one discontinuous step)."""
import json
import os

import numpy as np
import pytest
import torch

import rtdetr_ref as RR
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
DEV = 'cuda:0'
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return RR.load_fixtures(GOLDEN)


def build_model(tag, device='cpu'):
    from mgdt_yolo_amd.nn.tasks import RTDETRDetectionModel
    m = RTDETRDetectionModel(RR.case_cfg(tag), nc=RR.CASES[tag][1], verbose=False)
    return seed_state_dict_(m, RR.WEIGHT_SEED).eval().to(device)


def g(seed):
    return torch.Generator().manual_seed(seed)


def fp32_bound(fn, *args):
    """(float64 result, bound): max(1e-6, 8 x the largest difference of the restatement run in fp32 on the CPU to the float64 one)"""
    cast = lambda a, dt: a.to(dt) if torch.is_tensor(a) and a.is_floating_point() else a
    r64 = fn(*[cast(a, torch.float64) for a in args])
    r32 = fn(*[cast(a, torch.float32) for a in args])
    return r64, max(1e-6, 8 * float((r32.double() - r64).abs().max()))


def close(got, want64, bound, what):
    d = float((got.detach().cpu().double() - want64).abs().max())
    print(f'{what}: max |d| {d:.3e}, bound {bound:.3e}')
    assert d <= bound, (what, d, bound)


# ================================================================================================================ CPU
def test_restatements_reproduce_the_fixtures(fx):
    """Chained with the recorded indices, the restatements give the reference's float64 outputs of cases C and D within 1e-9, every decoder layer
    included; free-running, the stable selection is the recorded one."""
    for tag in RR.CHAINED:
        nq, ndl = RR.case_nq_ndl(tag)
        sd = RR.head_state(build_model(tag))
        feats = [torch.from_numpy(fx[f'{tag}_input64_{i}']) for i in range(3)]
        idx = torch.from_numpy(fx[f'{tag}_index'])
        trace = []
        out = RR.head_forward(sd, feats, nq, ndl, index=idx, trace=trace)
        for k in ('enc_bboxes', 'enc_scores', 'dec_bboxes', 'dec_scores', 'score_max'):
            d = float((out[k] - torch.from_numpy(fx[f'{tag}_{k}64'])).abs().max())
            print(tag, k, f'{d:.3e}')
            assert d < 1e-9, (tag, k, d)
        d = float((torch.stack(trace) - torch.from_numpy(fx[f'{tag}_layers64'])).abs().max())
        assert d < 1e-9, (tag, 'layers', d)
        free = RR.head_forward(sd, feats, nq, ndl)
        assert torch.equal(free['index'], idx)


def test_anchor_restatement_counts_the_invalid_tokens(fx):
    for tag, want in (('A', 0), ('B', 168), ('C', 126), ('D', 0)):
        _, _, (b, h, w) = RR.CASES[tag]
        anc, valid = RR.anchors(RR.level_shapes(h, w), torch.float32)
        assert int((~valid).sum()) == want == int(fx[f'{tag}_ninvalid'])
        assert bool(torch.isinf(anc[~valid]).all()) and bool(torch.isfinite(anc[valid]).all())


def test_post_restatement_gives_the_predictor_rows(fx):
    conf = float(fx['A_pred_conf'])
    rows = RR.post(torch.from_numpy(fx['A_dec_bboxes']), torch.from_numpy(fx['A_dec_scores']), conf)
    for i, r in enumerate(rows):
        want = fx[f'A_pred_rows_{i}']
        assert r.shape == want.shape and 5 <= len(r) <= 295
        np.testing.assert_allclose(r.numpy(), want, atol=1e-7, rtol=0)


def test_stable_topk_restatement():
    s = torch.tensor([[1., 3., 3., 0., 3., 2.]])
    assert RR.stable_topk(s, 4).tolist() == [[1, 2, 4, 5]]


@pytest.mark.parametrize('tag', ['A', 'C'])
def test_parse_model_builds_the_recorded_graph(fx, tag):
    m = build_model(tag)
    sd = m.state_dict()
    assert list(sd.keys()) == list(fx[f'{tag}_keys'])
    assert [','.join(map(str, v.shape)) for v in sd.values()] == list(fx[f'{tag}_shapes'])
    assert sum(p.numel() for p in m.parameters()) == int(fx[f'{tag}_nparams'])
    assert m.stride.tolist() == fx[f'{tag}_stride'].tolist() == [32.0]
    h = m.model[-1]
    nq, ndl = RR.case_nq_ndl(tag)
    assert (h.num_queries, h.num_decoder_layers, h.nc, h.nl) == (nq, ndl, RR.CASES[tag][1], 3)


def test_graph_table_and_model_class(fx):
    from mgdt_yolo_amd.models import get_config
    from mgdt_yolo_amd.nn.tasks import DetectionModel, RTDETRDetectionModel, guess_model_task, model_class_of, parse_model, yaml_model_load
    ref = json.load(open(os.path.join(GOLDEN, 'rtdetr_yaml.json')))
    cfg = get_config('yolov8-rtdetr', 'n')
    norm = lambda rows: json.loads(json.dumps(rows))
    assert norm(cfg['backbone']) == ref['backbone'] and norm(cfg['head']) == ref['head'] and cfg['nc'] == ref['nc']
    assert {k: list(v) for k, v in cfg['scales'].items()} == ref['scales']
    assert model_class_of(cfg) is RTDETRDetectionModel and guess_model_task(cfg) == 'detect'
    assert model_class_of(get_config('yolov8', 'n')) is DetectionModel
    assert yaml_model_load('yolov8n-rtdetr.yaml')['head'][-1][2] == 'RTDETRDecoder'
    bad = get_config('yolov8-rtdetr', 'n')
    bad['backbone'][0] = [-1, 1, 'HGStem', [32, 48]]                      # the rtdetr-l / rtdetr-x graphs stay unbuilt
    with pytest.raises(KeyError):
        parse_model(bad, 3, verbose=False)


def test_deterministic_initial_values(fx):
    from mgdt_yolo_amd.nn.tasks import RTDETRDetectionModel
    for tag in ('A', 'C'):
        h = RTDETRDetectionModel(RR.case_cfg(tag), nc=RR.CASES[tag][1], verbose=False).model[-1]
        l0 = h.decoder.layers[0].cross_attn
        assert np.array_equal(l0.sampling_offsets.bias.detach().numpy(), fx[f'{tag}_init_offsets_bias'])
        assert np.array_equal(h.enc_score_head.bias.detach().numpy(), fx[f'{tag}_init_enc_score_bias'])
        for lin in [h.enc_bbox_head.layers[-1]] + [b.layers[-1] for b in h.dec_bbox_head]:
            assert float(lin.weight.abs().max()) == 0.0 and float(lin.bias.abs().max()) == 0.0
        for cls_ in h.dec_score_head:
            assert np.array_equal(cls_.bias.detach().numpy(), fx[f'{tag}_init_enc_score_bias'])
        for l in h.decoder.layers:
            assert float(l.cross_attn.attention_weights.weight.abs().max()) == 0.0 and float(l.cross_attn.attention_weights.bias.abs().max()) == 0.0
            assert float(l.cross_attn.sampling_offsets.weight.abs().max()) == 0.0


def test_what_is_not_built_raises():
    from mgdt_yolo_amd.nn.modules import RTDETRDecoder
    m = build_model('C')
    x = torch.zeros(1, 3, 96, 160)
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.init_criterion()
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.loss({'img': x})
    with pytest.raises(NotImplementedError, match='training is not built'):
        m({'img': x})
    with pytest.raises(RuntimeError, match='augment=True is not built'):
        m(x, augment=True)
    with pytest.raises(NotImplementedError, match='training is not built'):
        m.model[-1].train()([x, x, x])
    for kw in (dict(hd=128), dict(nh=4), dict(ndp=8), dict(ch=(8, 8, 8, 8, 8)), dict(learnt_init_query=True)):
        with pytest.raises(NotImplementedError):
            RTDETRDecoder(**{'nc': 3, 'ch': (64, 128, 256), **kw})


def test_new_symbols_are_bound():
    from mgdt_yolo_amd import _lib
    names = ('mgdt_msdeform_attn_fwd', 'mgdt_mha_fwd', 'mgdt_add_layernorm_fwd', 'mgdt_rtdetr_rowmax_fwd', 'mgdt_rtdetr_topk_fwd', 'mgdt_rtdetr_gather_fwd',
             'mgdt_rtdetr_ref_init_fwd', 'mgdt_rtdetr_refine_fwd', 'mgdt_rtdetr_sigmoid_fwd', 'mgdt_rtdetr_post_fwd')
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'mgdt.h')).read()
    lib = _lib.lib()
    for n in names:
        assert n in _lib.PROTOTYPES and f'int {n}(' in hdr and hasattr(lib, n), n


# ================================================================================================================ GPU: kernels
DEFORM_SHAPES = [(5, 7), (3, 4), (2, 2)]


def deform_inputs():
    B, nq, nl = 2, 37, 3
    L = sum(h * w for h, w in DEFORM_SHAPES)
    value = torch.randn(B, L, 256, generator=g(1))
    ref = torch.rand(B, nq, 4, generator=g(2))
    off = torch.randn(B, nq, 8 * nl * 4 * 2, generator=g(3)) * 3
    wl = torch.randn(B, nq, 8 * nl * 4, generator=g(4)) * 2
    ref[0, 0] = torch.tensor([0.5, 0.5, 0.0, 0.5])                       # a box of width 0
    ref[0, 1] = 1.0                                                      # a box of all ones
    ref[0, 2] = torch.tensor([0.0, 1.0, 1.0, 1.0])                       # the centre on two borders
    off[0, 3] = 0.0                                                      # exactly a pixel centre of level 0: ((3 + 0.5) / 7, (2 + 0.5) / 5)
    ref[0, 3] = torch.tensor([3.5 / 7, 2.5 / 5, 0.3, 0.3])
    off[0, 4] = 0.0                                                      # exactly on the border of every map
    ref[0, 4] = torch.tensor([1.0, 0.0, 0.2, 0.2])
    loc = ref[:, :, None, :2] + off.reshape(B, nq, -1, 2) / 4 * ref[:, :, None, 2:] * 0.5
    assert float(loc[..., 0].min()) < 0 and float(loc[..., 0].max()) > 1 and float(loc[..., 1].min()) < 0 and float(loc[..., 1].max()) > 1
    return value, ref, off, wl


@gpu
def test_msdeform_attn_fp32():
    from mgdt_yolo_amd import ops
    value, ref, off, wl = deform_inputs()
    want, bound = fp32_bound(lambda v, r, o, w: RR.deform_attn(v, DEFORM_SHAPES, r, o, w), value, ref, off, wl)
    d = lambda t: t.to(DEV)
    close(ops.msdeform_attn(d(value), DEFORM_SHAPES, d(ref), d(off), d(wl)), want, bound, 'msdeform fp32')
    # the layouts the head hands over: a 256-column slice of a wider value matrix, offsets and weights as column slices of one panel
    wide = torch.randn(2, value.shape[1], 512, generator=g(5))
    wide[..., 256:] = value
    panel = torch.cat([off, wl], -1)
    got = ops.msdeform_attn(d(wide)[..., 256:], DEFORM_SHAPES, d(ref), d(panel)[..., :off.shape[-1]], d(panel)[..., off.shape[-1]:])
    close(got, want, bound, 'msdeform fp32, sliced operands')


@gpu
def test_msdeform_attn_bf16_value():
    from mgdt_yolo_amd import ops
    value, ref, off, wl = deform_inputs()
    r = lambda t: t.to(torch.bfloat16).to(torch.float64)
    want = RR.deform_attn(value.double(), DEFORM_SHAPES, ref.double(), off.double(), wl.double())
    emu = RR.deform_attn(r(value), DEFORM_SHAPES, r(ref), r(off), r(wl))
    bound = 3 * float((emu - want).abs().max())
    got = ops.msdeform_attn(value.to(DEV).to(torch.bfloat16), DEFORM_SHAPES, r(ref).float().to(DEV), r(off).float().to(DEV), r(wl).float().to(DEV))
    assert got.dtype == torch.float32
    close(got, want, bound, 'msdeform bf16 value')


@gpu
@pytest.mark.parametrize('nq', [300, 100, 37])
def test_mha(nq):
    from mgdt_yolo_amd import ops
    q, k, v = (torch.randn(2, nq, 256, generator=g(10 + i)) for i in range(3))
    sp = lambda t: t.reshape(2, nq, 8, 32).permute(0, 2, 1, 3)
    peak = float(((sp(q) @ sp(k).transpose(-1, -2)) / 32 ** 0.5).abs().max())
    q = q * (60.0 / peak)                                                # logits reach +-60: exp() of them overflows fp32 without the maximum
    want, bound = fp32_bound(RR.mha, q, k, v)
    assert bool(torch.isfinite(want).all())
    d = lambda t: t.to(DEV)
    close(ops.mha(d(q), d(k), d(v)), want, bound, f'mha nq {nq}')
    qk = torch.cat([q, k], -1).to(DEV)                                   # the head's layout: q and k as column slices of one matrix
    close(ops.mha(qk[..., :256], qk[..., 256:], d(v)), want, bound, f'mha nq {nq}, sliced q / k')


@gpu
def test_add_layernorm():
    from mgdt_yolo_amd import ops
    x, res = torch.randn(2, 51, 256, generator=g(20)) * 3, torch.randn(2, 51, 256, generator=g(21))
    x[0, 0], res[0, 0] = 1.25, 0.5                                        # a constant row: variance 0
    gamma, beta = torch.rand(256, generator=g(22)) + 0.5, torch.randn(256, generator=g(23))
    d = lambda t: t.to(DEV)
    want, bound = fp32_bound(lambda a, b, c, e: RR.add_ln(a, b, c, e), x, res, gamma, beta)
    got = ops.add_layernorm(d(x), d(res), d(gamma), d(beta))
    close(got, want, bound, 'add + LayerNorm')
    close(got[0, 0], beta.double(), 1e-6, 'constant row')
    want, bound = fp32_bound(lambda a, c, e: RR.add_ln(a, None, c, e), x, gamma, beta)
    close(ops.add_layernorm(d(x), None, d(gamma), d(beta)), want, bound, 'LayerNorm without a residual')
    # the masked form: invalid tokens read `fill`
    _, valid = RR.anchors(DEFORM_SHAPES, torch.float32)
    assert 0 < int((~valid).sum()) < 51
    fill = torch.randn(256, generator=g(24))
    want, bound = fp32_bound(lambda a, c, e, f: RR.add_ln(a, None, c, e, valid=valid, fill=f), x, gamma, beta, fill)
    close(ops.add_layernorm(d(x), None, d(gamma), d(beta), fill=d(fill), shapes=DEFORM_SHAPES), want, bound, 'masked LayerNorm')


def topk_scores(L, k, seed):
    s = torch.randn(2, L, generator=g(seed))
    for b in range(2):
        order = torch.argsort(s[b], descending=True)
        s[b, order[2:7]] = float(s[b, order[2]])                                 # a tied group inside the selection
        if L - k >= 12:
            s[b, order[L - 6:L - 1]] = float(s[b, order[L - 6]])                 # one outside
        if L > k:
            lo, hi = max(k - 3, 8), min(k + 3, L)
            s[b, order[lo:hi]] = float(s[b, order[lo]])                          # one straddling the cut
    return s


@gpu
@pytest.mark.parametrize('L', [300, 301, 504, 8400])
@pytest.mark.parametrize('k', [300, 100])
def test_topk(L, k):
    from mgdt_yolo_amd import ops
    s = topk_scores(L, k, L + k)
    want = RR.stable_topk(s, k)
    got = ops.rtdetr_topk(s.to(DEV), k).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, want)
    if L > k:                                                             # the lowest indices of the straddling group win
        for b in range(2):
            cut = s[b, want[b, -1]]
            tied = torch.nonzero(s[b] == cut).flatten()
            assert len(tied) > 1 and set(tied.tolist()) - set(want[b].tolist())
            assert set(tied[:int((s[b, want[b]] == cut).sum())].tolist()) <= set(got[b].tolist())


@gpu
def test_topk_refuses_k_above_L():
    from mgdt_yolo_amd import ops
    with pytest.raises(RuntimeError, match='out of range'):
        ops.rtdetr_topk(torch.zeros(1, 99, device=DEV), 100)


@gpu
def test_refine_and_ref_init():
    from mgdt_yolo_amd import ops
    delta = torch.randn(2, 40, 4, generator=g(30))
    ref = torch.rand(2, 40, 4, generator=g(31))
    ref[0, 0] = torch.tensor([0.0, 1.0, float(torch.sigmoid(torch.tensor(float('inf')))), float(torch.sigmoid(torch.tensor(float('-inf'))))])
    want, bound = fp32_bound(RR.refine, delta, ref)
    close(ops.rtdetr_refine(delta.to(DEV), ref.to(DEV)), want, bound, 'refine')
    wide = torch.randn(2, 40, 8, generator=g(32))                         # delta as the first columns of a padded matrix
    wide[..., :4] = delta
    close(ops.rtdetr_refine(wide.to(DEV)[..., :4], ref.to(DEV)), want, bound, 'refine, strided delta')
    L = sum(h * w for h, w in DEFORM_SHAPES)
    idx = torch.stack([torch.randperm(L, generator=g(33))[:40], torch.arange(L - 40, L)])
    anc, valid = RR.anchors(DEFORM_SHAPES, torch.float64)
    assert bool((~valid[idx]).any()) and bool(valid[idx].any())
    want = torch.sigmoid(delta.double() + anc[idx])
    anc32, _ = RR.anchors(DEFORM_SHAPES, torch.float32)
    bound = max(1e-6, 8 * float((torch.sigmoid(delta + anc32[idx]).double() - want).abs().max()))
    got = ops.rtdetr_ref_init(delta.to(DEV), idx.to(DEV), DEFORM_SHAPES)
    close(got, want, bound, 'ref_init')
    assert bool((got.cpu()[~valid[idx]] == 1.0).all())


@gpu
@pytest.mark.parametrize('nc', [80, 3])
def test_rowmax_gather_sigmoid(nc):
    from mgdt_yolo_amd import ops
    L, nq = 51, 20
    feat, logits = torch.randn(2, L, 256, generator=g(40)), torch.randn(2, L, nc, generator=g(41))
    idx = torch.stack([torch.randperm(L, generator=g(42))[:nq], torch.randperm(L, generator=g(43))[:nq]])
    assert torch.equal(ops.rtdetr_rowmax(logits.to(DEV)).cpu(), logits.max(-1).values)
    embed, enc = ops.rtdetr_gather(feat.to(DEV), logits.to(DEV), idx.to(DEV))
    bi = torch.arange(2)[:, None]
    assert torch.equal(embed.cpu(), feat[bi, idx]) and torch.equal(enc.cpu(), logits[bi, idx])
    want, bound = fp32_bound(torch.sigmoid, logits)
    close(ops.rtdetr_sigmoid(logits.to(DEV)), want, bound, 'sigmoid')


@gpu
def test_post():
    from mgdt_yolo_amd import ops
    B, nq, nc = 3, 300, 7
    boxes, scores = torch.rand(B, nq, 4, generator=g(50)), torch.rand(B, nq, nc, generator=g(51))
    wh = torch.tensor([[640., 480.], [33., 517.], [1., 1.]])
    for conf, classes, scale in ((0.8, None, None), (0.8, None, wh), (0.5, [1, 4], wh), (2.0, None, wh), (0.0, None, None)):
        want = RR.post(boxes.double(), scores.double(), conf, classes, None if scale is None else scale.tolist())
        keep = None
        if classes is not None:
            keep = torch.zeros(nc, dtype=torch.uint8)
            keep[classes] = 1
            keep = keep.to(DEV)
        rows, counts = ops.rtdetr_post(boxes.to(DEV), scores.to(DEV), conf, keep, None if scale is None else scale.to(DEV))
        rows, counts = rows.cpu(), counts.cpu()
        assert counts.dtype == torch.int32 and counts.tolist() == [len(w) for w in want]
        for i, w in enumerate(want):
            n = len(w)
            assert float((rows[i, :n, :4].double() - w[:, :4]).abs().max() if n else 0.0) <= 1e-4
            assert torch.equal(rows[i, :n, 5].double(), w[:, 5]) and torch.equal(rows[i, :n, 4].double(), w[:, 4])
            assert float(rows[i, n:].abs().max() if n < nq else 0.0) == 0.0
        if conf == 2.0:
            assert counts.tolist() == [0, 0, 0]
        if conf == 0.0:
            assert counts.tolist() == [nq] * B


# ================================================================================================================ GPU: model
_MODELS = {}


def gpu_model(tag):
    key = 'A' if tag == 'B' else tag                                     # cases A and B share a model
    if key not in _MODELS:
        _MODELS[key] = build_model(key, DEV)
    return _MODELS[key]


def case_input(tag):
    b, h, w = RR.CASES[tag][2]
    return seeded_images(b, h, w, seed=RR.IMG_SEED).to(DEV)


@gpu
@pytest.mark.parametrize('tag', list(RR.CASES))
def test_model_fp32_free_running(fx, tag):
    """The test that fails without the feature: image -> selection and outputs of the reference."""
    m, x = gpu_model(tag), case_input(tag)
    _, _, (b, h, w) = RR.CASES[tag]
    d64 = dict(zip(('box', 'conf', 'enc_box', 'enc_score', 'score_max'), fx[f'{tag}_d64'].tolist()))
    with torch.no_grad():
        index, score_max = m.select_queries(x)
        dec_b, dec_s, enc_b, enc_s, meta = m(x)
    assert meta is None and dec_b.dtype == dec_s.dtype == enc_b.dtype == enc_s.dtype == torch.float32
    nq = RR.case_nq_ndl(tag)[0]
    assert tuple(dec_b.shape) == (1, b, nq, 4) and tuple(dec_s.shape) == (1, b, nq, RR.CASES[tag][1]) and tuple(enc_b.shape) == (b, nq, 4)
    close(score_max, torch.from_numpy(fx[f'{tag}_score_max']).double(), max(1e-5, 8 * d64['score_max']), f'{tag} score_max')
    idx = index.cpu()
    assert idx.dtype == torch.int64 and torch.equal(idx, torch.from_numpy(fx[f'{tag}_index'])), 'the selection after the tie rule'
    assert torch.equal(idx, RR.stable_topk(score_max, nq))
    _, valid = RR.anchors(RR.level_shapes(h, w), torch.float32)
    tied = set(torch.nonzero(~valid).flatten().tolist())
    for i in range(b):
        sel, ref_sel = set(idx[i].tolist()), set(fx[f'{tag}_topk_ref'][i].tolist())
        if tied & sel and not tied <= sel:                                # the cut falls inside the tied group (case C): the untied part is the reference's
            assert sel - tied == ref_sel - tied and len(sel & tied) == len(ref_sel & tied)
        else:
            assert sel == ref_sel
    px = torch.tensor([w, h, w, h], dtype=torch.float64)
    close(dec_b[0].cpu().double() * px, torch.from_numpy(fx[f'{tag}_dec_bboxes']).double() * px, max(1e-3, 8 * d64['box']), f'{tag} boxes (px)')
    close(dec_s[0], torch.from_numpy(fx[f'{tag}_dec_scores']).double(), max(1e-4, 8 * d64['conf']), f'{tag} confidences')
    close(enc_b.cpu().double() * px, torch.from_numpy(fx[f'{tag}_enc_bboxes']).double() * px, max(1e-3, 8 * d64['enc_box']), f'{tag} enc boxes (px)')
    close(enc_s, torch.from_numpy(fx[f'{tag}_enc_scores']).double(), max(1e-4, 8 * d64['enc_score']), f'{tag} enc scores')
    if tag == 'B':                                                        # every invalid token is selected: reference box 1, identical rows
        inv = torch.isin(idx, torch.tensor(sorted(tied)))
        assert int(inv.sum()) == b * len(tied) and bool((enc_b.cpu()[inv] == 1.0).all())
    # a forced index in another order gives the same rows in that order
    perm = torch.flip(index, dims=[1])
    with torch.no_grad():
        fb, fs = m(x, query_index=perm)[:2]
    close(torch.flip(fb[0], dims=[1]), dec_b[0].cpu().double(), 1e-5, f'{tag} forced index: boxes')
    close(torch.flip(fs[0], dims=[1]), dec_s[0].cpu().double(), 1e-5, f'{tag} forced index: confidences')


_MODELS16 = {}


def gpu_model_bf16():
    if 'A' not in _MODELS16:
        _MODELS16['A'] = build_model('A', DEV).set_compute_dtype(torch.bfloat16)
    return _MODELS16['A']


@gpu
@pytest.mark.parametrize('tag', list(RR.BF16))
def test_model_bf16(fx, tag):
    """bf16 token memory and values: with the recorded indices forced every quantity is within 3 x the emulation's recorded difference of the fp32
    reference; free-running, the selection is the stable sort of the model's own score_max, which is within 3 x the emulation's."""
    m, x = gpu_model_bf16(), case_input(tag).to(torch.bfloat16)
    _, _, (b, h, w) = RR.CASES[tag]
    db = dict(zip(('box', 'conf', 'enc_box', 'enc_score', 'score_max'), fx[f'{tag}_dbf16'].tolist()))
    idx = torch.from_numpy(fx[f'{tag}_index']).to(DEV)
    with torch.no_grad():
        dec_b, dec_s, enc_b, enc_s, _ = m(x, query_index=idx)
        index, score_max = m.select_queries(x)
    assert dec_b.dtype == dec_s.dtype == enc_b.dtype == enc_s.dtype == score_max.dtype == torch.float32
    px = torch.tensor([w, h, w, h], dtype=torch.float64)
    close(dec_b[0].cpu().double() * px, torch.from_numpy(fx[f'{tag}_dec_bboxes']).double() * px, 3 * db['box'], f'{tag} bf16 boxes (px)')
    close(dec_s[0], torch.from_numpy(fx[f'{tag}_dec_scores']).double(), 3 * db['conf'], f'{tag} bf16 confidences')
    close(enc_b.cpu().double() * px, torch.from_numpy(fx[f'{tag}_enc_bboxes']).double() * px, 3 * db['enc_box'], f'{tag} bf16 enc boxes (px)')
    close(enc_s, torch.from_numpy(fx[f'{tag}_enc_scores']).double(), 3 * db['enc_score'], f'{tag} bf16 enc scores')
    close(score_max, torch.from_numpy(fx[f'{tag}_score_max']).double(), 3 * db['score_max'], f'{tag} bf16 score_max')
    assert torch.equal(index.cpu(), RR.stable_topk(score_max, RR.case_nq_ndl(tag)[0]))


@gpu
def test_quantize_fp8_leaves_the_head_on_bf16():
    import copy
    m = copy.deepcopy(gpu_model_bf16())
    x = case_input('A').to(torch.bfloat16)
    table = m.quantize_fp8(x)
    n = len(m.model) - 1
    assert table and not any(k.startswith(f'model.{n}') for k in table)
    with torch.no_grad():
        out = m(x)
    assert out[0].dtype == torch.float32 and bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_model_capture_batch_and_fuse(dtype):
    """Model plus head capture into one graph and replay bit-equal to eager; a batch of 2 equals its images run alone; fuse() changes no bit."""
    m = gpu_model('A') if dtype == torch.float32 else gpu_model_bf16()
    xs = [seeded_images(2, 160, 160, seed=s).to(DEV).to(dtype) for s in (RR.IMG_SEED, RR.IMG_SEED + 1)]
    flat = lambda out: [t for t in out if t is not None]
    with torch.no_grad():
        ref = [[t.clone() for t in flat(m(x))] for x in xs]
    xin = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        m(xin)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = flat(m(xin))
    for x, r in zip(xs[::-1], ref[::-1]):
        xin.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, r):
            assert torch.equal(a, b), float((a - b).abs().max())
    with torch.no_grad():
        for i in range(2):
            one = flat(m(xs[0][i:i + 1]))
            for a, b, bdim in zip(one, ref[0], (1, 1, 0, 0)):
                assert torch.equal(a.select(bdim, 0), b.select(bdim, i)), (i, float((a.select(bdim, 0) - b.select(bdim, i)).abs().max()))
        import copy
        fused = flat(copy.deepcopy(m).fuse()(xs[0]))
    for a, b in zip(fused, ref[0]):
        assert torch.equal(a, b), float((a - b).abs().max())


@gpu
def test_large_token_matrices_go_in_batch_chunks():
    """A token matrix beyond the convolution's 2 GiB view limit is handed over in batch chunks: forced here at a small size, bit-equal to one call."""
    m, x = gpu_model('A'), case_input('A')
    head = m.model[-1]
    with torch.no_grad():
        want = m(x)[:4]
        head.VIEW_BYTES = 525 * 1536 * 4                                 # one image of the widest matrix (the values) per call
        try:
            got = m(x)[:4]
        finally:
            del head.VIEW_BYTES
    assert head.VIEW_BYTES == (1 << 31) - 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@gpu
def test_predictor(fx):
    from mgdt_yolo_amd.vit.rtdetr.predict import RTDETRPredictor
    conf = float(fx['A_pred_conf'])
    import copy
    p = RTDETRPredictor(copy.deepcopy(gpu_model('A')), imgsz=160, conf=conf)      # the predictor fuses its model in place
    x = case_input('A')
    rows = p(x)
    for i, r in enumerate(rows):
        want = torch.from_numpy(fx[f'A_pred_rows_{i}'])
        assert tuple(r.shape) == tuple(want.shape), 'the kept queries, in query order'
        r = r.cpu()
        assert torch.equal(r[:, 5], want[:, 5])
        assert float(((r[:, :4] - want[:, :4]).abs() * 160).max()) <= 1e-3 and float((r[:, 4] - want[:, 4]).abs().max()) <= 1e-4
    # a list source: two uint8 images of different original sizes, scaled to each image's own (w, h)
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (120, 200, 3), dtype=np.uint8), rng.integers(0, 256, (90, 70, 3), dtype=np.uint8)]
    got = p(imgs)
    with torch.no_grad():
        pre = p.preprocess(imgs)
        dec_b, dec_s = p.model(pre)[:2]
    want = RR.post(dec_b[0].cpu().double(), dec_s[0].cpu().double(), conf, None, [(200, 120), (70, 90)])
    for r, w_, im in zip(got, want, imgs):
        assert len(r) == len(w_) and len(r) > 0
        assert float((r.cpu()[:, :4].double() - w_[:, :4]).abs().max()) <= 1e-3
        assert float(r[:, 2].max()) <= im.shape[1] * 1.5 and float(r[:, 3].max()) <= im.shape[0] * 1.5
