"""The RT-DETR criterion: mgdt_detr_match_fwd / mgdt_detr_loss_fwd, HungarianMatcher, DETRLoss / RTDETRDetectionLoss, predict_layers and
loss_from_preds against the float64 restatements of tests/rtdetr_loss_ref.py and the reference's recorded outputs (tests/golden/rtdetr_loss_NN.npz,
written by tests/golden/gen_rtdetr_loss.py).

Bounds.  Cost matrix: max(1e-6, 8 x |restatement in fp32 on the CPU - float64|), the rule of tests/test_rtdetr.py.  Assignment against the
reference: first 2 * ng * max|C_device - C_float64| < the image's recorded gap (second-best minus best assignment cost) - under that condition
rounding cannot change the optimum - then equality.  Solver alone: equality with scipy on the kernel's own cost, no tolerance.  Losses and
gradients: max(8 x the recorded fp32-vs-fp64 difference of that quantity, 1e-6 x max|float64 value|).  Case a's d_logits are recorded for the last
layer only (the whole float64 tensor is 2.7 MB): the CPU part pins the restatement on the records (1e-9), the GPU part compares the device with
the restatement's float64 run, which covers every layer."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import rtdetr_loss_ref as LR
import rtdetr_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
DEV = 'cuda:0'
gpu = pytest.mark.gpu
NEW = ('mgdt_detr_match_workspace_bytes', 'mgdt_detr_match_fwd', 'mgdt_detr_loss_workspace_bytes', 'mgdt_detr_loss_fwd', 'mgdt_rtdetr_val_post_fwd')
TAGS = tuple(LR.CASES)


@pytest.fixture(scope='module')
def fx():
    return LR.load_fixtures(GOLDEN)


_TRUTH = {}


def truth(tag, fx=None):
    """the float64 restatement of a case with the recorded assignment forced (computed once, shared, never modified)"""
    if tag not in _TRUTH:
        _TRUTH[tag] = LR.criterion(tag, torch.float64, assign=None if fx is None else fx[f'{tag}_match'].astype(np.int64))
    return _TRUTH[tag]


def off_of(groups):
    return np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)


# ================================================================================================================ CPU
@pytest.mark.parametrize('tag', TAGS)
def test_restatements_reproduce_the_fixtures(fx, tag):
    """inputs by checksum; the assignment of scipy on the float64 cost equals the reference's match_indices; losses and gradients within 1e-9"""
    inp = LR.make_inputs(tag)
    for k in ('boxes', 'logits', 'gt_boxes', 'gt_cls'):
        assert LR.checksum(inp[k]) == float(fx[f'{tag}_sum_{k}']), k
    r = LR.criterion(tag, torch.float64)
    assert np.array_equal(r['used'], fx[f'{tag}_match'])          # with use_uni_match: every auxiliary layer on auxiliary layer uni_match_ind's
    assert (fx[f'{tag}_gap'] >= LR.GAP_MIN).all()
    keys = [str(k) for k in fx[f'{tag}_keys']]
    assert sorted(r['losses']) == keys
    for k, want in zip(keys, fx[f'{tag}_loss64']):
        assert abs(r['losses'][k] - want) <= 1e-9 * max(1.0, abs(want)), (k, r['losses'][k], want)
    names = ['d_boxes', 'd_logits'] + (['dn_d_boxes', 'dn_d_logits'] if 'dn' in LR.CASES[tag] else [])
    for n in names:
        want = fx[f'{tag}_{n}64']
        got = r[n].numpy()
        got = got[-want.shape[0]:]
        assert np.abs(got - want).max() <= 1e-9, n
        assert abs(float(np.abs(r[n].numpy()).max()) - float(fx[f'{tag}_{n}_absmax'])) <= 1e-9, n


def test_gap_restatement_rejects_a_near_tie():
    """the gap is what the generator's condition rests on: a block with two optima has gap 0, and a clear one its margin"""
    c = np.array([[1.0, 2.0], [2.0, 3.0], [5.0, 5.0]])
    assert LR.gap_of(c) == 0.0
    c[0, 0] = 0.5
    assert abs(LR.gap_of(c) - 0.5) < 1e-12


def test_dn_match_indices_and_signatures():
    from mgdt_yolo_amd.vit.utils import DETRLoss, HungarianMatcher, RTDETRDetectionLoss, loss_and_head_grads  # noqa: F401
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(HungarianMatcher.__init__)[1:] == ['cost_gain', 'use_fl', 'with_mask', 'num_sample_points', 'alpha', 'gamma']
    assert sig(HungarianMatcher.forward)[1:6] == ['pred_bboxes', 'pred_scores', 'gt_bboxes', 'gt_cls', 'gt_groups']
    assert sig(DETRLoss.__init__)[1:] == ['nc', 'loss_gain', 'aux_loss', 'use_fl', 'use_vfl', 'use_uni_match', 'uni_match_ind']
    assert sig(RTDETRDetectionLoss.forward)[1:] == ['preds', 'batch', 'dn_bboxes', 'dn_scores', 'dn_meta']
    d = inspect.signature(DETRLoss.__init__).parameters
    assert (d['nc'].default, d['aux_loss'].default, d['use_fl'].default, d['use_vfl'].default, d['use_uni_match'].default, d['uni_match_ind'].default) == (80, True, True, False, False, 0)
    crit = RTDETRDetectionLoss(nc=3, use_vfl=True)
    assert crit.matcher.cost_gain == {'class': 2, 'bbox': 5, 'giou': 2} and crit.loss_gain['bbox'] == 5 and crit.matcher.alpha == 0.25 and crit.matcher.gamma == 2.0
    inp = LR.make_inputs('g')
    groups = LR.CASES['g']['groups']
    mi = RTDETRDetectionLoss.get_dn_match_indices([torch.from_numpy(p) for p in inp['dn_pos_idx']], inp['dn_num_group'], list(groups))
    want, _ = LR.dn_assign(inp['dn_pos_idx'], inp['dn_num_group'], groups, inp['dn_num_split'][0])
    assert len(mi) == len(groups) and mi[0][0].numel() == 0 and mi[0][1].dtype == torch.int32
    for i, (q, g) in enumerate(mi):
        assert g.dtype == torch.int32 and np.array_equal(want[i][q.numpy()], g.numpy())


def test_unbuilt_options_raise():
    from mgdt_yolo_amd.vit.utils import DETRLoss, HungarianMatcher, RTDETRDetectionLoss
    with pytest.raises(NotImplementedError, match='use_fl=False'):
        HungarianMatcher(use_fl=False)
    with pytest.raises(NotImplementedError, match='with_mask=True'):
        HungarianMatcher(with_mask=True)
    with pytest.raises(NotImplementedError, match='use_fl=False'):
        DETRLoss(use_fl=False)
    with pytest.raises(NotImplementedError, match='mask'):
        RTDETRDetectionLoss()._get_loss_mask(None, None, None)


def test_new_symbols_are_declared_bound_and_exported():
    from mgdt_yolo_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    lib = _lib.lib()
    for n in NEW:
        assert re.search(r'\b(int|size_t) ' + n + r'\(', hdr) and n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert ops.DETR_GCAP == int(re.search(r'#define MGDT_DETR_GCAP (\d+)', hdr).group(1)) >= 128
    assert ops.DETR_MAX_NQ == int(re.search(r'#define MGDT_DETR_MAX_NQ (\d+)', hdr).group(1))
    assert ops.RTDETR_VAL_MAX_NQ == int(re.search(r'#define MGDT_RTDETR_VAL_MAX_NQ (\d+)', hdr).group(1))
    assert lib.mgdt_detr_match_workspace_bytes(7, 320, 300) == 7 * 320 * 300 * 4 and lib.mgdt_detr_match_workspace_bytes(0, 1, 1) == 0
    assert lib.mgdt_detr_loss_workspace_bytes(7, 32, 300) == 16 + 7 * 32 * 5 * 3 * 8
    mk = open(os.path.join(ROOT, 'mgdt_yolo_amd', 'csrc', 'Makefile')).read()
    assert 'detr_loss.hip' in mk and re.search(r'detr_loss\.o[^\n]*-ffp-contract=off', mk)
    assert not re.search(r'^[^\n#]*detr_loss\.o[^\n]*: NOPK =', mk, re.M), 'the default NOPK flags'
    from mgdt_yolo_amd.vit.rtdetr import RTDETRValidator  # noqa: F401
    from mgdt_yolo_amd.nn.tasks import RTDETRDetectionModel
    from mgdt_yolo_amd.nn.modules.head import RTDETR_TRAIN_MSG, RTDETRDecoder
    assert all(hasattr(RTDETRDetectionModel, n) for n in ('predict_layers', 'detr_criterion', 'loss_from_preds')) and hasattr(RTDETRDecoder, 'forward_layers')
    assert 'training is not built' in RTDETR_TRAIN_MSG and 'denoising' in RTDETR_TRAIN_MSG and 'reverse pass' in RTDETR_TRAIN_MSG


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    """every refusal below happens on the host, before any launch: the device pointers are never dereferenced"""
    from mgdt_yolo_amd import _lib
    lib = _lib.lib()
    BAD_SHAPE, BAD_ARG = -1, -4
    p = C.c_void_p(256)
    host = lambda *v: (C.c_int32 * len(v))(*v)
    big = 1 << 30

    def match(nq=8, off=host(0, 2), ws=big, boxes=p, assign=p, layer_of_match=-1, nc=3, workspace=p):
        return lib.mgdt_detr_match_fwd(boxes, p, nc, 1, 1, nq, nc, p, p, p, off, 2.0, 5.0, 2.0, 0.25, 2.0, layer_of_match, workspace, ws, assign, None, None)
    assert match(nq=4, off=host(0, 5)) == BAD_SHAPE and b'ground truths' in lib.mgdt_last_error()          # ng > nq
    assert match(nq=1024, off=host(0, 257)) == BAD_SHAPE                                                   # ng > g_cap
    assert match(nq=0) == BAD_SHAPE and match(nq=4096) == BAD_SHAPE and match(nc=0) == BAD_SHAPE
    assert match(boxes=None) == BAD_ARG and match(assign=None) == BAD_ARG and match(off=None) == BAD_ARG and match(workspace=None) == BAD_ARG
    assert match(ws=8 * 2 * 4 - 1) == BAD_ARG and b'workspace' in lib.mgdt_last_error()
    assert match(off=host(0, -1)) == BAD_ARG and match(off=host(1, 2)) == BAD_ARG and match(layer_of_match=1) == BAD_ARG

    def loss(nq=8, ws=big, out=p, d_boxes=p, d_logits=p, num_pairs=2, G=2, gts=p):
        return lib.mgdt_detr_loss_fwd(p, p, 3, 1, 1, nq, 3, gts, gts, G, p, num_pairs, 1.0, 5.0, 2.0, 1, 1.0, p, ws, out, p, d_boxes, d_logits, None)
    assert loss(nq=0) == BAD_SHAPE and loss(out=None) == BAD_ARG and loss(d_logits=None) == BAD_ARG and loss(num_pairs=-1) == BAD_ARG and loss(gts=None) == BAD_ARG
    assert loss(ws=16 + 3 * 8 - 1) == BAD_ARG and b'workspace' in lib.mgdt_last_error()
    post = lambda nq=8, rows=p: lib.mgdt_rtdetr_val_post_fwd(p, p, 1, nq, 3, None, rows, p, None)
    assert post(nq=0) == BAD_SHAPE and post(nq=4097) == BAD_SHAPE and post(rows=None) == BAD_ARG


# ================================================================================================================ GPU
def dev_inputs(tag):
    inp = LR.make_inputs(tag)
    t = lambda k: torch.from_numpy(inp[k]).float().to(DEV)
    return inp, t('boxes'), t('logits'), t('gt_boxes'), torch.from_numpy(inp['gt_cls']).to(DEV)


def run_match(tag, layer_of_match=-1):
    from mgdt_yolo_amd.vit.utils import HungarianMatcher
    _, boxes, logits, gb, gc = dev_inputs(tag)
    m = HungarianMatcher(cost_gain={'class': 2, 'bbox': 5, 'giou': 2})
    assign, cost = m.assign(boxes, logits, gb, gc, list(LR.CASES[tag]['groups']), layer_of_match=layer_of_match, want_cost=True)
    torch.cuda.synchronize()
    return assign.cpu().numpy(), cost.cpu().numpy()


def own_columns(cost, groups):
    """the exported (l, B, nq, g_cap) cost -> list over images of (l, nq, ng)"""
    return [cost[:, b, :, :n] for b, n in enumerate(groups)]


@gpu
@pytest.mark.parametrize('tag', ('a', 'b', 'd'))
def test_cost_matrix(tag):
    groups = LR.CASES[tag]['groups']
    inp = LR.make_inputs(tag)
    off = off_of(groups)
    _, cost = run_match(tag)
    t = lambda k, dt: torch.from_numpy(inp[k]).to(dt)
    c64 = LR.cost_matrix(t('boxes', torch.float64), t('logits', torch.float64), t('gt_boxes', torch.float64), torch.from_numpy(inp['gt_cls'])).numpy()
    c32 = LR.cost_matrix(t('boxes', torch.float32), t('logits', torch.float32), t('gt_boxes', torch.float32), torch.from_numpy(inp['gt_cls'])).double().numpy()
    bound = max(1e-6, 8 * float(np.abs(c32 - c64).max()))
    for b, blk in enumerate(own_columns(cost, groups)):
        if groups[b]:
            d = float(np.abs(blk.astype(np.float64) - c64[:, b, :, off[b]:off[b + 1]]).max())
            print(f'{tag} image {b}: cost max |d| {d:.3e}, bound {bound:.3e}')
            assert d <= bound
        assert not cost[:, b, :, groups[b]:].any(), 'columns past the image\'s ground truths stay untouched'


@gpu
@pytest.mark.parametrize('tag', ('a', 'b', 'd', 'e'))
def test_solver_equals_scipy_on_its_own_cost(tag):
    c = LR.CASES[tag]
    groups, off = c['groups'], off_of(c['groups'])
    k = c['kw'].get('uni_match_ind', 0) if c['kw'].get('use_uni_match') else -1
    assign, cost = run_match(tag, layer_of_match=k)
    for b, blk in enumerate(own_columns(cost, groups)):
        for l in range(c['layers']):
            want = np.full(c['nq'], -1, np.int64)
            if groups[b]:
                i, j = LR.solve(blk[l].astype(np.float64))
                want[i] = j + off[b]
            assert np.array_equal(assign[l, b], want), (tag, l, b)
    if k >= 0:
        assert all(np.array_equal(assign[l], assign[k]) for l in range(c['layers']))


@gpu
def test_solver_with_identical_ground_truths_and_odd_costs():
    """two identical ground-truth boxes of one class: the optimum is not unique, so the total cost equals scipy's and every ground truth has a distinct
    query; a NaN / inf prediction takes the documented large cost, and the launch neither faults nor hangs"""
    from mgdt_yolo_amd import ops
    r = np.random.RandomState(5)
    nq, nc = 70, 4
    boxes = torch.from_numpy(np.concatenate([r.uniform(0.1, 0.9, (1, 1, nq, 2)), r.uniform(0.05, 0.4, (1, 1, nq, 2))], -1)).float()
    logits = torch.from_numpy(r.normal(-2, 1.5, (1, 1, nq, nc))).float()
    gt = torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.5, 0.5, 0.2, 0.2], [0.3, 0.6, 0.1, 0.3]])
    cls = torch.tensor([1, 1, 2], dtype=torch.int32)
    boxes[0, 0, 3] = float('nan')
    logits[0, 0, 5] = float('inf')
    boxes[0, 0, 6, 2] = float('inf')
    assign, cost = ops.detr_match(boxes.to(DEV), logits.to(DEV), gt.to(DEV), cls.to(DEV), [3], want_cost=True)
    a, c = assign.cpu().numpy()[0, 0], cost.cpu().numpy()[0, 0, :, :3].astype(np.float64)
    big = float(np.float32(1e18))
    assert np.isfinite(c).all() and (c[3] == big).all() and (c[6] == big).all()
    q = np.nonzero(a >= 0)[0]
    assert sorted(a[q].tolist()) == [0, 1, 2] and len(set(q.tolist())) == 3
    i, j = LR.solve(c)
    assert c[q, a[q]].sum() == c[i, j].sum()


@gpu
@pytest.mark.parametrize('tag', TAGS)
def test_assignment_equals_the_reference(fx, tag):
    c = LR.CASES[tag]
    groups, off = c['groups'], off_of(c['groups'])
    assign, cost = run_match(tag)
    c64 = truth(tag, fx)['cost'].numpy()
    for b, blk in enumerate(own_columns(cost, groups)):
        if groups[b]:
            for l in range(c['layers']):
                d = float(np.abs(blk[l].astype(np.float64) - c64[l, b, :, off[b]:off[b + 1]]).max())
                gap = float(fx[f'{tag}_gap'][l, b])
                print(f'{tag} layer {l} image {b}: 2 ng max|dC| = {2 * groups[b] * d:.3e}, gap {gap:.3e}')
                assert 2 * groups[b] * d < gap
    # the reference's record: with use_uni_match the last layer on its own costs, every auxiliary layer on auxiliary layer uni_match_ind's
    assert np.array_equal(LR.uni_assign(assign, c['kw']), fx[f'{tag}_match'])


@gpu
def test_matcher_forward_returns_the_reference_form(fx):
    from mgdt_yolo_amd.vit.utils import HungarianMatcher
    _, boxes, logits, gb, gc = dev_inputs('b')
    groups = list(LR.CASES['b']['groups'])
    m = HungarianMatcher(cost_gain={'class': 2, 'bbox': 5, 'giou': 2})
    out = m(boxes[-1], logits[-1], gb, gc, groups)
    want = fx['b_match'][-1]
    assert len(out) == len(groups)
    for b, (q, gidx) in enumerate(out):
        assert q.dtype == torch.int32 and gidx.dtype == torch.int32 and q.device.type == 'cpu' and len(q) == groups[b]
        wq = np.nonzero(want[b] >= 0)[0]
        assert np.array_equal(q.numpy(), wq) and np.array_equal(gidx.numpy(), want[b][wq])
    empty = m(boxes[-1], logits[-1], gb[:0], gc[:0], [0, 0, 0])
    assert all(len(q) == 0 and q.dtype == torch.int32 for q, _ in empty)


def make_crit(tag):
    from mgdt_yolo_amd.vit.utils import RTDETRDetectionLoss
    c = LR.CASES[tag]
    return RTDETRDetectionLoss(nc=c['nc'], **{'use_vfl': True, **c['kw']})


def crit_inputs(tag):
    inp, boxes, logits, gb, gc = dev_inputs(tag)
    batch = {'cls': gc, 'bboxes': gb, 'gt_groups': list(LR.CASES[tag]['groups'])}
    kw = {}
    if 'dn' in LR.CASES[tag]:
        kw = dict(dn_bboxes=torch.from_numpy(inp['dn_boxes']).float().to(DEV), dn_scores=torch.from_numpy(inp['dn_logits']).float().to(DEV),
                  dn_meta={'dn_pos_idx': [torch.from_numpy(p) for p in inp['dn_pos_idx']], 'dn_num_group': inp['dn_num_group'], 'dn_num_split': inp['dn_num_split']})
    return boxes, logits, batch, kw


def check_losses(fx, tag, d, grads, mode):
    keys = [str(k) for k in fx[f'{tag}_keys']]
    assert sorted(d) == keys
    t = truth(tag, fx)
    for k, want, d64 in zip(keys, fx[f'{tag}_loss64'], fx[f'{tag}_loss_d64']):
        assert d[k].dim() == 0 and d[k].device.type == 'cuda'
        bound = max(8 * float(d64), 1e-6 * abs(float(want)))
        got = float(d[k].detach())
        diff = abs(got - float(want))
        print(f'{tag} {mode} {k}: {got:.7f} vs {float(want):.7f}: |d| {diff:.3e}, bound {bound:.3e}')
        assert diff <= bound, (k, diff, bound)
    names = ['d_boxes', 'd_logits'] + (['dn_d_boxes', 'dn_d_logits'] if 'dn' in LR.CASES[tag] else [])
    for n, got, d64 in zip(names, grads, fx[f'{tag}_d64']):
        want = t[n].numpy()
        bound = max(8 * float(d64), 1e-6 * float(np.abs(want).max()))
        diff = float(np.abs(got.detach().cpu().double().numpy() - want).max())
        print(f'{tag} {mode} {n}: max |d| {diff:.3e}, bound {bound:.3e}')
        assert diff <= bound, (n, diff, bound)


@gpu
@pytest.mark.parametrize('mode', ('free', 'forced'))
@pytest.mark.parametrize('tag', TAGS)
def test_losses_and_gradients(fx, tag, mode):
    """every dict entry and the gradients of the summed dict against the float64 records, free-running and with the recorded assignment forced"""
    crit = make_crit(tag)
    boxes, logits, batch, kw = crit_inputs(tag)
    leaves = [boxes.requires_grad_(), logits.requires_grad_()] + ([kw['dn_bboxes'].requires_grad_(), kw['dn_scores'].requires_grad_()] if kw else [])
    if mode == 'forced':
        forced = torch.from_numpy(LR.uni_assign(fx[f'{tag}_match'].astype(np.int64), LR.CASES[tag]['kw'])).to(torch.int32).to(DEV)
        crit._assign = lambda *a, **k: forced
    d = crit((boxes, logits), batch, **kw)
    sum(d.values()).backward()
    grads = [x.grad if x.grad is not None else torch.zeros_like(x) for x in leaves]
    check_losses(fx, tag, d, grads, mode)
    used = LR.uni_assign(fx[f'{tag}_match'].astype(np.int64), LR.CASES[tag]['kw'])
    assert not grads[0].cpu().numpy()[used < 0].any(), 'the box gradient of an unmatched query is exactly 0'


@gpu
def test_autograd_explicit_repeat_and_graph(fx):
    """backward through the autograd Function == loss_and_head_grads bit for bit; two runs bit-equal; a captured graph (one stream, no parallel branch)
    equals eager bit for bit; and the criterion is two launches"""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.vit.utils import loss_and_head_grads
    tag = 'a'
    crit = make_crit(tag)
    boxes, logits, batch, _ = crit_inputs(tag)
    batch['cls'] = batch['cls'].to(torch.int32)
    batch['gt_off'] = torch.from_numpy(off_of(batch['gt_groups']).astype(np.int32)).to(DEV)
    b1, l1 = boxes.clone().requires_grad_(), logits.clone().requires_grad_()
    d = crit((b1, l1), batch)
    sum(d.values()).backward()
    d2, gb2, gl2 = loss_and_head_grads(crit, (boxes, logits), batch)
    d3, gb3, gl3 = loss_and_head_grads(crit, (boxes, logits), batch)
    for k in d:
        assert torch.equal(d[k], d2[k]) and torch.equal(d2[k], d3[k]), k
    assert torch.equal(b1.grad, gb2) and torch.equal(l1.grad, gl2) and torch.equal(gb2, gb3) and torch.equal(gl2, gl3)
    _, gbs, gls = loss_and_head_grads(crit, (boxes, logits), batch, gscale=0.5)
    assert torch.equal(gbs, gb2 * 0.5) and torch.equal(gls, gl2 * 0.5), 'gscale is a power of two here: exact'
    with ops.profile() as prof:
        loss_and_head_grads(crit, (boxes, logits), batch)
    names = [p[0] for p in prof.rows]
    assert names == ['detr_match_fwd', 'detr_loss_fwd'], names
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            dg, gbg, glg = loss_and_head_grads(crit, (boxes, logits), batch)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for k in d2:
        assert torch.equal(dg[k], d2[k]), k
    assert torch.equal(gbg, gb2) and torch.equal(glg, gl2)


def build_model(tag, device):
    from mgdt_yolo_amd.nn.tasks import RTDETRDetectionModel
    from mgdt_yolo_amd.seeding import seed_state_dict_
    m = RTDETRDetectionModel(RR.case_cfg(tag), nc=RR.CASES[tag][1], verbose=False)
    return seed_state_dict_(m, RR.WEIGHT_SEED).eval().to(device)


@gpu
def test_predict_layers_and_loss_from_preds(fx):
    """case D with the recorded query index forced: every layer within the model bounds of tests/test_rtdetr.py (1e-3 px / 1e-4, or 8 x the recorded
    fp32-vs-fp64 difference where larger); the last layer equals the eval forward bit for bit; loss_from_preds on the RECORDED predictions equals the
    reference's (sum, items) within the loss bound"""
    from mgdt_yolo_amd.seeding import seeded_images
    rfx = RR.load_fixtures(GOLDEN)
    tag = 'D'
    _, nc, (b, h, w) = RR.CASES[tag]
    m = build_model(tag, DEV)
    x = seeded_images(b, h, w, seed=RR.IMG_SEED).to(DEV)
    idx = torch.from_numpy(rfx['D_index']).to(DEV)
    with torch.no_grad():
        dec_b, dec_s, enc_b, enc_s, meta = m.predict_layers(x, query_index=idx)
        ev = m.predict(x, query_index=idx)
    nq, ndl = RR.case_nq_ndl(tag)
    assert meta is None and tuple(dec_b.shape) == (ndl, b, nq, 4) and tuple(dec_s.shape) == (ndl, b, nq, nc)
    assert torch.equal(dec_b[-1], ev[0][0]) and torch.equal(torch.sigmoid(dec_s[-1]), ev[1][0]) and torch.equal(enc_b, ev[2]) and torch.equal(enc_s, ev[3])
    px = torch.tensor([w, h, w, h], dtype=torch.float64)
    d64 = fx['h_d64']
    for name, got, scale, floor, dd in (('dec_bboxes', dec_b, px, 1e-3, d64[0]), ('dec_scores', dec_s, 1.0, 1e-4, d64[1]), ('enc_bboxes', enc_b, px, 1e-3, d64[0]),
                                        ('enc_scores', enc_s, 1.0, 1e-4, d64[1])):
        diff = float(((got.cpu().double() - torch.from_numpy(fx[f'h_{name}']).double()) * scale).abs().max())
        bound = max(floor, 8 * float(dd))
        print(f'h {name}: max |d| {diff:.3e}, bound {bound:.3e}')
        assert diff <= bound
    preds = tuple(torch.from_numpy(fx[f'h_{k}']).to(DEV) for k in ('dec_bboxes', 'dec_scores', 'enc_bboxes', 'enc_scores')) + (None,)
    lab = torch.from_numpy(fx['h_labels'])
    batch = dict(img=x, batch_idx=torch.zeros(len(lab)), cls=lab[:, :1], bboxes=lab[:, 1:])
    total, items = m.loss_from_preds(batch, preds)
    got = np.array([float(total)] + items.cpu().tolist())
    want, d = fx['h_loss64'], np.abs(fx['h_loss32'] - fx['h_loss64'])
    for i, name in enumerate(('sum', 'loss_giou', 'loss_class', 'loss_bbox')):
        bound = max(8 * float(d[i]), 1e-6 * abs(float(want[i])))
        print(f'h {name}: {got[i]:.7f} vs {want[i]:.7f}, bound {bound:.3e}')
        assert abs(got[i] - want[i]) <= bound
    assert items.device.type == 'cuda' and tuple(items.shape) == (3,)


@gpu
def test_training_is_still_not_built():
    """next to the new entry points: the criterion exists, a training forward and the reverse pass do not"""
    m = build_model('D', DEV)
    x = torch.zeros(1, 3, 96, 96, device=DEV)
    assert type(m.detr_criterion()).__name__ == 'RTDETRDetectionLoss' and m.detr_criterion().nc == 3 and m.detr_criterion().use_vfl
    for call in (m.init_criterion, lambda: m.loss({'img': x}), lambda: m({'img': x})):
        with pytest.raises(NotImplementedError, match='training is not built'):
            call()
    m.train()
    for call in (lambda: m.predict(x), lambda: m.predict_layers(x), lambda: m.model[-1].forward_layers([x, x, x])):
        with pytest.raises(NotImplementedError, match='training is not built'):
            call()
