"""The detection loss, the task-aligned assigner (loss.hip) and the optimizer kernels (optim.hip) against float64, per route.  GPU cases need a real
MI355X (-m gpu); the checks of the reference itself (it reproduces the committed fixture, the decision margins of every case, the census of
decision edges) run on the host.

Yardstick of the loss: oracle.loss.detection_loss evaluated in float64 on the maps the kernel reads (rounded to the kernel's dtype first), the
dense fp32 targets upcast as they are, the gradient by torch.autograd.  No rounding of the kernel is restated: its arithmetic is fp32 whatever the
map dtype, and the gradient it stores is rounded once.  Yardstick of the optimizer: the same recurrence in float64 torch on the CPU, the scalars as
the C ABI receives them (fp32).

Bounds are kernel_ref._close / _exact, unchanged: fp32 outputs relative L2 <= 2e-5 and every element within 1e-4 * max|ref|; bf16 outputs every
element within 2^-8 * |ref| + 1e-3 * max|ref|; fg and target_gt_idx bit-exact.  tscore, the loss items and every optimizer buffer are fp32 in both
map dtypes and take the fp32 bound.

The assigner takes decisions (top-10 per GT, multi-claim resolution, the clamp of the CIoU at 0, min / max inside the CIoU).  A float64 and an fp32
evaluation agree on all of them when the INPUTS keep a margin, asserted on the reference alone for every case (kernel_ref.loss_margins):
(a) 10th vs 11th largest align metric of a GT >= 1e-4 relative, or both exactly 0 (index order decides, identically); (b) best vs second-best align
over the GTs at a multiply claimed anchor >= 1e-4 relative, or exactly equal because the GT rows are identical (the lower row wins on both sides);
(c) no in-box member of a top-k has a raw CIoU within 1e-5 of 0; (d) no predicted box coordinate equals its target's (autograd splits a min / max
tie, the kernel gives it to one side); (e) no positive align metric of a top-k is below 1e-30 (it would leave the fp32 normal range and could tie
with the exact zeros).  fp32 evaluates s^alpha * ov^8 to a few 1e-6 relative (8 x the error of ov, plus powf), so a 1e-4 gap cannot flip: the
1e-4 is a condition on the inputs, not a tolerance on the kernel.  The salts of the cases were picked on the CPU so that the conditions hold; no
anchor, GT or case is excluded from any comparison.  In-box decisions need no margin: anchor centres and GT edges are fp32 values, their difference
has the right sign in fp32 and is either 0 or far above the 1e-9 threshold.

Measured on MI355X: the 111 GPU cases pass in 5.8 s (the whole module's wall time; the slowest, the 1000-class grid-stride case, 1.0 s; the 35 host
tests take 4.5 s).  Largest share of the bound used: tscore 0.10, items 0.03, fp32 gradient 0.03, bf16 gradient 0.73 (a correctly rounded bf16 store
alone uses up to 0.5), optimizer buffers 0.012, clip 0.005.  The oracle evaluated in fp32 torch on the CPU takes the same integer decisions as
float64 in every case and uses at most 0.054 of the fp32 bound.
"""
import functools

import numpy as np
import pytest
import torch

import inputs as GI
from kernel_ref import (BF16, DEV, F32, _check, _exact, _gen, _nhwc, _rand, f32r, loss_census, loss_gt_random, loss_maps, loss_margins, loss_reference,
                        ref_clip, ref_ema, ref_sgd)
from optim_ref import ref_adam, ref_rmsprop

gpu = pytest.mark.gpu
DTS = [pytest.param(F32, id='f32'), pytest.param(BF16, id='bf16')]
DTN = {F32: 'f32', BF16: 'bf16'}
GAINS = (7.5, 0.5, 1.5)
CALLS = [0, 160, 161, 161 * 40, 161 * 100]      # alpha = 0.5, 0.5, 0.495, 0.3, 0 (s^0 must be 1 at every score)


def _edges_gt():
    """The constructed targets of the 'edges' case (12x12 @ 8: anchor centres at 4, 12, ..., 92 px).  Image 0: rows 0 and 1 identical with edges ON
    anchor centres (12, 60, 52 are centres: those anchors are outside); row 2 overlaps them with another label (multi-claims resolved by
    margin); row 3 lies between four centres (no anchor inside); row 4 holds four centres.  Image 1: no box.  Image 2: two ordinary boxes.
    Image 3: one box of nearly the whole image (DFL targets far beyond reg_max - 1.01)."""
    gt = torch.zeros(4, 5, 5, dtype=F32)
    gt[0] = torch.tensor([[0, 12, 12, 60, 52], [0, 12, 12, 60, 52], [3, 36, 28, 84, 92], [2, 5, 5, 11, 11], [1, 66, 2, 82, 14]], dtype=F32)
    gt[2, :2] = torch.tensor([[1, 10.5, 30.25, 50.75, 70.5], [2, 40.25, 8.5, 90.5, 44.75]], dtype=F32)
    gt[3, 0] = torch.tensor([3, 4.5, 3.5, 90.0, 91.0], dtype=F32)
    return gt


# name -> levels (H, W, stride), B, R, nc, N, boxes per image (None: constructed), box sides px, view (off, extra), dtypes, call counts, salt
CASES = {
    'levels3-scalar': dict(levels=((13, 11, 8), (7, 6, 16), (4, 3, 32)), B=3, R=4, nc=3, N=4, counts=(4, 2, 0), sides=(10, 60), view=(0, 0), dts=(F32, BF16), calls=CALLS, salt=0),
    'a400-vec': dict(levels=((20, 20, 8),), B=3, R=4, nc=4, N=6, counts=(6, 3, 1), sides=(12, 80), view=(0, 0), dts=(F32, BF16), calls=CALLS, salt=0),
    'tood-r16-nc80': dict(levels=((13, 11, 8), (7, 6, 16)), B=2, R=16, nc=80, N=5, counts=(5, 2), sides=(16, 90), view=(0, 0), dts=(F32, BF16), calls=[0], salt=0),
    'slice4-vec': dict(levels=((13, 11, 8),), B=2, R=4, nc=8, N=4, counts=(4, 2), sides=(10, 60), view=(4, 4), dts=(F32, BF16), calls=[0], salt=0),
    'slice1-scalar': dict(levels=((13, 11, 8),), B=2, R=4, nc=8, N=4, counts=(4, 2), sides=(10, 60), view=(1, 2), dts=(F32, BF16), calls=[0], salt=0),
    'nc1': dict(levels=((9, 7, 8),), B=2, R=4, nc=1, N=3, counts=(3, 1), sides=(10, 40), view=(0, 0), dts=(F32,), calls=[0], salt=0),
    'edges': dict(levels=((12, 12, 8),), B=4, R=4, nc=4, N=5, counts=None, sides=None, view=(0, 0), dts=(F32, BF16), calls=[0], salt=0),
    # B * H * W * (1 + nc / 4) = 16 896 * 251 = 4 240 896 items > 16384 * 256: the grid-stride loop of loss_bwd_vec_kernel takes a second trip
    'stride-loop': dict(levels=((66, 64, 8),), B=4, R=4, nc=1000, N=3, counts=(3, 2, 1, 2), sides=(20, 200), view=(0, 0), dts=(BF16,), calls=[0], salt=0),
}
SMALL = [n for n in CASES if n != 'stride-loop']
USES = [(n, dt, cc) for n, c in CASES.items() for dt in c['dts'] for cc in c['calls']]
_id = lambda u: f'{u[0]}-{DTN[u[1]]}-call{u[2]}'


@functools.lru_cache(maxsize=None)
def _inputs(name, dt):
    """(maps: CPU fp64 values representable in dt, one per level; gt (B, N, 5) fp32) of a case.  The targets do not depend on dt."""
    c = CASES[name]
    gen = _gen('loss', name, c['salt'])
    h0, w0, s0 = c['levels'][0]
    gt = _edges_gt() if c['counts'] is None else loss_gt_random(gen, c['B'], c['N'], c['nc'], w0 * s0, h0 * s0, c['counts'], *c['sides'])
    return loss_maps(gen, c['B'], c['R'], c['nc'], c['levels'], dt), gt


@functools.lru_cache(maxsize=None)
def _reference(name, dt, calls):
    """The float64 reference of a case, computed once and shared (nothing in it is modified)."""
    c = CASES[name]
    maps, gt = _inputs(name, dt)
    return loss_reference(maps, gt, [l[2] for l in c['levels']], c['R'], c['nc'], calls)


# ------------------------------------------------------------------------------------------------ host: the reference itself
@pytest.mark.parametrize('seed,calls', GI.LOSS_CASES)
def test_float64_oracle_reproduces_the_fixture(golden, seed, calls):
    """Host: the oracle in float64, fed the fixture's maps upcast and the dense fp32 targets the criterion builds, gives the committed loss.npz
    (the reference's own v8DetectionLoss + autograd) within the tolerances test_oracle_golden.py holds the fp32 oracle to."""
    from oracle import loss as OLoss
    g = golden('loss')
    B, nc, R, hw = (GI.LOSS_SHAPE[k] for k in ('B', 'nc', 'R', 'hw'))
    feats, lab = GI.loss_inputs(seed, B, nc, R, hw)
    scale = torch.tensor([hw[1] * 8.0, hw[0] * 8.0, hw[1] * 8.0, hw[0] * 8.0])
    targets = OLoss.dense_targets(lab['batch_idx'], lab['cls'], lab['bboxes'], B, scale)
    assert targets.dtype == F32
    ref = loss_reference([feats.double()], targets, [8.0], R, nc, calls)
    k = f's{seed}'
    np.testing.assert_allclose(ref['total'].item(), g[k + '_total'], rtol=2e-6)
    np.testing.assert_allclose(ref['items'].numpy(), g[k + '_items'], rtol=2e-6)
    np.testing.assert_allclose(ref['grads'][0].numpy(), g[k + '_grad'], atol=2e-6, rtol=1e-4)
    # and through the batch dictionary, where dense_targets now follows the dtype of the predictions
    _, items, _ = OLoss.detection_loss([feats.double()], lab, [8.0], R, nc, call_count=calls)
    assert items.dtype == torch.float64
    np.testing.assert_allclose(items.numpy(), g[k + '_items'], rtol=2e-6)


@pytest.mark.parametrize('use', USES, ids=_id)
def test_decision_margins_of_every_case(use):
    """Host: conditions (a)-(e) of the module docstring on the float64 reference of every (case, dtype, call count) the GPU tests run."""
    name, dt, calls = use
    loss_margins(_reference(name, dt, calls), _inputs(name, dt)[1], CASES[name]['R'], _id(use))


def test_census_of_decision_edges():
    """Host: over the random and constructed cases the reference contains every decision edge at least once, each asserted by name."""
    total = {}
    for name, dt, calls in USES:
        c = CASES[name]
        for k, v in loss_census(_reference(name, dt, calls), _inputs(name, dt)[1], c['R'], c['nc']).items():
            total[k] = total.get(k, 0) + v
    print(total)
    for k in ('multi_claim_by_margin', 'gt_with_1_to_9_anchors', 'gt_without_anchor', 'padded_gt_row', 'empty_image_in_labelled_batch',
              'dfl_target_clamped', 'positive_label_0', 'positive_label_last', 'centre_on_gt_edge', 'duplicate_rows_tie_to_lower'):
        assert total[k] > 0, (k, total)
    # the constructed case alone holds the edges that random boxes cannot hit
    edges = loss_census(_reference('edges', F32, 0), _inputs('edges', F32)[1], 4, 4)
    for k in ('centre_on_gt_edge', 'duplicate_rows_tie_to_lower', 'gt_without_anchor', 'gt_with_1_to_9_anchors', 'empty_image_in_labelled_batch'):
        assert edges[k] > 0, (k, edges)


def test_alpha_zero_at_the_last_schedule_point():
    """Host: call count 161 * 100 gives alpha = 0, where the align metric is ov^8 whatever the score."""
    ref = _reference('a400-vec', F32, 161 * 100)
    aux = ref['aux']
    assert torch.equal(aux['align'], aux['overlaps'].pow(8.0)) and ref['fg'].any()


def test_out_of_range_labels_are_refused_on_the_host():
    """Host: v8DetectionLoss.preprocess refuses a label outside [0, nc) before anything reaches the device (tal_metrics_kernel indexes the class
    map with the label as it is); labels 0 and nc - 1 pass."""
    import types
    from mgdt_yolo_amd.yolo.utils.loss import v8DetectionLoss
    head = types.SimpleNamespace(nc=4, reg_max=4, no=20, stride=torch.tensor([8.0]))
    crit = v8DetectionLoss(types.SimpleNamespace(model=[head], args=None, parameters=lambda: iter([torch.zeros(1)])))
    batch = lambda labels: {'batch_idx': torch.zeros(len(labels)), 'cls': torch.tensor(labels).view(-1, 1), 'bboxes': torch.full((len(labels), 4), 0.5)}
    assert crit.preprocess(batch([0.0, 3.0]), 1, (64, 64)).shape == (1, 2, 5)
    for bad in ([4.0], [-1.0], [0.0, float('nan')]):
        with pytest.raises(ValueError):
            crit.preprocess(batch(bad), 1, (64, 64))


# ------------------------------------------------------------------------------------------------ GPU: loss and assigner
def _to_device(name, dt):
    """Device views of a case's maps (channel slices of wider buffers filled with random values where the case says so) and the untouched CPU copy
    of every whole buffer."""
    c = CASES[name]
    off, extra = c['view']
    gen = _gen('loss-buffers', name)
    views, bufs = [], []
    for m in _inputs(name, dt)[0]:
        v, big = _nhwc(m, dt, off, extra, gen)
        views.append(v)
        bufs.append((big, big.cpu().clone()))
    return views, bufs


def _check_forward(st, ref, what):
    _exact(st.fg, ref['fg'], what + ' fg')
    _exact(st.gt_idx, ref['gt_idx'], what + ' gt_idx')
    _check(st.tscore, ref['tscore'], F32, what + ' tscore')
    _check(st.out5[1:4], ref['items'], F32, what + ' items')
    _check(st.out5[0:1], ref['total'].reshape(1), F32, what + ' total*B')
    _check(st.out5[4:5], ref['tss'].reshape(1), F32, what + ' max(sum tscore, 1)')


def _check_backward(grads, ref, c, dt, gscale, what):
    a0 = 0
    for l, (g, (h, w, _)) in enumerate(zip(grads, c['levels'])):
        assert g.dtype == dt
        _check(g, ref['grads'][l] * gscale, dt, f'{what} grad level {l}')
        bg = ~ref['fg'][:, a0:a0 + h * w].reshape(c['B'], 1, h, w)
        box = g[:, :4 * c['R']].float().cpu()
        assert (box[bg.expand_as(box)] == 0).all(), (what, l, 'box gradient at a background anchor')
        a0 += h * w


def _run_case(name, dt, calls, gscale):
    from mgdt_yolo_amd import ops
    c = CASES[name]
    ref = _reference(name, dt, calls)
    views, bufs = _to_device(name, dt)
    gt = _inputs(name, dt)[1].to(DEV)
    what = f'{name}-{DTN[dt]}-call{calls}'
    st = ops.detect_loss_fwd(views, [l[2] for l in c['levels']], c['R'], c['nc'], gt, calls, GAINS, want_assignment=True)
    _check_forward(st, ref, what)
    grads = ops.detect_loss_bwd(st, gscale)
    _check_backward(grads, ref, c, dt, gscale, what)
    for big, big0 in bufs:
        assert torch.equal(big.cpu(), big0), (what, 'an input buffer was written')
    assert ref['fg'].any()


LOSS_RUNS = [(n, dt, cc, 1.0) for n in SMALL for dt in CASES[n]['dts'] for cc in CASES[n]['calls']] + \
            [(n, dt, 0, 1024.0) for n in ('levels3-scalar', 'a400-vec') for dt in (F32, BF16)]


@gpu
@pytest.mark.parametrize('name,dt,calls,gscale', LOSS_RUNS, ids=lambda v: DTN.get(v, None) if isinstance(v, torch.dtype) else str(v))
def test_loss_and_assigner_match_float64(name, dt, calls, gscale):
    """One detect_loss_fwd(want_assignment) and one detect_loss_bwd per case of the table in DESIGN.md section 4: fg / target_gt_idx bit-exact,
    tscore, items, total * B and max(sum tscore, 1) under the fp32 bound, the gradient of every level under the bound of the map dtype against
    gscale x autograd, box-channel gradients of background anchors exactly 0, input buffers (slice borders included) unchanged."""
    _run_case(name, dt, calls, gscale)


@gpu
def test_vec_backward_grid_stride_loop():
    """loss_bwd_vec_kernel beyond its 16384-block cap: 4 x 66 x 64 anchors x (1 + 1000 / 4) quads = 4 240 896 items > 4 194 304, bf16; the whole
    34 MB gradient is compared.  The float64 reference of this case (oracle + autograd over 17 M logits) takes about 1 s on the CPU."""
    _run_case('stride-loop', BF16, 0, 1.0)


@gpu
@pytest.mark.parametrize('calls', CALLS)
@pytest.mark.parametrize('dt', DTS)
def test_device_counter_entry_point(dt, calls):
    """mgdt_detect_loss_fwd_dev (the alpha schedule read from an int32 on the device) against the host-counter call: fg / target_gt_idx identical,
    and each result separately against float64."""
    from mgdt_yolo_amd import ops
    name = 'levels3-scalar'
    c = CASES[name]
    ref = _reference(name, dt, calls)
    views, _ = _to_device(name, dt)
    gt = _inputs(name, dt)[1].to(DEV)
    strides = [l[2] for l in c['levels']]
    host = ops.detect_loss_fwd(views, strides, c['R'], c['nc'], gt, calls, GAINS, want_assignment=True)
    counter = torch.tensor([calls], dtype=torch.int32, device=DEV)
    dev = ops.detect_loss_fwd(views, strides, c['R'], c['nc'], gt, 0, GAINS, want_assignment=True, call_count_dev=counter)
    _exact(dev.fg, host.fg.cpu(), 'fg dev vs host')
    _exact(dev.gt_idx, host.gt_idx.cpu(), 'gt_idx dev vs host')
    _check_forward(host, ref, f'host counter {calls}')
    _check_forward(dev, ref, f'device counter {calls}')
    assert int(counter.item()) == calls


@gpu
@pytest.mark.parametrize('nc', [3, 4], ids=['nc3-scalar', 'nc4-vec'])
@pytest.mark.parametrize('dt', DTS)
def test_empty_labels(dt, nc):
    """n_gt = 0 over two levels: every anchor background, box and dfl items exactly 0, the cls item and the gradient the float64 BCE against
    all-zero targets, box-channel gradients exactly 0."""
    from mgdt_yolo_amd import ops
    c = dict(levels=((13, 11, 8), (7, 6, 16)), B=2, R=4, nc=nc)
    maps = loss_maps(_gen('loss-empty', nc), 2, 4, nc, c['levels'], dt)
    gt = torch.zeros(2, 0, 5, dtype=F32)
    ref = loss_reference(maps, gt, [8.0, 16.0], 4, nc, 0)
    assert not ref['fg'].any() and ref['items'][0] == 0 and ref['items'][2] == 0 and ref['items'][1] > 0
    views = [_nhwc(m, dt)[0] for m in maps]
    st = ops.detect_loss_fwd(views, [8.0, 16.0], 4, nc, gt.to(DEV), 0, GAINS, want_assignment=True)
    _check_forward(st, ref, 'empty')
    assert (st.fg == 0).all() and (st.tscore == 0).all() and st.out5[1].item() == 0 and st.out5[3].item() == 0 and st.out5[4].item() == 1
    _check_backward(ops.detect_loss_bwd(st, 1.0), ref, c, dt, 1.0, 'empty')


# ------------------------------------------------------------------------------------------------ GPU: optimizer kernels
LR, LR_BIAS, MOM = 0.01, 0.1, 0.937
N_CLIP = [1, 255, 257, 1024 * 256 + 3]          # the last: beyond the 1024-block cap of sumsq_partial_kernel
N_FLAT = [1, 257, 8192 * 256 + 5]               # the last: beyond the 8192-block cap of the flat kernels


def _d(t):
    return t.float().to(DEV).contiguous()


def _wd(n):
    """The three parameter groups interleaved: decay 5e-4, no decay, the bias group (-1: no decay, lr_bias)."""
    return torch.tensor([5e-4, 0.0, -1.0], dtype=F32).repeat(n // 3 + 1)[:n].clone()


def _clip2(coef):
    return None if coef is None else torch.tensor([123.0, coef], dtype=F32, device=DEV)


@gpu
@pytest.mark.parametrize('n,regime', [(n, r) for n in N_CLIP for r in ('below', 'above', 'mixed') if n > 1 or r != 'mixed'])      # one element cannot mix magnitudes
def test_grad_clip_coef(n, regime):
    """mgdt_grad_clip_coef: norm and min(1, max_norm / (norm + 1e-6)) against float64; below max_norm the coefficient is exactly 1.0; entries of
    magnitude 1e-20 and 1e+15 mixed keep a finite norm (the squares are accumulated in double)."""
    from mgdt_yolo_amd import ops
    gen = _gen('clip', n, regime)
    g = _rand(gen, n)
    if regime == 'mixed':
        g = (torch.where(torch.arange(n) % 2 == 0, 1e-20, 1e15) * (1.0 + 0.25 * torch.rand(n, generator=gen)) * torch.sign(g)).float().double()
        assert g.abs().min() < 1e-19 and g.abs().max() >= 1e15
    max_norm = 10.0 if regime == 'mixed' else float(g.norm()) * (2.0 if regime == 'below' else 0.5)
    norm, coef = ref_clip(g, max_norm)
    out = ops.grad_clip_coef(_d(g), max_norm)
    _check(out[0:1], norm.reshape(1), F32, f'norm n={n} {regime}')
    _check(out[1:2], coef.reshape(1), F32, f'coef n={n} {regime}')
    if regime == 'below':
        assert coef.item() == 1.0 and out[1].item() == 1.0
    else:
        assert coef.item() < 1.0 and out[1].item() < 1.0


def _sgd_three_steps(n, first, nesterov, coef, wd, what):
    from mgdt_yolo_amd import ops
    gen = _gen('sgd', what, n, first, nesterov, coef)
    p, buf = _rand(gen, n), _rand(gen, n, scale=0.3)          # with first = 1 the buffer's content must be ignored
    dp, dbuf, dwd = _d(p), _d(buf), None if wd is None else _d(wd)
    for s in range(3):
        g = _rand(gen, n)
        lr, lrb, mom = LR * (1 + s), LR_BIAS / (1 + s), MOM - 0.1 * s
        fst = first if s == 0 else 0
        ops.sgd_step(dp, _d(g), dbuf, dwd, lr, mom, nesterov, fst, clip=_clip2(coef), lr_bias=lrb)
        p, buf = ref_sgd(p, g, buf, wd, lr, lrb, mom, nesterov, fst, 1.0 if coef is None else f32r(coef))
        _check(dbuf, buf, F32, f'{what} buf step {s}')
        _check(dp, p, F32, f'{what} p step {s}')


@gpu
@pytest.mark.parametrize('coef', [None, 0.37], ids=['noclip', 'clip0.37'])
@pytest.mark.parametrize('nesterov', [0, 1])
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('n', N_FLAT)
def test_sgd_step_recurrence(n, first, nesterov, coef):
    """mgdt_sgd_step over three consecutive steps with changing gradients and scalars, buf and p checked after each: the momentum recurrence
    momentum * buf + g', the decay group, the bias group's own learning rate (lr_bias = 10 x lr), Nesterov, the clip coefficient."""
    _sgd_three_steps(n, first, nesterov, coef, _wd(n), 'groups')


@gpu
@pytest.mark.parametrize('n', N_FLAT)
def test_sgd_step_without_groups(n):
    """wd = NULL: no decay and lr everywhere."""
    _sgd_three_steps(n, 1, 1, 0.37, None, 'wd-none')


@gpu
@pytest.mark.parametrize('decay', [0.0, 0.5, 0.9999])
@pytest.mark.parametrize('n', N_FLAT)
def test_ema_update(n, decay):
    from mgdt_yolo_amd import ops
    gen = _gen('ema', n, decay)
    ema, p = _rand(gen, n), _rand(gen, n)
    dema = _d(ema)
    ops.ema_update(dema, _d(p), decay)
    _check(dema, ref_ema(ema, p, decay), F32, f'ema n={n} d={decay}')


@gpu
@pytest.mark.parametrize('with_ema', [True, False], ids=['ema', 'noema'])
@pytest.mark.parametrize('nesterov', [0, 1])
@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('n_param', [257, 259, 8192 * 256 + 5])          # % 4 == 1, 3, 1: the quad that straddles n_param is cut both ways
def test_sgd_ema_step_dev(n_param, first, nesterov, with_ema):
    """mgdt_sgd_ema_step_dev (the kernel of the captured step) over three steps with `hyper` rewritten on the device between them and the clip
    coefficient present, absent, present: p, buf, ema against float64; the 1000-element tail [n_param, n_total) receives EMA only and keeps its p
    bit for bit; without an EMA buffer p and buf still match; and the result is bit-equal to mgdt_sgd_step followed by mgdt_ema_update (same
    operations in the same order, both built without contraction)."""
    from mgdt_yolo_amd import ops
    n_total = n_param + 1000
    gen = _gen('sgd-ema-dev', n_param, first, nesterov, with_ema)
    data, buf, ema, wd = _rand(gen, n_total), _rand(gen, n_param, scale=0.3), _rand(gen, n_total), _wd(n_param)
    d_data, d_buf, d_ema, d_wd = _d(data), _d(buf), _d(ema) if with_ema else None, _d(wd)
    s_data, s_buf, s_ema = d_data.clone(), d_buf.clone(), _d(ema)                   # the two-kernel chain on the same inputs
    hyper = torch.zeros(4, dtype=F32, device=DEV)
    tail0 = data[n_param:].clone()
    for s in range(3):
        g = _rand(gen, n_param)
        lr, lrb, mom, dec = LR * (1 + s), LR_BIAS / (1 + s), MOM - 0.1 * s, (0.0, 0.5, 0.9999)[s]
        coef = None if s == 1 else 0.37
        fst = first if s == 0 else 0
        hyper.copy_(torch.tensor([lr, lrb, mom, dec], dtype=F32))
        ops.sgd_ema_step_dev(d_data[:n_param], _d(g), d_buf, d_wd, d_ema, d_data, hyper, nesterov, fst, clip=_clip2(coef))
        ops.sgd_step(s_data[:n_param], _d(g), s_buf, d_wd, lr, mom, nesterov, fst, clip=_clip2(coef), lr_bias=lrb)
        if with_ema:
            ops.ema_update(s_ema, s_data, dec)
        pn, buf = ref_sgd(data[:n_param], g, buf, wd, lr, lrb, mom, nesterov, fst, 1.0 if coef is None else f32r(coef))
        data = torch.cat([pn, data[n_param:]])
        ema = ref_ema(ema, data, dec)
        what = f'n={n_param} step {s}'
        _check(d_buf, buf, F32, what + ' buf')
        _check(d_data, data, F32, what + ' p')
        _exact(d_data[n_param:], tail0, what + ' tail of p')
        _exact(d_data, s_data.cpu(), what + ' p vs sgd_step')
        _exact(d_buf, s_buf.cpu(), what + ' buf vs sgd_step')
        if with_ema:
            _check(d_ema, ema, F32, what + ' ema')
            _exact(d_ema, s_ema.cpu(), what + ' ema vs ema_update')


# The flat kernel takes 16-byte accesses only when every array it is given is 16-byte aligned; otherwise every element goes through the scalar
# path, which evaluates the same element function.  n_param % 4 == 3 and n_total % 4 == 0: a straddling quad and no tail when aligned.
N_PARAM_Q, N_TOTAL_Q, SENTINEL = 259, 268, 12345.0


def _place(t, shifted):
    """Device copy of the CPU tensor t as a view into a SENTINEL-filled allocation with slack on both sides: 16-byte aligned, or with `shifted`
    starting one float into it.  Returns (view, allocation, offset of the view)."""
    big = torch.full((t.numel() + 8,), SENTINEL, dtype=F32, device=DEV)
    off = 1 if shifted else 4
    view = big[off:off + t.numel()]
    view.copy_(t.float())
    assert view.data_ptr() % 16 == (4 if shifted else 0)
    return view, big, off


def _flat_case(kind, gen):
    """Inputs of one step of `kind` ('sgd', 'adam', 'rmsprop', 'ema'), |g| >= 0.05 and v a square of such a magnitude so that the float64 bound
    holds for the divisions; a function that runs the step on placed arrays; which arrays it writes; and the float64 results."""
    from mgdt_yolo_amd import ops
    n_param, n_total = N_PARAM_Q, N_TOTAL_Q
    lr, lrb, mom, dec, coef, beta2, alpha, eps, step = LR, LR_BIAS, 0.9, 0.5, 0.37, 0.999, 0.99, 1e-8, 4
    a = dict(data=_rand(gen, n_total), ema=_rand(gen, n_total))
    if kind == 'ema':
        return a, lambda V: ops.ema_update(V['ema'], V['data'], dec), dict(data=a['data'], ema=ref_ema(a['ema'], a['data'], dec))
    r = _rand(gen, n_param)
    a.update(g=(torch.where(r < 0, -1.0, 1.0) * (0.05 + r.abs())).float().double(), m=_rand(gen, n_param, scale=0.3), wd=_wd(n_param).double())
    p, c, clip = a['data'][:n_param], f32r(coef), _clip2(coef)
    if kind == 'sgd':
        hyper = torch.tensor([lr, lrb, mom, dec], dtype=F32, device=DEV)
        pn, m = ref_sgd(p, a['g'], a['m'], a['wd'], lr, lrb, mom, 1, 0, c)
        ref = dict(m=m)

        def run(V):
            ops.sgd_ema_step_dev(V['data'][:n_param], V['g'], V['m'], V['wd'], V['ema'], V['data'], hyper, 1, 0, clip=clip)
    else:
        a['v'] = ((0.05 + _rand(gen, n_param).abs()) ** 2).float().double()
        if kind == 'adam':
            hyper = torch.tensor(ops.adam_hyper(lr, lrb, mom, beta2, step, dec), dtype=F32, device=DEV)
            pn, m, v = ref_adam(p, a['g'], a['m'], a['v'], a['wd'], lr, lrb, mom, beta2, eps, step, 1, c)

            def run(V):
                ops.adam_ema_step_dev(V['data'][:n_param], V['g'], V['m'], V['v'], V['wd'], V['ema'], V['data'], hyper, beta2, eps, 1, clip=clip)
        else:
            hyper = torch.tensor(ops.rmsprop_hyper(lr, lrb, mom, dec), dtype=F32, device=DEV)
            pn, v, m = ref_rmsprop(p, a['g'], a['v'], a['m'], a['wd'], lr, lrb, alpha, eps, mom, c)

            def run(V):
                ops.rmsprop_ema_step_dev(V['data'][:n_param], V['g'], V['v'], V['m'], V['wd'], V['ema'], V['data'], hyper, alpha, eps, True, clip=clip)
        ref = dict(m=m, v=v)
    ref['data'] = torch.cat([pn, a['data'][n_param:]])
    ref['ema'] = ref_ema(a['ema'], ref['data'], dec)
    return a, run, ref


@gpu
@pytest.mark.parametrize('kind', ['sgd', 'adam', 'rmsprop', 'ema'])
def test_unaligned_arrays_take_the_scalar_path(kind):
    """One step of mgdt_sgd_ema_step_dev / mgdt_adam_ema_step_dev / mgdt_rmsprop_ema_step_dev (with momentum) / mgdt_ema_update from the same
    values three times: every array 16-byte aligned; one array (wd; p for the EMA) starting one float into its allocation; every array so.  The
    two scalar-path runs give the bits of the aligned run, all three stay inside the float64 bound, and the slack around every view is left
    alone."""
    a, run, ref = _flat_case(kind, _gen('flat-unaligned', kind))
    one = 'data' if kind == 'ema' else 'wd'
    aligned = None
    for shifted in ((), (one,), tuple(a)):
        placed = {k: _place(t, k in shifted) for k, t in a.items()}
        run({k: view for k, (view, _, _) in placed.items()})
        for k, (view, big, off) in placed.items():
            slack = torch.cat([big[:off], big[off + view.numel():]]).cpu()
            assert slack.numel() == 8 and (slack == SENTINEL).all(), (kind, shifted, k, 'slack written')
        got = {k: placed[k][0].cpu() for k in ref}
        for k in ref:
            _check(got[k], ref[k], F32, f'{kind} shifted={shifted} {k}')
            if aligned is not None:
                _exact(got[k], aligned[k], f'{kind} shifted={shifted} {k} vs aligned')
        aligned = aligned or got
    _exact(got['data'][N_PARAM_Q:], a['data'][N_PARAM_Q:], kind + ' tail of p')


@gpu
def test_sgd_ema_step_dev_reads_four_hyper_slots():
    """`hyper` of mgdt_sgd_ema_step_dev is fp32[4]: with an 8-float vector whose slots 4..7 are NaN the result is the same bit for bit."""
    a, _, ref = _flat_case('sgd', _gen('sgd-hyper4'))
    from mgdt_yolo_amd import ops
    out = []
    for extra in ([], [float('nan')] * 4):
        V = {k: _d(t) for k, t in a.items()}
        hyper = torch.tensor([LR, LR_BIAS, 0.9, 0.5] + extra, dtype=F32, device=DEV)
        ops.sgd_ema_step_dev(V['data'][:N_PARAM_Q], V['g'], V['m'], V['wd'], V['ema'], V['data'], hyper, 1, 0, clip=_clip2(0.37))
        out.append({k: V[k].cpu() for k in ref})
    for k in ref:
        _check(out[0][k], ref[k], F32, f'hyper4 {k}')
        _exact(out[1][k], out[0][k], f'hyper8 with NaN in 4..7, {k}')


@gpu
@pytest.mark.parametrize('form', ['eager', 'dev'])
def test_sgd_first_step_ignores_a_nan_buffer(form):
    """first = 1: the momentum buffer becomes g' whatever it held - here NaN in every element, vector path and straddling quad alike."""
    from mgdt_yolo_amd import ops
    n = N_PARAM_Q
    gen = _gen('sgd-first-nan', form)
    p, g, wd = _rand(gen, n), _rand(gen, n), _wd(n)
    dp, dbuf = _d(p), torch.full((n,), float('nan'), dtype=F32, device=DEV)
    if form == 'eager':
        ops.sgd_step(dp, _d(g), dbuf, _d(wd), LR, MOM, 1, 1, clip=_clip2(0.37), lr_bias=LR_BIAS)
    else:
        hyper = torch.tensor([LR, LR_BIAS, MOM, 0.5], dtype=F32, device=DEV)
        ops.sgd_ema_step_dev(dp, _d(g), dbuf, _d(wd), None, dp, hyper, 1, 1, clip=_clip2(0.37))
    rp, rbuf = ref_sgd(p, g, torch.zeros(n, dtype=torch.float64), wd, LR, LR_BIAS, MOM, 1, 1, f32r(0.37))
    assert torch.isfinite(dp).all() and torch.isfinite(dbuf).all()
    _check(dbuf, rbuf, F32, f'first with NaN buffer, {form}: buf')
    _check(dp, rp, F32, f'first with NaN buffer, {form}: p')
