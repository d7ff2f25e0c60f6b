"""Adam / AdamW / RMSProp and optimizer='auto' (yolo/engine/trainer.py:614-668 build_optimizer, :317-326 warm-up, :260-264 schedule of the reference).

Kernel tests (GPU): mgdt_adam_step / mgdt_rmsprop_step against the float64 restatements of optim_ref.py AND against float64 torch.optim.Adam /
AdamW / RMSprop run on the three groups (the reference's optimizer), within kernel_ref._close's fp32 bound: maximum error at most 1e-4 of the
largest reference magnitude and relative L2 at most 2e-5.  The inputs are drawn so that the bound is a fair one - second moments are squares of
magnitudes >= 0.05, gradients have |g| >= 0.05 (>= 0.016 after the clip coefficient 0.37 and the decay term), so Adam's sqrt(v) / sqrt(bc2) + eps and RMSProp's
sqrt(sq) + eps stay >= 1e-3, from zero state too - and test_kernel_inputs_keep_torch_fp32_inside_the_bound checks
on the CPU that torch's own fp32 step stays inside the same bound on exactly these inputs.  The captured-step forms are compared bit for bit
with the eager kernel followed by mgdt_ema_update.

Trainer tests: the `auto` rule, the per-optimizer warm-up and cos_lr against tests/golden/optim_traj.npz (gen_optim.py: the reference's
build_optimizer, warm-up lines, clip, optimizer.step and ModelEMA on seeded gradients), the optimizer state in torch's layout, and on the GPU
the recorded trajectories, captured == eager, the packed-weight caches and a falling loss.
"""
import functools

import numpy as np
import pytest
import torch

import optim_inputs as OI
from kernel_ref import DEV, F32, _check, _exact, _gen, _rand, f32r, ref_ema
from mgdt_yolo_amd import _lib
from mgdt_yolo_amd.models import get_config
from mgdt_yolo_amd.nn import tasks
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images
from optim_ref import ref_adam, ref_rmsprop

gpu = pytest.mark.gpu
N_FLAT = [1, 257, 8192 * 256 + 5]               # one element; a scalar tail past a full block; past the grid cap with n % 4 != 0
EPS, ALPHA = 1e-8, 0.99
STARTS = ['zero', 'random']
COEFS = [pytest.param(None, id='noclip'), pytest.param(0.37, id='clip0.37')]


def _d(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _wd(n):
    """The three parameter groups interleaved: decay 5e-4, no decay, the bias group (-1: no decay, lr_bias)."""
    return torch.tensor([5e-4, 0.0, -1.0], dtype=F32).repeat(n // 3 + 1)[:n].clone()


def _clip2(coef):
    return None if coef is None else torch.tensor([123.0, coef], dtype=F32, device=DEV)


def _grad(gen, n):
    r = _rand(gen, n)
    return (torch.where(r < 0, -1.0, 1.0) * (0.05 + r.abs())).float().double()


def _adam_scalars(s, start):
    """lr of order 0.5 (the update is comparable to p), changing every step; `step` continues from 3 on a random state."""
    return dict(lr=0.5 / (1 + s), lr_bias=0.3 * (1 + s), beta1=0.9 - 0.1 * s, beta2=0.999 - 0.01 * s, step=s + 1 + (3 if start == 'random' else 0))


def _rms_scalars(s, momentum):
    return dict(lr=0.5 / (1 + s), lr_bias=0.3 * (1 + s), momentum=max(momentum - 0.1 * s, 0.0))


@functools.lru_cache(maxsize=None)
def _inputs(kind, n, start):
    """p, first-moment-like state, second-moment state (squares of magnitudes >= 0.05) and three gradients (|g| >= 0.05): CPU fp64 values
    representable in fp32.  Shared, unchanged, by the CPU condition test and the GPU tests."""
    gen = _gen('optim-kernel', kind, n, start)
    p = _rand(gen, n)
    if start == 'zero':
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    else:
        m, v = _rand(gen, n, scale=0.3), ((0.05 + _rand(gen, n).abs()) ** 2).float().double()
    return p, m, v, [_grad(gen, n) for _ in range(3)]


def _torch_run(kind, n, start, variant, coef, dtype):
    """The reference's optimizer: torch.optim.Adam / AdamW / RMSprop in `dtype` on the three groups [bias, decay, norm] of the interleaved
    layout, hyper-parameters rewritten per step as the warm-up does; returns per step the flat (p, m, v) (m None for RMSprop without momentum)."""
    p0, m0, v0, grads = _inputs(kind, n, start)
    wd = _wd(n)
    sel = [(wd < 0).nonzero().reshape(-1), (wd > 0).nonzero().reshape(-1), (wd == 0).nonzero().reshape(-1)]
    sel = [(gi, ix) for gi, ix in enumerate(sel) if ix.numel()]
    params = {gi: torch.nn.Parameter(p0[ix].to(dtype)) for gi, ix in sel}
    groups = [{'params': [params[gi]], 'weight_decay': 5e-4 if gi == 1 else 0.0} for gi, _ in sel]
    if kind == 'adam':
        opt = (torch.optim.AdamW if variant else torch.optim.Adam)(groups, lr=1.0, eps=EPS)
        mkey, vkey = 'exp_avg', 'exp_avg_sq'
    else:
        opt = torch.optim.RMSprop(groups, lr=1.0, alpha=ALPHA, eps=EPS, momentum=variant)
        mkey, vkey = 'momentum_buffer', 'square_avg'
    if start == 'random':
        for gi, ix in sel:
            e = {'step': torch.tensor(3.0), vkey: v0[ix].to(dtype)}
            if kind == 'adam' or variant > 0:
                e[mkey] = m0[ix].to(dtype)
            opt.state[params[gi]] = e
    out = []
    for s in range(3):
        sc = _adam_scalars(s, start) if kind == 'adam' else _rms_scalars(s, variant)
        for g, (gi, ix) in zip(opt.param_groups, sel):
            g['lr'] = sc['lr_bias'] if gi == 0 else sc['lr']
            if kind == 'adam':
                g['betas'] = (sc['beta1'], sc['beta2'])
            else:
                g['momentum'] = sc['momentum']
            c = 1.0 if coef is None else f32r(coef)
            params[gi].grad = (grads[s][ix] * c).to(dtype) if dtype == torch.float64 else grads[s][ix].to(dtype) * torch.tensor(c, dtype=dtype)
        opt.step()
        flat = [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
        for gi, ix in sel:
            st = opt.state[params[gi]]
            flat[0][ix] = params[gi].detach().double()
            flat[2][ix] = st[vkey].double()
            if mkey in st:
                flat[1][ix] = st[mkey].double()
        out.append(tuple(flat))
    return out


@functools.lru_cache(maxsize=None)
def _torch_f64(kind, n, start, variant, coef):
    return _torch_run(kind, n, start, variant, coef, torch.float64)


KERNEL_CASES = [('adam', n, st, dec) for n in N_FLAT for st in STARTS for dec in (0, 1)] + \
               [('rmsprop', n, st, mom) for n in N_FLAT for st in STARTS for mom in (0.0, 0.9)]


# ------------------------------------------------------------------------------------------------ not GPU
@pytest.mark.parametrize('coef', COEFS)
@pytest.mark.parametrize('kind,n,start,variant', KERNEL_CASES)
def test_kernel_inputs_keep_torch_fp32_inside_the_bound(kind, n, start, variant, coef):
    """The condition of the GPU kernel tests: on exactly their inputs torch's own fp32 CPU step stays within _close's fp32 bound of the same
    step in float64, for p and for both moments, after every one of the three steps."""
    p0, m0, v0, grads = _inputs(kind, n, start)
    assert all(g.abs().min() >= 0.05 for g in grads) and (start == 'zero' or v0.sqrt().min() >= 0.05 - 1e-6)
    f32, f64 = _torch_run(kind, n, start, variant, coef, torch.float32), _torch_f64(kind, n, start, variant, coef)
    for s in range(3):
        bc2 = 1 - _adam_scalars(s, start)['beta2'] ** _adam_scalars(s, start)['step'] if kind == 'adam' else 1.0
        assert (f64[s][2].sqrt() / bc2 ** 0.5 + EPS).min() >= 1e-3, 'the denominator left the conditioned range'
        for name, a, b in zip(('p', 'm', 'v'), f32[s], f64[s]):
            _check(a, b, F32, f'torch fp32 vs fp64 {kind} n={n} {start} {variant} step {s} {name}')


def test_auto_resolution_matches_the_reference(golden):
    """optimizer='auto' (build_optimizer trainer.py:635-639) for (nc, iterations) in {1, 2, 80} x {100, 10000, 10001}: name, lr, momentum and
    the mutated warmup_bias_lr as the reference's own build_optimizer decided them."""
    from mgdt_yolo_amd.yolo.engine.trainer import resolve_optimizer
    g = golden('optim_traj')
    names, vals = str(g['auto_name']).split('\n'), g['auto_vals']
    assert len(names) == len(OI.AUTO_CASES) == 9
    for (nc, it), name, (lr, mom, wbl) in zip(OI.AUTO_CASES, names, vals):
        got = resolve_optimizer('auto', nc, it, 0.001, 0.937, 0.1)
        assert got == (name, lr, mom, wbl), (nc, it, got, name, lr, mom, wbl)
    assert resolve_optimizer('RMSProp', 4, None, 0.001, 0.937, 0.1) == ('RMSProp', 0.001, 0.937, 0.1)


def _cpu_model(nc=4):
    return seed_state_dict_(tasks.DetectionModel(get_config('mspa_c2f_gd_yolov8', 'n', nc), verbose=False), 0)


def test_optimizer_names():
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer, resolve_optimizer
    with pytest.raises(ValueError, match='iterations'):
        DetectionTrainer(_cpu_model(), optimizer='auto')
    for name in ('Adamax', 'NAdam', 'RAdam'):
        with pytest.raises(NotImplementedError, match='not built'):
            resolve_optimizer(name, 4, None, 0.001, 0.937, 0.1)
    for name in ('adamw', 'Lion', ''):
        with pytest.raises(NotImplementedError, match=r'\[Adam, AdamW, NAdam, RAdam, RMSProp, SGD, auto\]'):
            resolve_optimizer(name, 4, None, 0.001, 0.937, 0.1)
    tr = DetectionTrainer(_cpu_model(), optimizer='auto', iterations=5000)
    assert (tr.optimizer, tr.lr0, tr.opt_momentum, tr.warmup_bias_lr) == ('AdamW', 0.00125, 0.9, 0.0) and tr.state.second_moment is not None
    tr = DetectionTrainer(_cpu_model(), optimizer='auto', iterations=20000)          # no schedule: SGD's own 0.9 is what steps
    tr.warmup(0)
    assert (tr.optimizer, tr.lr0, tr.opt_momentum, tr.mom, tr.warmup_bias_lr) == ('SGD', 0.01, 0.9, 0.9, 0.0) and tr.state.second_moment is None
    tr = DetectionTrainer(_cpu_model(), optimizer='auto', iterations=20000, batch_size=64, nb=10)
    tr.ni = 101; tr.warmup(0)                                                        # after the warm-up: its target, the `momentum` argument
    assert tr.mom == 0.937 and tr.opt_momentum == 0.9
    tr = DetectionTrainer(_cpu_model())                                              # the default stays the SGD trainer
    assert tr.optimizer == 'SGD' and tr.state.second_moment is None and tr.opt_momentum == 0.937


@pytest.mark.parametrize('tag', list(OI.TRAJ))
def test_schedule_per_optimizer_matches_the_reference_loop(golden, tag):
    """lr of the groups [bias, decay, norm] and the momentum / beta1 per iteration as the reference's warm-up lines set them on the optimizer
    its build_optimizer returned: beta1 of Adam / AdamW never moves, RMSProp's momentum is warmed."""
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    g = golden('optim_traj')
    name, iterations, n_it, _ = OI.TRAJ[tag]
    A = OI.TRAJ_ARGS
    tr = DetectionTrainer(_cpu_model(A['nc']), optimizer=name, iterations=iterations, batch_size=A['batch'], nb=A['nb'])
    assert tr.nw == A['nw'] and tr.accumulate == 1
    assert {'AdamW': 'AdamW', 'Adam': 'Adam', 'RMSProp': 'RMSprop'}[tr.optimizer] == str(g[f'{tag}_type'])
    assert (tr.lr0, tr.warmup_bias_lr) == tuple(g[f'{tag}_resolved'])
    for it in range(n_it):
        tr.ni = it
        tr.warmup(0)
        assert (tr.lr_bias, tr.lr, tr.lr) == pytest.approx(tuple(g[f'{tag}_lr'][it]), rel=1e-12, abs=0)
        assert tr.mom == pytest.approx(g[f'{tag}_mom'][it][0], rel=1e-12)
    moms = g[f'{tag}_mom'][:, 0]
    if tag == 'rmsprop':
        assert moms[0] == 0.8 and (np.diff(moms) > 0).all()
    else:
        assert (moms == tr.opt_momentum).all()
        tr.ni = 1000; tr.warmup(5)
        assert tr.mom == tr.opt_momentum


def test_cos_lr_is_the_reference_one_cycle(golden):
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    tr = DetectionTrainer(_cpu_model(), cos_lr=True, lrf=0.01, epochs=100)
    assert [tr.lf(e) for e in OI.ONE_CYCLE_EPOCHS] == list(golden('optim_traj')['one_cycle'])
    tr = DetectionTrainer(_cpu_model(), lrf=0.01, epochs=100)
    assert tr.lf(50) == (1 - 50 / 100) * (1.0 - 0.01) + 0.01


def test_new_entry_points_reject_bad_arguments():
    """-4 (MGDT_BAD_ARG) before any launch: null pointers, n <= 0, n_total < n_param, step < 1.  No GPU needed."""
    lib = _lib.lib()
    x = 64          # a non-null address that is never dereferenced
    for name in ('mgdt_adam_step', 'mgdt_adam_ema_step_dev', 'mgdt_rmsprop_step', 'mgdt_rmsprop_ema_step_dev'):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.mgdt_adam_step(None, x, x, x, x, 8, 0.1, 0.1, 0.9, 0.999, 1e-8, 1, 1, None, None) == -4
    assert lib.mgdt_adam_step(x, x, x, None, x, 8, 0.1, 0.1, 0.9, 0.999, 1e-8, 1, 1, None, None) == -4
    assert lib.mgdt_adam_step(x, x, x, x, x, 0, 0.1, 0.1, 0.9, 0.999, 1e-8, 1, 1, None, None) == -4
    assert lib.mgdt_adam_step(x, x, x, x, x, 8, 0.1, 0.1, 0.9, 0.999, 1e-8, 0, 1, None, None) == -4
    assert lib.mgdt_adam_ema_step_dev(x, x, x, x, x, 8, x, 8, None, 0.999, 1e-8, 1, None, None) == -4
    assert lib.mgdt_adam_ema_step_dev(x, x, x, x, x, 8, x, 7, x, 0.999, 1e-8, 1, None, None) == -4
    assert lib.mgdt_adam_ema_step_dev(x, None, x, x, x, 8, x, 8, x, 0.999, 1e-8, 1, None, None) == -4
    assert lib.mgdt_rmsprop_step(x, x, None, x, x, 8, 0.1, 0.1, 0.99, 1e-8, 0.9, None, None) == -4
    assert lib.mgdt_rmsprop_step(x, x, x, None, x, 8, 0.1, 0.1, 0.99, 1e-8, 0.9, None, None) == -4          # momentum needs its buffer
    assert lib.mgdt_rmsprop_step(x, x, x, x, x, -1, 0.1, 0.1, 0.99, 1e-8, 0.9, None, None) == -4
    assert lib.mgdt_rmsprop_ema_step_dev(x, x, x, x, x, 8, x, 8, None, 0.99, 1e-8, 1, None, None) == -4
    assert lib.mgdt_rmsprop_ema_step_dev(x, x, x, None, x, 8, x, 8, x, 0.99, 1e-8, 1, None, None) == -4
    assert lib.mgdt_rmsprop_ema_step_dev(x, x, x, x, x, 8, x, 4, x, 0.99, 1e-8, 1, None, None) == -4


def _reference_ordered(model):
    from mgdt_yolo_amd.yolo.engine.trainer import param_groups
    grp, params = param_groups(model), dict(model.named_parameters())
    return [[params[n] for n, g in grp.items() if g == k] for k in (2, 0, 1)]


@pytest.mark.parametrize('name,cls', [('AdamW', torch.optim.AdamW), ('Adam', torch.optim.Adam), ('RMSProp', torch.optim.RMSprop), ('SGD', torch.optim.SGD)])
def test_optimizer_state_dict_round_trip(name, cls):
    """optimizer_state_dict() is torch's layout for the reference's groups [bias, decay, norm]: torch's own optimizer on those groups loads
    it; load_optimizer_state_dict(optimizer_state_dict()) is the identity; a state of another optimizer or other shapes raises."""
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    m = _cpu_model()
    tr = DetectionTrainer(m, optimizer=name)
    assert tr.optimizer_state_dict()['state'] == {}                # before the first step, as torch's
    gen = _gen('state-dict', name)
    st = tr.state
    st.momentum_buf.copy_(torch.randn(st.n_param, generator=gen))
    if st.second_moment is not None:
        st.second_moment.copy_(torch.rand(st.n_param, generator=gen))
    st.steps = 3
    sd = tr.optimizer_state_dict()
    groups = _reference_ordered(m)
    assert [len(g['params']) for g in sd['param_groups']] == [len(g) for g in groups] and sd['param_groups'][1]['weight_decay'] == 5e-4
    kw = dict(momentum=0.937) if name in ('SGD', 'RMSProp') else {}
    opt = cls([{'params': g} for g in groups], lr=0.001, **kw)
    opt.load_state_dict(sd)
    keys = {'AdamW': ('exp_avg', 'exp_avg_sq'), 'Adam': ('exp_avg', 'exp_avg_sq'), 'RMSProp': ('momentum_buffer', 'square_avg'), 'SGD': ('momentum_buffer',)}[name]
    p = dict(m.named_parameters())['model.0.conv.weight']
    off, k = st.offsets['model.0.conv.weight']
    assert set(opt.state[p]) - {'step'} == set(keys)
    for key in keys:
        src = st.momentum_buf if key in ('exp_avg', 'momentum_buffer') else st.second_moment
        assert torch.equal(opt.state[p][key].reshape(-1), src[off:off + k])
    if name != 'SGD':
        assert float(opt.state[p]['step']) == 3
    frozen = [q for q in m.parameters() if not q.requires_grad]
    assert frozen and all(q not in opt.state for q in frozen)      # dfl.conv.weight is a group member without state
    # identity
    tr2 = DetectionTrainer(_cpu_model(), optimizer=name)
    tr2.load_optimizer_state_dict(sd)
    assert torch.equal(tr2.state.momentum_buf, st.momentum_buf)
    assert st.second_moment is None or torch.equal(tr2.state.second_moment, st.second_moment)
    sd2 = tr2.optimizer_state_dict()
    assert sd2['state'].keys() == sd['state'].keys()
    for i, e in sd['state'].items():
        assert e.keys() == sd2['state'][i].keys() and all(torch.equal(torch.as_tensor(e[k]), torch.as_tensor(sd2['state'][i][k])) for k in e)
    if name != 'SGD':
        assert tr2.state.steps + tr2.opt_step_offset == 3
    # another optimizer's state, other shapes
    other = DetectionTrainer(_cpu_model(), optimizer='SGD' if name != 'SGD' else 'AdamW')
    with pytest.raises(ValueError, match='needs'):
        other.load_optimizer_state_dict(sd)
    bad = {'state': {i: dict(e) for i, e in sd['state'].items()}, 'param_groups': sd['param_groups']}
    i0 = next(iter(bad['state']))
    bad['state'][i0][keys[0]] = torch.zeros(3, 5)
    with pytest.raises(ValueError, match='shape'):
        tr2.load_optimizer_state_dict(bad)
    bad = {'state': sd['state'], 'param_groups': sd['param_groups'][:2]}
    with pytest.raises(ValueError, match='groups'):
        tr2.load_optimizer_state_dict(bad)


# ------------------------------------------------------------------------------------------------ GPU: kernels
@gpu
@pytest.mark.parametrize('coef', COEFS)
@pytest.mark.parametrize('decoupled', [0, 1], ids=['adam', 'adamw'])
@pytest.mark.parametrize('start', STARTS)
@pytest.mark.parametrize('n', N_FLAT)
def test_adam_step(n, start, decoupled, coef):
    """mgdt_adam_step over three consecutive steps with changing gradients and scalars: m, v, p after every step against the float64
    restatement and against float64 torch.optim.Adam / AdamW on the three groups."""
    from mgdt_yolo_amd import ops
    p, m, v, grads = _inputs('adam', n, start)
    wd = _wd(n)
    dp, dm, dv, dwd = _d(p), _d(m), _d(v), _d(wd)
    ref = _torch_f64('adam', n, start, decoupled, coef)
    c = 1.0 if coef is None else f32r(coef)
    for s in range(3):
        sc = _adam_scalars(s, start)
        ops.adam_step(dp, _d(grads[s]), dm, dv, dwd, sc['lr'], sc['beta1'], sc['beta2'], EPS, sc['step'], decoupled, clip=_clip2(coef), lr_bias=sc['lr_bias'])
        p, m, v = ref_adam(p, grads[s], m, v, wd, sc['lr'], sc['lr_bias'], sc['beta1'], sc['beta2'], EPS, sc['step'], decoupled, c)
        for name, got, r, t in (('m', dm, m, ref[s][1]), ('v', dv, v, ref[s][2]), ('p', dp, p, ref[s][0])):
            _check(got, r, F32, f'adam n={n} {start} dec={decoupled} step {s} {name} vs restatement')
            _check(got, t, F32, f'adam n={n} {start} dec={decoupled} step {s} {name} vs torch f64')


@gpu
@pytest.mark.parametrize('coef', COEFS)
@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('start', STARTS)
@pytest.mark.parametrize('n', N_FLAT)
def test_rmsprop_step(n, start, momentum, coef):
    """mgdt_rmsprop_step, momentum 0 and 0.9, same protocol; without momentum the buffer is left alone (and may be NULL)."""
    from mgdt_yolo_amd import ops
    p, buf, sq, grads = _inputs('rmsprop', n, start)
    wd = _wd(n)
    dp, dbuf, dsq, dwd = _d(p), _d(buf), _d(sq), _d(wd)
    buf0 = dbuf.clone()
    ref = _torch_f64('rmsprop', n, start, momentum, coef)
    c = 1.0 if coef is None else f32r(coef)
    for s in range(3):
        sc = _rms_scalars(s, momentum)
        ops.rmsprop_step(dp, _d(grads[s]), dsq, dbuf if (momentum > 0 or s == 1) else None, dwd, sc['lr'], ALPHA, EPS, sc['momentum'], clip=_clip2(coef),
                         lr_bias=sc['lr_bias'])
        p, sq, buf = ref_rmsprop(p, grads[s], sq, buf, wd, sc['lr'], sc['lr_bias'], ALPHA, EPS, sc['momentum'], c)
        what = f'rmsprop n={n} {start} mom={momentum} step {s}'
        for name, got, r, t in (('sq', dsq, sq, ref[s][2]), ('p', dp, p, ref[s][0])):
            _check(got, r, F32, f'{what} {name} vs restatement')
            _check(got, t, F32, f'{what} {name} vs torch f64')
        if momentum > 0:
            _check(dbuf, buf, F32, what + ' buf vs restatement')
            _check(dbuf, ref[s][1], F32, what + ' buf vs torch f64')
        else:
            _exact(dbuf, buf0.cpu(), what + ' buf untouched')


@gpu
@pytest.mark.parametrize('with_ema', [True, False], ids=['ema', 'noema'])
@pytest.mark.parametrize('kind,variant', [('adam', 0), ('adam', 1), ('rmsprop', 0.0), ('rmsprop', 0.9)], ids=['adam', 'adamw', 'rmsprop', 'rmsprop-mom'])
@pytest.mark.parametrize('n_param', [257, 8192 * 256 + 7], ids=['257(%4=1)', '2097159(%4=3)'])
def test_ema_step_dev_forms(n_param, kind, variant, with_ema):
    """mgdt_adam_ema_step_dev / mgdt_rmsprop_ema_step_dev over three steps with `hyper` rewritten on the device between them and the clip
    coefficient present, absent, present: bit-equal to the eager kernel followed by mgdt_ema_update; p, moments and EMA against float64; the
    1000-element tail [n_param, n_total) keeps its p bit for bit and receives EMA only; ema = NULL still matches.  n_param % 4 is 1 and 3,
    so the quad that straddles n_param is cut both ways."""
    from mgdt_yolo_amd import ops
    n_total = n_param + 1000
    gen = _gen('optim-dev', n_param, kind, variant, with_ema)
    data, ema, wd = _rand(gen, n_total), _rand(gen, n_total), _wd(n_param)
    m, v = _rand(gen, n_param, scale=0.3), ((0.05 + _rand(gen, n_param).abs()) ** 2).float().double()
    d_data, d_m, d_v, d_ema, d_wd = _d(data), _d(m), _d(v), _d(ema) if with_ema else None, _d(wd)
    s_data, s_m, s_v, s_ema = d_data.clone(), d_m.clone(), d_v.clone(), _d(ema)                  # the two-kernel chain on the same inputs
    hyper = torch.zeros(ops.OPT_HYPER_LEN, dtype=F32, device=DEV)
    tail0 = data[n_param:].clone()
    for s in range(3):
        g = _grad(gen, n_param)
        dec = (0.0, 0.5, 0.9999)[s]
        coef = None if s == 1 else 0.37
        c = 1.0 if coef is None else f32r(coef)
        if kind == 'adam':
            sc = _adam_scalars(s, 'random')
            hyper.copy_(torch.tensor(ops.adam_hyper(sc['lr'], sc['lr_bias'], sc['beta1'], sc['beta2'], sc['step'], dec), dtype=F32))
            ops.adam_ema_step_dev(d_data[:n_param], _d(g), d_m, d_v, d_wd, d_ema, d_data, hyper, sc['beta2'], EPS, variant, clip=_clip2(coef))
            ops.adam_step(s_data[:n_param], _d(g), s_m, s_v, d_wd, sc['lr'], sc['beta1'], sc['beta2'], EPS, sc['step'], variant, clip=_clip2(coef),
                          lr_bias=sc['lr_bias'])
            pn, m, v = ref_adam(data[:n_param], g, m, v, wd, sc['lr'], sc['lr_bias'], sc['beta1'], sc['beta2'], EPS, sc['step'], variant, c)
        else:
            sc = _rms_scalars(s, variant)
            mom = sc['momentum'] if variant > 0 else 0.0
            hyper.copy_(torch.tensor(ops.rmsprop_hyper(sc['lr'], sc['lr_bias'], mom, dec), dtype=F32))
            ops.rmsprop_ema_step_dev(d_data[:n_param], _d(g), d_v, d_m, d_wd, d_ema, d_data, hyper, ALPHA, EPS, mom > 0, clip=_clip2(coef))
            ops.rmsprop_step(s_data[:n_param], _d(g), s_v, s_m, d_wd, sc['lr'], ALPHA, EPS, mom, clip=_clip2(coef), lr_bias=sc['lr_bias'])
            pn, v, m = ref_rmsprop(data[:n_param], g, v, m, wd, sc['lr'], sc['lr_bias'], ALPHA, EPS, mom, c)
        if with_ema:
            ops.ema_update(s_ema, s_data, dec)
        data = torch.cat([pn, data[n_param:]])
        ema = ref_ema(ema, data, dec)
        what = f'{kind} {variant} n={n_param} step {s}'
        _check(d_m, m, F32, what + ' m')
        _check(d_v, v, F32, what + ' v')
        _check(d_data, data, F32, what + ' p')
        _exact(d_data[n_param:], tail0, what + ' tail of p')
        _exact(d_data, s_data.cpu(), what + ' p vs eager')
        _exact(d_m, s_m.cpu(), what + ' m vs eager')
        _exact(d_v, s_v.cpu(), what + ' v vs eager')
        if with_ema:
            _check(d_ema, ema, F32, what + ' ema')
            _exact(d_ema, s_ema.cpu(), what + ' ema vs ema_update')


# ------------------------------------------------------------------------------------------------ GPU: trainer
def _gpu_model(nc=4):
    return _cpu_model(nc).to(DEV)


def _sampled(tr, flat):
    return OI.sample_flat([flat[off:off + k] for off, k in tr.state.offsets.values()])


@gpu
@pytest.mark.parametrize('tag', list(OI.TRAJ))
def test_trainer_follows_the_reference_trajectory(golden, tag):
    """warmup() + optimizer_step() on the regenerated seeded gradients against what the reference's build_optimizer('auto' -> AdamW / 'RMSProp'
    / 'Adam') + warm-up lines + clip_grad_norm_(10) + optimizer.step() + ModelEMA.update left: sampled parameters, EMA and optimizer state."""
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    g = golden('optim_traj')
    name, iterations, n_it, snaps = OI.TRAJ[tag]
    A = OI.TRAJ_ARGS
    tr = DetectionTrainer(_gpu_model(A['nc']), optimizer=name, iterations=iterations, batch_size=A['batch'], nb=A['nb'])
    st = tr.state
    assert list(st.offsets) == str(g[f'{tag}_names']).split('\n')
    for it in range(n_it):
        st.grad.copy_(OI.traj_grad(tag, it, st.n_param))
        tr.warmup(0)
        tr.optimizer_step()
        tr.ni += 1
        if it + 1 in snaps:
            _check(_sampled(tr, st.data), torch.from_numpy(g[f'{tag}_p_{it + 1}']).double(), F32, f'{tag} p after {it + 1}')
            _check(_sampled(tr, st.ema), torch.from_numpy(g[f'{tag}_ema_{it + 1}']).double(), F32, f'{tag} ema after {it + 1}')
    assert list(g[f'{tag}_state_step']) == [float(n_it)] and st.steps == n_it
    for key, buf in (('exp_avg', st.momentum_buf), ('momentum_buffer', st.momentum_buf), ('exp_avg_sq', st.second_moment), ('square_avg', st.second_moment)):
        if f'{tag}_state_{key}' in g.files:
            _check(_sampled(tr, buf), torch.from_numpy(g[f'{tag}_state_{key}']).double(), F32, f'{tag} {key}')
    sd = tr.optimizer_state_dict()
    assert len(sd['state']) == len(st.offsets) and float(sd['state'][0]['step']) == n_it


@gpu
@pytest.mark.parametrize('amp,split', [(False, False), (True, False), (False, True), (True, True)], ids=['f32', 'bf16', 'f32-two-graphs', 'bf16-two-graphs'])
@pytest.mark.parametrize('optimizer', ['AdamW', 'RMSProp'])
def test_captured_step_equals_the_eager_step(optimizer, amp, split):
    """The model, shapes and nine steps of test_captured_training_step_equals_the_eager_step with Adam's / RMSProp's kernels in the captured
    step: losses, parameters, both moment buffers and EMA bit-equal to the eager trainer over replays of two graphs during the warm-up, i.e.
    the bias corrections, learning rates and (RMSProp) momentum written into `hyper` advance between replays of one graph."""
    from mgdt_yolo_amd.seeding import seeded_labels
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    nc, B, S = 4, 4, 96
    batches = []
    for r, (lo, hi) in enumerate([(2, 4), (17, 30), (3, 9)]):
        lab = seeded_labels(B, nc, seed=10 + r, max_boxes=hi, min_boxes=lo)
        lab['bboxes'][:, 2:] = lab['bboxes'][:, 2:] * 0.5 + 0.1
        batches.append(dict(img=(seeded_images(B, S, S, seed=20 + r) * 255).to(torch.uint8), **lab))
    res = {}
    for graph in (False, True):
        tr = DetectionTrainer(_gpu_model(nc), lr0=0.002, amp=amp, graph=graph, graph_split=split, batch_size=64, nb=10, epochs=3, warmup_bias_lr=0.01,
                              optimizer=optimizer)
        losses, lrs = [], []
        for i in range(9):
            losses.append(tr.step(batches[i % 3])[0].item())
            lrs.append((tr.lr, tr.mom))
        st = tr.state
        res[graph] = (losses, st.data.clone(), st.ema.clone(), st.momentum_buf.clone(), st.second_moment.clone(), st.steps)
        if graph:
            assert sorted(tr._graphs) == [16, 32] and all(len(gs) == (2 if split else 1) for gs, _, _ in tr._graphs.values())
            assert len(set(lrs)) == 9, 'the warm-up must move the scalars every step'
    (l0, w0, e0, m0, v0, s0), (l1, w1, e1, m1, v1, s1) = res[False], res[True]
    assert s0 == s1 == 9 and all(np.isfinite(l0))
    assert l0 == l1, (l0, l1)
    assert torch.equal(w0, w1) and torch.equal(e0, e1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert v0.abs().sum().item() > 0 and m0.abs().sum().item() > 0


@gpu
def test_packed_weight_caches_follow_an_adamw_step():
    """As test_packed_weight_caches_follow_the_hip_optimizer: the AdamW kernel moves the parameters behind torch's back; an eval forward after
    it equals a forward of a model rebuilt from the stepped weights."""
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.seeding import seeded_labels
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    cfg = get_config('mspa_c2f_gd_yolov8', 'n', 80)
    m = seed_state_dict_(DetectionModel(cfg, verbose=False), 0).to(DEV)
    tr = DetectionTrainer(m, lr0=0.01, optimizer='AdamW')
    batch = seeded_labels(2, 80, seed=1)
    batch['img'] = (seeded_images(2, 96, 96, seed=2) * 255).round().to(torch.uint8)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    x = seeded_images(2, 96, 96, seed=5).to(DEV)
    m.eval()
    with torch.no_grad():
        y0 = m(x)[0].clone()
    m.train()
    for _ in range(2):
        tr.step(batch)
    m.eval()
    fresh = DetectionModel(cfg, verbose=False).to(DEV)
    fresh.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    fresh.eval()
    with torch.no_grad():
        y1, y2 = m(x)[0], fresh(x)[0]
    assert not torch.equal(y0, y1), 'two AdamW steps at lr 0.01 must change the output'
    assert torch.equal(y1, y2)


@gpu
def test_loss_falls_under_adamw():
    """One fixed batch, 20 AdamW steps at the shape of test_optimizer_step_matches_torch_sgd_and_loss_decreases (nc 4, B 4, 64 x 64)."""
    from mgdt_yolo_amd.seeding import seeded_labels
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    nc, B, S = 4, 4, 64
    tr = DetectionTrainer(_gpu_model(nc), optimizer='AdamW')
    batch = dict(img=(seeded_images(B, S, S, seed=2) * 255).to(torch.uint8), **seeded_labels(B, nc, seed=6, max_boxes=4, min_boxes=2))
    batch['bboxes'][:, 2:] = batch['bboxes'][:, 2:] * 0.5 + 0.1
    losses = [tr.step(batch)[0].item() for _ in range(20)]
    print('losses', [round(v, 2) for v in losses])
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    assert tr.state.steps == 20
