"""The normalisation kernels on ill-conditioned data: a ladder of R = |mean| / std per normalisation set (channel for BatchNorm, (image, group) for
GroupNorm, pixel for LayerNorm), each rung against float64 torch on the CPU.  GPU cases need a real MI355X (-m gpu); the two tests at the top run on
the host and come first.

Rungs.  fp32: R = 8 (the anchor: what every other statistics test draws), 64, 512, 4096, -512, and a near-constant map (mean 1, std 2^-10: variance
below eps).  bf16: R = 8, 64 and the near-constant map; at R = 64 the bf16 spacing is 0.5 x std and a host assertion checks that the rounded data
keep 0.9 of the intended std.  Every rung of a case shifts the same N(0, 1) draw; inputs are representable in the kernel's dtype.
GRN has no mean: its ladder is the magnitude of the input (x 2^-20, 1, 2^20).

Bounds come from the reference alone (kernel_ref.cond_bounds): an fp32 output - every fp32 statistic and parameter gradient of a bf16 run included -
must be within  relative L2 <= max(2e-5, 8 x d32)  and  largest element <= max(1e-4 x max|ref|, 8 x d32_max),  d32 / d32_max the distance of the same
torch functional run in float32 on the CPU to its float64 run.  At R = 8 that is kernel_ref._close.  bf16 outputs keep _close's bf16 bound.

What the ladder is there to catch is a one-pass variance E[x^2] - mean^2 formed from fp32 sums: it loses R^2 of 2^-24.  test_ladder_sees_the_one_pass_form
keeps that arithmetic as numpy code and requires the ladder to reject it.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_ref import BF16, DEV, F32, _check, _close_allow, _gen, _nhwc, _q, cond_bounds, cond_check, cnx_allowance, cnx_deltas, cond_use, ladder_map, ref_cnx_block, ref_dwconv7_ln, ref_grn_scale

gpu = pytest.mark.gpu
F64 = torch.float64
ACTS = {'silu': F.silu, 'none': lambda t: t}
RUNGS = {F32: [8, 64, 512, 4096, -512, 'const'], BF16: [8, 64, 'const']}
UP = [8, 64, 512, 4096]                                    # the rungs over which a bound must not shrink


def _dt_id(dt):
    return 'f32' if dt == F32 else 'bf16'


def _act_code(name):
    from mgdt_yolo_amd import ops
    return {'silu': ops.ACT_SILU, 'none': ops.ACT_NONE}[name]


def _rung_params(cases):
    return [pytest.param(c, R, dt, id=f'{c[0]}-R{R}-{_dt_id(dt)}') for c in cases for dt in (F32, BF16) for R in RUNGS[dt]]


def _f32(t):
    return t.float().to(DEV)


def _params(key, C):
    gen = _gen('cond-params', *key, C)
    gamma = (torch.rand(C, generator=gen, dtype=F64) + 0.5).float().double()
    beta = (torch.randn(C, generator=gen, dtype=F64) * 0.3).float().double()
    return gamma, beta


# ------------------------------------------------------------------------------------------------ cases (the smallest per route the suite already has)
# BatchNorm: (route id, B, C, H, W, act, channel offset) - BN_CASES of test_reverse_kernels.py
BN_CASES = [('bnf_v4-c16', 2, 16, 10, 12, 'silu', 0), ('scalar-c6', 2, 6, 9, 11, 'silu', 0), ('scalar-slice', 2, 16, 10, 12, 'silu', 2),
            ('bnf_v4-npix8320-80splits', 2, 4, 64, 65, 'silu', 0)]
BN_EPS, BN_MOM = 1e-3, 0.1
# GroupNorm: (id, B, C, H, W, groups, act)
GN_CASES = [('c64-g16', 2, 64, 6, 5, 16, 'silu'), ('c320-second-trip', 3, 320, 5, 6, 16, 'silu'), ('c16-one-channel-per-group', 2, 16, 5, 3, 16, 'none'),
            ('c32-g1', 2, 32, 9, 7, 1, 'none')]
GN_EPS = 1e-5
# dwconv7_ln: (id, C, B, H, W) - one per dwconv7_ln_route family of test_cnx_kernels.py (fp32 / bf16: row8 / row8, generic / row10, generic / generic)
LN_CASES = [('row8-c32', 32, 2, 13, 11), ('generic-row10-c100', 100, 2, 13, 11), ('generic-c104', 104, 2, 9, 7)]
LN_EPS = 1e-6
# dwconv7_ln_bwd: (id, B, C, H, W, channel offset) - the vector and the scalar route of test_reverse_kernels.py
LNB_CASES = [('vec_nq1-c8', 2, 8, 7, 5, 0), ('scalar-slice', 2, 32, 7, 5, 2)]


# ------------------------------------------------------------------------------------------------ torch functionals, run in float64 and in float32
def bn_torch(y, gz, gamma, beta, rm0, rv0, act, ev):
    yr, ga, be = (t.to(ev).clone().requires_grad_(True) for t in (y, gamma, beta))
    rm, rv = rm0.to(ev).clone(), rv0.to(ev).clone()
    z = ACTS[act](F.batch_norm(yr, rm, rv, ga, be, True, BN_MOM, BN_EPS))
    z.backward(gz.to(ev))
    yy = y.to(ev)
    return dict(mean=yy.mean((0, 2, 3)), rstd=1.0 / torch.sqrt(yy.var((0, 2, 3), unbiased=False) + BN_EPS), running_mean=rm, running_var=rv,
                z=z.detach(), dy=yr.grad, dgamma=ga.grad, dbeta=be.grad)


def gn_torch(y, g, gamma, beta, groups, act, ev, gu_bf16):
    """gu_bf16: the one rounding the bf16 chain makes - gu = g * act'(u) is stored in the activation dtype (see test_tood_kernels.test_gn_act_bwd)."""
    yr, ga, be = (t.to(ev).clone().requires_grad_(True) for t in (y, gamma, beta))
    u = F.group_norm(yr, groups, ga, be, GN_EPS)
    ud = u.detach().requires_grad_(True)
    z = ACTS[act](ud)
    z.backward(g.to(ev))
    u.backward(ud.grad.to(BF16).to(ev) if gu_bf16 else ud.grad)
    yy = y.to(ev)
    B, C = yy.shape[:2]
    yg = yy.reshape(B, groups, -1)
    mean, rstd = yg.mean(-1), 1.0 / torch.sqrt(yg.var(-1, unbiased=False) + GN_EPS)
    rc, mc = rstd.repeat_interleave(C // groups, 1), mean.repeat_interleave(C // groups, 1)
    gam, bet = gamma.to(ev), beta.to(ev)
    return dict(y=z.detach(), A=gam[None] * rc, B=bet[None] - mc * rc * gam[None], mean=mean, rstd=rstd, dy=yr.grad, dgamma=ga.grad, dbeta=be.grad), ud.grad


def ln_torch(u, gy, lw, lb, ev):
    ur, lwr, lbr = (t.to(ev).clone().requires_grad_(True) for t in (u, lw, lb))
    y = F.layer_norm(ur.permute(0, 2, 3, 1), (u.shape[1],), lwr, lbr, LN_EPS).permute(0, 3, 1, 2)
    y.backward(gy.to(ev))
    return dict(y=y.detach(), du=ur.grad, d_ln_w=lwr.grad, d_ln_b=lbr.grad)


def grn_torch(t, g, gamma, beta, ev):
    """GRN of convnextv2.py: y = gamma * (t * Nx) + beta + t, Nx = Gx / (mean_c Gx + 1e-6), Gx = ||t||_2 over the map."""
    tr, ga, be = (a.to(ev).clone().requires_grad_(True) for a in (t, gamma, beta))
    gx = torch.sqrt((tr * tr).sum((2, 3), keepdim=True))
    nx = gx / (gx.mean(1, keepdim=True) + 1e-6)
    (ga.view(1, -1, 1, 1) * (tr * nx) + be.view(1, -1, 1, 1) + tr).backward(g.to(ev))
    return dict(dt=tr.grad, dgamma=ga.grad, dbeta=be.grad)


@functools.lru_cache(maxsize=None)
def bn_case(case, R, dt):
    cid, B, C, H, W, act, off = case
    y = ladder_map(('bn', cid), (B, C, H, W), R, dt)
    gen = _gen('cond-bn', cid)
    gz = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt)
    gamma, beta = _params(('bn', cid), C)
    rm0 = (torch.randn(C, generator=gen, dtype=F64)).float().double()
    rv0 = (torch.rand(C, generator=gen, dtype=F64) + 0.5).float().double()
    args = (y, gz, gamma, beta, rm0, rv0, act)
    return dict(y=y, gz=gz, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, r64=bn_torch(*args, F64), r32=bn_torch(*args, F32))


@functools.lru_cache(maxsize=None)
def gn_case(case, R, dt):
    cid, B, C, H, W, groups, act = case
    y = ladder_map(('gn', cid), (B, C, H, W), R, dt)
    g = _q(torch.randn(B, C, H, W, generator=_gen('cond-gn', cid), dtype=F64), dt)
    gamma, beta = _params(('gn', cid), C)
    args = (y, g, gamma, beta, groups, act)
    r64, r32 = gn_torch(*args, F64, dt == BF16)[0], gn_torch(*args, F32, dt == BF16)[0]
    return dict(y=y, g=g, gamma=gamma, beta=beta, r64=r64, r32=r32)


@functools.lru_cache(maxsize=None)
def lnb_case(case, R, dt):
    cid, B, C, H, W, off = case
    u = ladder_map(('lnb', cid), (B, C, H, W), R, dt)
    gen = _gen('cond-lnb', cid)
    gy = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt)
    lw, lb = _params(('lnb', cid), C)
    return dict(u=u, gy=gy, lw=lw, lb=lb, r64=ln_torch(u, gy, lw, lb, F64), r32=ln_torch(u, gy, lw, lb, F32))


@functools.lru_cache(maxsize=None)
def ln_case(case, R, dt):
    """dwconv7_ln on a zero-mean bf16-representable x: the depth-wise conv output has mean 0 over the channels of every pixel, so a constant added to
    every channel's conv bias is the pixel mean; it is R x the median pixel std of the conv output (fp32-rounded).  The near-constant rung shrinks the
    conv weights by 2^-10 / that std around a bias of 1."""
    cid, C, B, H, W = case
    gen = _gen('cond-ln', cid)
    x = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), BF16)
    dw = (torch.randn(C, 1, 7, 7, generator=gen) * 0.2)
    lw, lb = (torch.rand(C, generator=gen) + 0.5), torch.randn(C, generator=gen) * 0.1
    std = F.conv2d(x, dw.double(), None, 1, 3, 1, C).std(1, unbiased=False).median().item()
    if R == 'const':
        dw, dwb = (dw * (2.0 ** -10 / std)).float(), torch.ones(C)
    else:
        dwb = torch.full((C,), R * std).float()
    args = (x, dw, dwb, lw, lb, LN_EPS)
    (y64, u64), (y32, u32) = ref_dwconv7_ln(*args, dt=F64), ref_dwconv7_ln(*args, dt=F32)
    ratio = (u64.mean(1).abs() / u64.std(1, unbiased=False)).median().item()
    return dict(x=x, dw=dw, dwb=dwb, lw=lw, lb=lb, y64=y64, u64=u64, y32=y32, u32=u32, ratio=ratio)


@functools.lru_cache(maxsize=None)
def addln_case(R, dt):
    """add_layernorm over 8 rows of 256: x carries the mean (fp32 or bf16 values), the fp32 residual is N(0, 1/4) (2^-11 x N(0, 1) on the near-constant rung)."""
    x = ladder_map(('addln',), (1, 1, 8, 256), R, dt).reshape(8, 256)
    gen = _gen('cond-addln')
    res = (torch.randn(8, 256, generator=gen, dtype=F64) * (2.0 ** -11 if R == 'const' else 0.5)).float().double()
    gamma, beta = _params(('addln',), 256)
    fn = lambda ev: F.layer_norm(x.to(ev) + res.to(ev), (256,), gamma.to(ev), beta.to(ev), 1e-5)
    return dict(x=x, res=res, gamma=gamma, beta=beta, r64=dict(out=fn(F64)), r32=dict(out=fn(F32)))


GRN_MAGS = [-20, 0, 20]


@functools.lru_cache(maxsize=None)
def grn_case(mag, dt):
    """t x 2^mag on GRN_CASES 'c64-HW117' of test_cnx_kernels.py: a power of two keeps t representable."""
    B, C, H, W = 2, 64, 13, 9
    gen = _gen('cond-grn')
    t = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64) * 0.7 + 0.2, dt) * 2.0 ** mag
    g = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt)
    gamma = (torch.randn(C, generator=gen, dtype=F64) * 0.5).float().double()
    beta = torch.randn(C, generator=gen, dtype=F64).float().double()
    r64, r32 = grn_torch(t, g, gamma, beta, F64), grn_torch(t, g, gamma, beta, F32)
    r64['scale'], r32['scale'] = ref_grn_scale(t, gamma, F64), ref_grn_scale(t, gamma, F32)
    return dict(t=t, g=g, gamma=gamma, beta=beta, r64=r64, r32=r32)


def _cases_fp32():
    """(name, rung -> {quantity: (float64, float32)}) for every fp32 case of the ladder."""
    out = []
    for c in BN_CASES:
        out.append((f'bn-{c[0]}', {R: bn_case(c, R, F32) for R in RUNGS[F32]}))
    for c in GN_CASES:
        out.append((f'gn-{c[0]}', {R: gn_case(c, R, F32) for R in RUNGS[F32]}))
    for c in LNB_CASES:
        out.append((f'lnb-{c[0]}', {R: lnb_case(c, R, F32) for R in RUNGS[F32]}))
    for c in LN_CASES:
        out.append((f'ln-{c[0]}', {R: (lambda k: dict(r64=dict(y=k['y64']), r32=dict(y=k['y32'])))(ln_case(c, R, F32)) for R in RUNGS[F32]}))
    out.append(('add_layernorm', {R: addln_case(R, F32) for R in RUNGS[F32]}))
    return out


# ------------------------------------------------------------------------------------------------ host tests
def test_bounds_are_finite_and_ordered():
    """For every fp32 case and output - BatchNorm, GroupNorm, dwconv7_ln, dwconv7_ln_bwd, add_layernorm on the ladder; GRN and the two module cases on
    their own rungs - the bound comes from torch alone and is finite, and torch's own float32 run uses at most 1/8 of it.  On the ladder it does not
    shrink from one rung to the next of 8, 64, 512, 4096 (the largest-element bound up to 1e-3 of itself: its floor 1e-4 x max|ref| moves with the
    last bits of the shifted draw).  bf16: the rounded R = 64 data keep 0.9 of the intended std."""
    for name, rungs in _cases_fp32():
        for q in rungs[8]['r64']:
            prev = (0.0, 0.0)
            for R in RUNGS[F32]:
                r64, r32 = rungs[R]['r64'][q], rungs[R]['r32'][q]
                assert r64.dtype == F64 and r32.dtype == F32, (name, q, R)
                assert torch.isfinite(r64).all() and torch.isfinite(r32).all(), (name, q, R, 'non-finite reference')
                b = cond_bounds(r64, r32)
                assert all(np.isfinite(b)) and b[0] >= 2e-5 and b[1] > 0, (name, q, R, b)
                assert cond_use(r32, r64, r32) <= 0.125 + 1e-12, (name, q, R, 'torch float32 above 1/8 of the bound')
                if R in UP:
                    assert b[0] >= prev[0] and b[1] >= prev[1] * (1 - 1e-3), (name, q, R, 'bound shrank', prev, b)
                    prev = b
    for c in LN_CASES:                                                        # the conv bias really sets the pixel ratio
        for R in RUNGS[F32][:5]:
            ratio = ln_case(c, R, F32)['ratio']
            assert 0.8 * abs(R) < ratio < 1.25 * abs(R), (c[0], R, 'pixel mean / std', ratio)
    # GRN (a magnitude ladder: no R to order by) and the two module cases (one rung): finite references and bounds, torch float32 within 1/8
    single = [(f'grn-x2^{mag}', grn_case(mag, F32)) for mag in GRN_MAGS] + [('Conv conv1', conv_module_case()), ('Conv_GN', conv_gn_module_case())]
    for name, k in single:
        for q, r64 in k['r64'].items():
            r32 = k['r32'][q]
            assert r64.dtype == F64 and r32.dtype == F32, (name, q)
            assert torch.isfinite(r64).all() and torch.isfinite(r32).all(), (name, q, 'non-finite reference')
            b = cond_bounds(r64, r32)
            assert all(np.isfinite(b)) and b[0] >= 2e-5 and b[1] > 0, (name, q, b)
            assert cond_use(r32, r64, r32) <= 0.125 + 1e-12, (name, q, 'torch float32 above 1/8 of the bound')
    for cases, maker, key in ((BN_CASES, bn_case, 'y'), (GN_CASES, gn_case, 'y'), (LNB_CASES, lnb_case, 'u')):
        for c in cases:
            for R in (8, 64):
                std = maker(c, R, BF16)[key].std().item()
                assert std >= 0.9, (c[0], R, 'bf16 rounding left std', std)


# ---- the arithmetic the ladder must catch, as the kernels had it: fp32 partial sums of x and x * x (serial, in the kernels' pixel order), the
# subtraction afterwards.  numpy float32 throughout; np.cumsum keeps the serial association.
f32 = np.float32


def _ssum(a, axis=-1):
    return np.take(np.cumsum(a.astype(f32), axis=axis, dtype=f32), -1, axis=axis)


def one_pass_gn(x, gu, gamma, beta, G, eps):
    """GroupNorm forward (y = x * A + B) and backward (dy = gu * P + x * Q + R, dgamma) with the statistics var = max(E[x^2] - mean^2, 0) and the
    projection S2 - mean * S1 formed from fp32 sums per (image, channel)."""
    B, C, H, W = x.shape
    cg, cnt = C // G, f32(C // G * H * W)
    xf, gf = x.reshape(B, C, -1).astype(f32), gu.reshape(B, C, -1).astype(f32)
    s, ss = _ssum(xf), _ssum(xf * xf)
    a, b = _ssum(s.reshape(B, G, cg)), _ssum(ss.reshape(B, G, cg))
    mean = a / cnt
    var = np.maximum(b / cnt - mean * mean, f32(0))
    rstd = f32(1) / np.sqrt(var + f32(eps))
    m, r = np.repeat(mean, cg, 1), np.repeat(rstd, cg, 1)
    A = gamma.astype(f32)[None] * r
    Bc = beta.astype(f32)[None] - m * A
    y = xf * A[..., None] + Bc[..., None]
    s1, s2 = _ssum(gf), _ssum(gf * xf)
    proj = r * (s2 - m * s1)
    M1 = np.repeat(_ssum((gamma.astype(f32)[None] * s1).reshape(B, G, cg)) / cnt, cg, 1)
    M2 = np.repeat(_ssum((gamma.astype(f32)[None] * proj).reshape(B, G, cg)) / cnt, cg, 1)
    P, Q, Rr = A, -r * r * M2, -r * M1 + m * r * r * M2
    dy = gf * P[..., None] + xf * Q[..., None] + Rr[..., None]
    return y.reshape(x.shape), dy.reshape(x.shape), _ssum(proj, 0)


def one_pass_bn_rstd(x, eps, per_thread=1):
    """BatchNorm statistics as bnf_reduce and the scalar kernel had them: every thread adds x and the fp32 product x * x of its pixels in fp32, the
    threads' sums are added in double, then mean, var = E[x^2] - mean^2 and rstd in double.  On this file's maps every thread holds ONE pixel (at least
    64 splits x 256 / (C / 4) pixel lanes, 512 splits in the scalar kernel), so per_thread = 1: the rounding of x * x alone is what is left of the form."""
    C = x.shape[1]
    xf = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(C, -1).astype(f32)
    n = xf.shape[1]
    pad = -n % per_thread
    xp = np.concatenate([xf, np.zeros((C, pad), f32)], 1).reshape(C, -1, per_thread)
    s, ss = _ssum(xp).astype(np.float64).sum(-1), _ssum(xp * xp).astype(np.float64).sum(-1)
    m = s / n
    return 1.0 / np.sqrt(np.maximum(ss / n - m * m, 0.0) + eps)


GN_FROM, BN_FROM = 64, 512                                 # the first rung at which the one-pass form must be at least 2 x over the bound


def one_pass_factors():
    """{(kind, rung): bound use of the one-pass form} on the first GroupNorm case (activation 'none', so gu = g) and the many-splits BatchNorm case."""
    out = {}
    cid, B, C, H, W, groups, _ = GN_CASES[0]
    for R in RUNGS[F32][:5]:
        y = ladder_map(('gn', cid), (B, C, H, W), R, F32)
        g = torch.randn(B, C, H, W, generator=_gen('cond-gn', cid), dtype=F64).float().double()
        gamma, beta = _params(('gn', cid), C)
        r64, r32 = (gn_torch(y, g, gamma, beta, groups, 'none', ev, False)[0] for ev in (F64, F32))
        yy, dy, dgam = one_pass_gn(y.numpy(), g.numpy(), gamma.numpy(), beta.numpy(), groups, GN_EPS)
        for q, got in (('y', yy), ('dy', dy), ('dgamma', dgam)):
            out['gn-' + q, R] = cond_use(torch.from_numpy(got.astype(np.float64)), r64[q], r32[q])
        for i in (0, 3):
            k = bn_case(BN_CASES[i], R, F32)
            out[f'bn-rstd-{BN_CASES[i][0]}', R] = cond_use(torch.from_numpy(one_pass_bn_rstd(k['y'].numpy(), BN_EPS)), k['r64']['rstd'], k['r32']['rstd'])
    return out


def test_ladder_sees_the_one_pass_form():
    """The one-pass arithmetic above must leave the ladder's bound by at least 2 x: GroupNorm's y, dy and dgamma from R = 64 on, BatchNorm's rstd from
    R = 512 on; at the anchor R = 8 it passes (which is why the suite never saw it).  Share of the bound it uses, on this file's first GroupNorm case
    (without the activation) and the 240- and 8320-pixel BatchNorm cases, measured on the host:
                               R = 8     64      512     4096     -512
      GroupNorm y              0.19     6.6     245    1.7e5      192
      GroupNorm dy             0.20    13.0     334    4.2e9      409
      GroupNorm dgamma         0.18     4.3      63    7.1e4       35
      BatchNorm rstd, 240 px   0.00    0.20    11.2    2.5e3     10.2
      BatchNorm rstd, 8320 px  0.00    0.03     5.1    2.3e3      5.1
    (the parent commit's kernels, run once under this file on an MI355X, used 6.7 / 158 / 1.6e5 of the bound on GroupNorm y and 11.2 / 2.5e3 on the 240-pixel
    BatchNorm rstd at the same rungs: the restatement is the kernels' arithmetic)."""
    fac = one_pass_factors()
    for (q, R), v in sorted(fac.items(), key=str):
        print(f'one-pass {q} at R = {R}: {v:.2f} of the bound')
    for (q, R), v in fac.items():
        assert np.isfinite(v)
        if R == 8:
            assert v <= 1.0, (q, R, v, 'the anchor rung rejects the one-pass form: it is no longer the range the other tests cover')
        elif abs(R) >= (GN_FROM if q.startswith('gn') else BN_FROM):
            assert v >= 2.0, (q, R, v, 'the ladder does not see the one-pass form at this rung')


# ------------------------------------------------------------------------------------------------ GPU: BatchNorm
@gpu
@pytest.mark.parametrize('case,R,dt', _rung_params(BN_CASES))
def test_bn_ladder(case, R, dt):
    """bn_stats (mean, rstd, running_mean, running_var), bn_act (z) and bn_act_bwd (dy, dgamma, dbeta), the last two fed the device's own mean / rstd
    as Conv.train_fwd / backward do."""
    from mgdt_yolo_amd import ops
    cid, B, C, H, W, act, off = case
    k = bn_case(case, R, dt)
    r64, r32 = k['r64'], k['r32']
    gen = _gen('cond-bn-buf', cid)
    yd, _ = _nhwc(k['y'], dt, off, 8 if off else 0, gen=gen)
    gzd, _ = _nhwc(k['gz'], dt, off, 8 if off else 0, gen=gen)
    rm, rv = _f32(k['rm0']), _f32(k['rv0'])
    mean, rstd = ops.bn_stats(yd, BN_EPS, BN_MOM, rm, rv)
    for q, got in (('mean', mean), ('rstd', rstd), ('running_mean', rm), ('running_var', rv)):
        cond_check(got, r64[q], r32[q], F32, f'bn_stats {q} {cid} R{R}')
    ga, be = _f32(k['gamma']), _f32(k['beta'])
    z = ops.bn_act(yd, mean, rstd, ga, be, _act_code(act))
    assert z.dtype == dt
    cond_check(z, r64['z'], r32['z'], dt, f'bn_act z {cid} R{R}')
    dgamma, dbeta = torch.full((C,), float('nan'), device=DEV), torch.full((C,), float('nan'), device=DEV)
    dy = ops.bn_act_bwd(gzd, yd, mean, rstd, ga, be, _act_code(act), dgamma, dbeta)
    cond_check(dy, r64['dy'], r32['dy'], dt, f'bn_act_bwd dy {cid} R{R}')
    cond_check(dgamma, r64['dgamma'], r32['dgamma'], F32, f'bn_act_bwd dgamma {cid} R{R}')
    cond_check(dbeta, r64['dbeta'], r32['dbeta'], F32, f'bn_act_bwd dbeta {cid} R{R}')


# ------------------------------------------------------------------------------------------------ GPU: GroupNorm
@gpu
@pytest.mark.parametrize('case,R,dt', _rung_params(GN_CASES))
def test_gn_ladder(case, R, dt):
    """groupnorm (y), gn_affine (A, B, mean, rstd) and gn_act_bwd (dy, dgamma, dbeta; written over NaN, then accumulated onto pre-loaded values).
    The bf16 dy is held to _close's plain bf16 bound on every rung.  The chain stores gu = g * act'(u) as bf16, and each element whose rounding falls
    the other way than the float64 reference's moves its dy by gamma * rstd bf16 steps: with u = y * A + B from fp32 A, B the 320-channel near-constant
    map used 1.16 of that bound on an MI355X (torch's own float32 run, rounded the same way, uses 1.005 of it on the 320-channel map at R = 64);
    with u formed in double (mgdt_gn_act_grad) it uses 0.63, and no bf16 rung more than 0.71."""
    from mgdt_yolo_amd import ops
    cid, B, C, H, W, groups, act = case
    k = gn_case(case, R, dt)
    r64, r32 = k['r64'], k['r32']
    yd, gd = _nhwc(k['y'], dt)[0], _nhwc(k['g'], dt)[0]
    ga, be = _f32(k['gamma']), _f32(k['beta'])
    out = ops.groupnorm(yd, ga, be, groups, GN_EPS, _act_code(act))
    assert out.dtype == dt
    cond_check(out, r64['y'], r32['y'], dt, f'groupnorm y {cid} R{R}')
    for q, got in zip(('A', 'B', 'mean', 'rstd'), ops.gn_affine(yd, ga, be, groups, GN_EPS)):
        cond_check(got, r64[q], r32[q], F32, f'gn_affine {q} {cid} R{R}')
    for accumulate in (False, True):
        gen = _gen('cond-gn-acc', cid)
        dg0 = torch.randn(C, generator=gen, dtype=F64).float().double() if accumulate else torch.full((C,), float('nan'), dtype=F64)
        db0 = torch.randn(C, generator=gen, dtype=F64).float().double() if accumulate else torch.full((C,), float('nan'), dtype=F64)
        dgamma, dbeta = _f32(dg0), _f32(db0)
        dy = ops.gn_act_bwd(gd, yd, ga, be, groups, GN_EPS, _act_code(act), dgamma, dbeta, accumulate)
        mode = 'accumulate' if accumulate else 'write'
        add = (lambda r, o: r + o.to(r.dtype)) if accumulate else (lambda r, o: r)
        cond_check(dy, r64['dy'], r32['dy'], dt, f'gn_act_bwd dy {mode} {cid} R{R}')
        cond_check(dgamma, add(r64['dgamma'], dg0), add(r32['dgamma'], dg0), F32, f'gn_act_bwd dgamma {mode} {cid} R{R}')
        cond_check(dbeta, add(r64['dbeta'], db0), add(r32['dbeta'], db0), F32, f'gn_act_bwd dbeta {mode} {cid} R{R}')


# ------------------------------------------------------------------------------------------------ GPU: LayerNorm routes (these subtract the mean first)
@gpu
@pytest.mark.parametrize('case,R,dt', _rung_params(LN_CASES))
def test_dwconv7_ln_ladder(case, R, dt):
    """dwconv7_ln and dwconv7_ln_train: y against ref_dwconv7_ln in float64, the bound from its float32 run."""
    from mgdt_yolo_amd import ops
    cid, C, B, H, W = case
    k = ln_case(case, R, dt)
    xv = _nhwc(k['x'], dt)[0]
    args = (k['dw'].reshape(C, 49).t().contiguous().to(DEV), k['dwb'].to(DEV), k['lw'].to(DEV), k['lb'].to(DEV), LN_EPS)
    print(f'pixel |mean| / std: {k["ratio"]:.1f}, route {ops.dwconv7_ln_route(B, H, W, C, dt)["family"]}')
    cond_check(ops.dwconv7_ln(xv, *args), k['y64'], k['y32'], dt, f'dwconv7_ln y {cid} R{R}')
    y2, _ = ops.dwconv7_ln_train(xv, *args)
    cond_check(y2, k['y64'], k['y32'], dt, f'dwconv7_ln_train y {cid} R{R}')


@gpu
@pytest.mark.parametrize('case,R,dt', _rung_params(LNB_CASES))
def test_dwconv7_ln_bwd_ladder(case, R, dt):
    """dwconv7_ln_bwd on a stored u with pixel mean R x std: the LayerNorm's input gradient du (the kernel's intermediate map, reached through the C
    entry point), d_ln_w and d_ln_b against autograd of F.layer_norm.  The scalar route gets gy and x as channel slices at offset 2."""
    from mgdt_yolo_amd import _lib, ops
    cid, B, C, H, W, off = case
    k = lnb_case(case, R, dt)
    r64, r32 = k['r64'], k['r32']
    gen = _gen('cond-lnb-buf', cid)
    x = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt)
    xv, gyv = _nhwc(x, dt, off, 8 if off else 0, gen=gen)[0], _nhwc(k['gy'], dt, off, 8 if off else 0, gen=gen)[0]
    uv = _nhwc(k['u'], dt)[0]
    w49c = (torch.randn(49, C, generator=gen) / 7).to(DEV)
    d_w = torch.full((C, 1, 7, 7), float('nan'), device=DEV)
    d_b, d_lw, d_lb = (torch.full((C,), float('nan'), device=DEV) for _ in range(3))
    dx, du = ops.like(xv), ops.like(xv)
    ws = torch.empty(_lib.lib().mgdt_dwconv7_ln_bwd_workspace_bytes(C), dtype=torch.uint8, device=DEV)
    ops._launch('dwconv7_ln_bwd', 'mgdt_dwconv7_ln_bwd', ops.vp(xv), ops.vp(uv), ops.vp(gyv), ops.ptr(w49c), ops.ptr(_f32(k['lw'])), LN_EPS, ops.vp(du), ops.vp(dx), 0,
                ops.ptr(d_w), ops.ptr(d_b), ops.ptr(d_lw), ops.ptr(d_lb), ops.ptr(ws), ops.dtype_code(dt), ops.stream())
    cond_check(du, r64['du'], r32['du'], dt, f'dwconv7_ln_bwd du {cid} R{R}')
    cond_check(d_lw, r64['d_ln_w'], r32['d_ln_w'], F32, f'dwconv7_ln_bwd d_ln_w {cid} R{R}')
    cond_check(d_lb, r64['d_ln_b'], r32['d_ln_b'], F32, f'dwconv7_ln_bwd d_ln_b {cid} R{R}')


@gpu
@pytest.mark.parametrize('R,dt', [pytest.param(R, dt, id=f'R{R}-{_dt_id(dt)}') for dt in (F32, BF16) for R in RUNGS[dt]])
def test_add_layernorm_ladder(R, dt):
    """add_layernorm over 8 rows of 256: x carries the mean (fp32 or bf16 values), the fp32 residual is N(0, 1/4); the output is fp32."""
    from mgdt_yolo_amd import ops
    k = addln_case(R, dt)
    got = ops.add_layernorm(k['x'].to(dt).to(DEV), _f32(k['res']), _f32(k['gamma']), _f32(k['beta']))
    cond_check(got, k['r64']['out'], k['r32']['out'], F32, f'add_layernorm R{R} {_dt_id(dt)}')


# ------------------------------------------------------------------------------------------------ GPU: GRN (no mean: a magnitude ladder)
@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('mag', GRN_MAGS, ids=lambda m: f'x2^{m}')
def test_grn_magnitude_ladder(mag, dt):
    """grn_scale and grn_bwd (with its nc_reduce sums, as convnextv2.py calls it) on t x 2^-20, 1, 2^20: a power of two keeps t representable."""
    from mgdt_yolo_amd import ops
    k = grn_case(mag, dt)
    gamma, r64, r32 = k['gamma'], k['r64'], k['r32']
    C = gamma.numel()
    td, gd = _nhwc(k['t'], dt)[0], _nhwc(k['g'], dt)[0]
    cond_check(ops.grn_scale(td, _f32(gamma)), r64['scale'], r32['scale'], F32, f'grn_scale x2^{mag}')
    dgamma, dbeta = torch.full((C,), float('nan'), device=DEV), torch.full((C,), float('nan'), device=DEV)
    dtt = ops.grn_bwd(gd, td, ops.nc_reduce(td, td), ops.nc_reduce(gd, td), ops.nc_reduce(gd), _f32(gamma), dgamma, dbeta)
    cond_check(dtt, r64['dt'], r32['dt'], dt, f'grn_bwd dt x2^{mag}')
    cond_check(dgamma, r64['dgamma'], r32['dgamma'], F32, f'grn_bwd dgamma x2^{mag}')
    cond_check(dbeta, r64['dbeta'], r32['dbeta'], F32, f'grn_bwd dbeta x2^{mag}')


# ------------------------------------------------------------------------------------------------ GPU: saturation
# N(0, 1) values with one element in eight replaced by +-20, +-90 or +-200 (all bf16-representable): exp() of them overflows fp32 or underflows to
# zero, which is where an activation, its derivative or a softmax written without care returns inf / inf or -inf * 0.  Every output must be finite and
# within the bound its own test module states, against float64 torch.
SAT_ACTS = {'silu': F.silu, 'gelu': F.gelu, 'relu': F.relu}


def saturating(key, *shape, dt=F32):
    gen = _gen('saturating', *key, shape)
    x = torch.randn(*shape, generator=gen, dtype=F64)
    big = torch.tensor([20.0, -20.0, 90.0, -90.0, 200.0, -200.0], dtype=F64)[torch.randint(0, 6, shape, generator=gen)]
    return _q(torch.where(torch.rand(*shape, generator=gen) < 0.125, big, x), dt)


def _sat_code(name):
    from mgdt_yolo_amd import ops
    return {'silu': ops.ACT_SILU, 'gelu': ops.ACT_GELU, 'relu': ops.ACT_RELU}[name]


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('act', list(SAT_ACTS))
@pytest.mark.parametrize('route,C,off', [pytest.param('bnf_v4', 64, 0, id='bnf_v4'), pytest.param('scalar', 64, 2, id='scalar-slice')])
def test_saturation_bias_act_forward_and_backward(route, C, off, act, dt):
    """bn_act in bias-only mode (mean = None) and the matching mode of bn_act_bwd (dy, dbias) on saturating pre-activations, both routes."""
    from mgdt_yolo_amd import ops
    gen = _gen('sat-bias', C, off)
    y, gz = saturating(('bias', act), 2, C, 9, 7, dt=dt), _q(torch.randn(2, C, 9, 7, generator=gen, dtype=F64), dt)
    b = torch.randn(C, generator=gen, dtype=F64).float().double()
    yr, br = y.clone().requires_grad_(True), b.clone().requires_grad_(True)
    z = SAT_ACTS[act](yr + br[None, :, None, None])
    z.backward(gz)
    yd, gzd = _nhwc(y, dt, off, 8 if off else 0, gen=gen)[0], _nhwc(gz, dt, off, 8 if off else 0, gen=gen)[0]
    _check(ops.bn_act(yd, None, None, None, _f32(b), _sat_code(act)), z.detach(), dt, f'bn_act bias-only {act} {route}')
    db = torch.full((C,), float('nan'), device=DEV)
    dy = ops.bn_act_bwd(gzd, yd, None, None, None, _f32(b), _sat_code(act), None, db)
    _check(dy, yr.grad, dt, f'bn_act_bwd bias-only dy {act} {route}')
    _check(db, br.grad, F32, f'bn_act_bwd bias-only dbias {act} {route}')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('act', ['silu', 'gelu'])
def test_saturation_bn_act_bwd(act, dt):
    """bn_stats -> bn_act_bwd with gamma = 40: the normalised values are N(0, 1) with outliers, the pre-activations gamma * xhat + beta reach +-200."""
    from mgdt_yolo_amd import ops
    B, C, H, W = 2, 16, 10, 12
    gen = _gen('sat-bn', act)
    y, gz = saturating(('bn', act), B, C, H, W, dt=dt), _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt)
    gamma = torch.full((C,), 40.0, dtype=F64)
    beta = (torch.randn(C, generator=gen, dtype=F64) * 0.3).float().double()
    yr, ga, be = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    SAT_ACTS[act](F.batch_norm(yr, None, None, ga, be, True, 0.0, BN_EPS)).backward(gz)
    yd, gzd = _nhwc(y, dt)[0], _nhwc(gz, dt)[0]
    mean, rstd = ops.bn_stats(yd, BN_EPS, 0.0)
    dgamma, dbeta = torch.full((C,), float('nan'), device=DEV), torch.full((C,), float('nan'), device=DEV)
    dy = ops.bn_act_bwd(gzd, yd, mean, rstd, _f32(gamma), _f32(beta), _sat_code(act), dgamma, dbeta)
    _check(dy, yr.grad, dt, f'bn_act_bwd dy {act}')
    _check(dgamma, ga.grad, F32, f'bn_act_bwd dgamma {act}')
    _check(dbeta, be.grad, F32, f'bn_act_bwd dbeta {act}')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_saturation_nc_affine_act_bwd_silu(dt):
    """nc_affine_act_bwd: gu = g * silu'(y * A + B) with y saturating, A around 1 and B small."""
    from mgdt_yolo_amd import ops
    B, C, H, W = 2, 64, 6, 5
    gen = _gen('sat-ncaff')
    y, g = saturating(('ncaff',), B, C, H, W, dt=dt), _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt)
    A = (torch.rand(B, C, generator=gen, dtype=F64) + 0.5).float().double()
    Bc = (torch.randn(B, C, generator=gen, dtype=F64) * 0.3).float().double()
    u = (y * A[:, :, None, None] + Bc[:, :, None, None]).requires_grad_(True)
    F.silu(u).backward(g)
    _check(ops.nc_affine_act_bwd(_nhwc(g, dt)[0], _nhwc(y, dt)[0], _f32(A), _f32(Bc), _sat_code('silu')), u.grad, dt, 'nc_affine_act_bwd silu')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_saturation_pixel_gate(dt):
    """pixel_gate and pixel_gate_bwd with the saturating values on the logit: x * sigmoid(l), gx = g * s, glogit = s (1 - s) sum_c g x."""
    from mgdt_yolo_amd import ops
    B, C, H, W = 2, 64, 9, 7
    gen = _gen('sat-gate')
    x, g = (_q(torch.randn(B, C, H, W, generator=gen, dtype=F64), dt) for _ in range(2))
    l = saturating(('gate',), B, 1, H, W, dt=dt)
    xr, lr = x.clone().requires_grad_(True), l.clone().requires_grad_(True)
    out = xr * torch.sigmoid(lr)
    out.backward(g)
    xd, ld = _nhwc(x, dt)[0], _nhwc(l, dt)[0]
    _check(ops.pixel_gate(xd, ld), out.detach(), dt, 'pixel_gate')
    gp4 = ops.new_act(B, 4, H, W, dt, DEV).zero_()
    gx, _ = ops.pixel_gate_bwd(_nhwc(g, dt)[0], xd, ld, glogit=gp4[:, :1])
    _check(gx, xr.grad, dt, 'pixel_gate_bwd gx')
    _check(gp4[:, :1], lr.grad, dt, 'pixel_gate_bwd glogit')


@gpu
def test_saturation_cls_softmax_and_rtdetr_sigmoid():
    """cls_softmax (test_classify.py's bound: atol 1e-6, rtol 2e-5, rows summing to 1 within 1e-6) and rtdetr_sigmoid (test_rtdetr.py's fp32_bound:
    max(1e-6, 8 x the float32 CPU run's distance)) on saturating logits."""
    from mgdt_yolo_amd import ops
    lg = saturating(('softmax',), 7, 1000)
    p = ops.cls_softmax(lg.float().to(DEV)).cpu().double()
    assert torch.isfinite(p).all()
    np.testing.assert_allclose(p.sum(1).numpy(), 1.0, atol=1e-6)
    np.testing.assert_allclose(p.numpy(), torch.softmax(lg, 1).numpy(), atol=1e-6, rtol=2e-5)
    x = saturating(('sigmoid',), 2, 300, 7)
    want = torch.sigmoid(x)
    bound = max(1e-6, 8 * (torch.sigmoid(x.float()).double() - want).abs().max().item())
    got = ops.rtdetr_sigmoid(x.float().to(DEV)).cpu().double()
    d = (got - want).abs().max().item()
    print(f'rtdetr_sigmoid: max |d| {d:.3e}, bound {bound:.3e}')
    assert torch.isfinite(got).all() and d <= bound, (d, bound)


# ------------------------------------------------------------------------------------------------ GPU: two modules at R = 512, fp32
def _module_step(m, x, g):
    """forward under ops.force_ctx(), backward under ops.defer_wgrad(), as tests/test_train_modules.py runs a module's training step"""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.nn.modules.conv import HipModule
    for sub in m.modules():
        if isinstance(sub, HipModule):
            sub._cdtype = F32
    d = lambda t: t.float().to(DEV).contiguous(memory_format=torch.channels_last)
    with ops.force_ctx():
        y = m(d(x))
    with ops.defer_wgrad():
        dx = m.backward(d(g))
    return y, dx


@functools.lru_cache(maxsize=None)
def conv_module_case():
    """`conv1` of GI.MODULE_CASES (conv 1x1 -> BatchNorm -> SiLU) with a constant added to its input: the conv output of channel k has mean
    offset x sum(w[k]) and std ||w[k]||; the offset makes the median channel's ratio 512.  The module (on the host), its input, the output gradient and
    the torch functionals in float64 and float32."""
    import inputs as GI
    import mgdt_yolo_amd.nn.modules as M
    from mgdt_yolo_amd.seeding import seed_state_dict_
    cls, args, _ = GI.MODULE_CASES['conv1']
    m = getattr(M, cls)(*args)
    m.bn.eps = 1e-3
    m = seed_state_dict_(m, GI.MODULE_SEED).train()
    w = m.conv.weight.detach().double()
    ratio = (w.sum((1, 2, 3)).abs() / w.flatten(1).norm(dim=1)).median().item()
    x = (GI.module_inputs('conv1')[0].double() + 512.0 / ratio).float().double()
    g = torch.randn(x.shape[0], w.shape[0], *x.shape[2:], generator=_gen('cond-conv1'), dtype=F64).float().double()
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items()}

    def run(ev):
        xr, wr, ga, be = (t.to(ev).clone().requires_grad_(True) for t in (x, sd['conv.weight'], sd['bn.weight'], sd['bn.bias']))
        rm, rv = sd['bn.running_mean'].to(ev).clone(), sd['bn.running_var'].to(ev).clone()
        c = F.conv2d(xr, wr)
        y = F.silu(F.batch_norm(c, rm, rv, ga, be, True, m.bn.momentum, m.bn.eps))
        y.backward(g.to(ev))
        r = (c.detach().mean((0, 2, 3)).abs() / c.detach().std((0, 2, 3))).median().item()
        return {'y': y.detach(), 'dx': xr.grad, 'g:conv.weight': wr.grad, 'g:bn.weight': ga.grad, 'g:bn.bias': be.grad, 'rm': rm, 'rv': rv}, r
    (r64, R), (r32, _) = run(F64), run(F32)
    assert 400 < R < 640, R
    return dict(m=m, x=x, g=g, r64=r64, r32=r32, R=R)


@gpu
def test_conv_module_at_R512():
    """Conv.train_fwd + backward on conv_module_case: output, dx, every parameter gradient and the running statistics against the torch functionals in
    float64, the bound from their float32 run."""
    k = conv_module_case()
    r64, r32, R = k['r64'], k['r32'], k['R']
    m = k['m'].to(DEV)
    y, dx = _module_step(m, k['x'], k['g'])
    got = {'y': y, 'dx': dx, 'g:conv.weight': m.conv.weight.grad, 'g:bn.weight': m.bn.weight.grad, 'g:bn.bias': m.bn.bias.grad, 'rm': m.bn.running_mean,
           'rv': m.bn.running_var}
    for q in r64:
        cond_check(got[q], r64[q], r32[q], F32, f'Conv conv1 R{R:.0f} {q}')


@functools.lru_cache(maxsize=None)
def conv_gn_module_case():
    """Conv_GN (conv 1x1 32 -> 64, GroupNorm(16), SiLU) with every row of the conv weight shifted to sum 1 and a constant offset on the input: every
    output channel then has mean = offset and std ||w[k]||, so each group of four channels has the ratio offset / ||w|| ~ 512 (with unequal row sums
    the spread of the channel means inside a group would be its std, whatever the offset)."""
    from mgdt_yolo_amd.nn.modules.head import Conv_GN
    from mgdt_yolo_amd.seeding import seed_state_dict_
    m = seed_state_dict_(Conv_GN(32, 64, 1), 11).train()
    gen = _gen('cond-convgn')
    with torch.no_grad():
        w = m.conv.weight.double()
        m.conv.weight.copy_((w - w.mean((1, 2, 3), keepdim=True) + 1.0 / 32).float())
    w = m.conv.weight.detach().double()
    off = 512.0 * w.flatten(1).norm(dim=1).median().item()
    x = (torch.randn(2, 32, 6, 5, generator=gen, dtype=F64) + off).float().double()
    g = torch.randn(2, 64, 6, 5, generator=gen, dtype=F64).float().double()
    sd = {k: v.detach().clone().double() for k, v in m.state_dict().items()}

    def run(ev):
        xr, wr, ga, be = (t.to(ev).clone().requires_grad_(True) for t in (x, sd['conv.weight'], sd['gn.weight'], sd['gn.bias']))
        c = F.conv2d(xr, wr)
        y = F.silu(F.group_norm(c, 16, ga, be, m.gn.eps))
        y.backward(g.to(ev))
        cg = c.detach().reshape(2, 16, -1)
        return {'y': y.detach(), 'dx': xr.grad, 'g:conv.weight': wr.grad, 'g:gn.weight': ga.grad, 'g:gn.bias': be.grad}, (cg.mean(-1).abs() / cg.std(-1)).median().item()
    (r64, R), (r32, _) = run(F64), run(F32)
    assert 400 < R < 640, R
    return dict(m=m, x=x, g=g, r64=r64, r32=r32, R=R)


@gpu
def test_conv_gn_module_at_R512():
    """Conv_GN.forward + backward on conv_gn_module_case: output, dx and every parameter gradient."""
    k = conv_gn_module_case()
    r64, r32, R = k['r64'], k['r32'], k['R']
    m = k['m'].to(DEV)
    y, dx = _module_step(m, k['x'], k['g'])
    got = {'y': y, 'dx': dx, 'g:conv.weight': m.conv.weight.grad, 'g:gn.weight': m.gn.weight.grad, 'g:gn.bias': m.gn.bias.grad}
    for q in r64:
        cond_check(got[q], r64[q], r32[q], F32, f'Conv_GN R{R:.0f} {q}')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_saturation_tood_layer_attn(dt):
    """tood_layer_attn and tood_layer_attn_bwd with the saturating values as the second layer's bias: the logits W2 relu(W1 avg + b1) + b2 sit at +-20,
    +-90, +-200 plus O(1).  Forward scale and dsums, dW1, db1, dW2, db2 (written over NaN) against float64, _close's fp32 bound
    (test_forward_kernels.py / test_tood_kernels.py)."""
    from mgdt_yolo_amd import ops
    B, C, S, hid, H, W = 2, 128, 8, 16, 6, 5
    gen = _gen('sat-tla')
    feat = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64) + 0.2, dt)
    w1 = (torch.randn(hid, C, generator=gen, dtype=F64) / C ** 0.5).float().double()
    b1 = (torch.randn(hid, generator=gen, dtype=F64) * 0.1).float().double()
    w2 = (torch.randn(S, hid, generator=gen, dtype=F64) / hid ** 0.5).float().double()
    b2 = torch.tensor([20.0, -20.0, 90.0, -90.0, 200.0, -200.0, 0.3, -0.4], dtype=F64)
    dscale = torch.randn(B, C, generator=gen, dtype=F64).float().double()
    sums = feat.sum((2, 3)).float().double()                              # what nc_reduce hands over, as fp32 values
    sr, w1r, b1r, w2r, b2r = (t.clone().requires_grad_(True) for t in (sums, w1, b1, w2, b2))
    wk = torch.sigmoid(torch.relu((sr / (H * W)) @ w1r.T + b1r) @ w2r.T + b2r)
    scale = wk.repeat_interleave(C // S, 1)
    (scale * dscale).sum().backward()
    dev = [_f32(t).contiguous() for t in (w1, b1, w2, b2)]
    fwd = torch.sigmoid(torch.relu(feat.mean((2, 3)) @ w1.T + b1) @ w2.T + b2).repeat_interleave(C // S, 1)
    _check(ops.tood_layer_attn(_nhwc(feat, dt)[0], *dev, S), fwd, F32, 'tood_layer_attn scale')
    refs = [w1r.grad, b1r.grad, w2r.grad, b2r.grad]
    bufs = [torch.full(r.shape, float('nan'), device=DEV) for r in refs]
    dsums = ops.tood_layer_attn_bwd(_f32(sums), _f32(dscale), H * W, *dev, S, *bufs, False)
    _check(dsums, sr.grad, F32, 'tood_layer_attn_bwd dsums')
    for name, buf, r in zip(('dW1', 'db1', 'dW2', 'db2'), bufs, refs):
        _check(buf, r, F32, f'tood_layer_attn_bwd {name}')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('softmax', [True, False], ids=['softmax', 'sigmoid'])
def test_saturation_spr_attention(softmax, dt):
    """spr_attention with the saturating values as fc2's bias (the logit of every channel's sigmoid), with and without the softmax over the groups;
    _close's fp32 bound (test_forward_kernels.py) against SPRModule per group in float64."""
    from mgdt_yolo_amd import ops
    from oracle import layers as OL
    B, groups, cw, H, W = 2, 4, 16, 9, 7
    C, hid = groups * cw, cw // 4
    gen = _gen('sat-spr', softmax)
    x = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64) + 0.3, dt)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64).float().double()
    sd = {'a.fc1.weight': r(hid, 5 * cw, 1, 1) * 0.4, 'a.fc1.bias': r(hid) * 0.2, 'a.fc2.weight': r(cw, hid, 1, 1) * 0.5,
          'a.fc2.bias': saturating(('spr',), cw).float().double()}
    ref = torch.cat([OL.spr(t, sd, 'a') for t in x.chunk(groups, 1)], 1).reshape(B, groups, cw)
    ref = (torch.softmax(ref, 1) if softmax else ref).reshape(B, C)
    w = [_f32(sd[k]).contiguous() for k in ('a.fc1.weight', 'a.fc1.bias', 'a.fc2.weight', 'a.fc2.bias')]
    _check(ops.spr_attention(_nhwc(x, dt)[0], *w, groups, softmax=softmax), ref, F32, f'spr_attention softmax={softmax}')


# ------------------------------------------------------------------------------------------------ GPU: the single-launch ConvNeXt block
@functools.lru_cache(maxsize=None)
def cnx_case(R):
    """'kc1-1-map-5x3' of test_cnx_kernels.BLOCK_CASES (C 32, 2 x 5 x 3) with the LayerNorm's pixel mean driven as in ln_case; reference, delta_s and flip
    allowance from kernel_ref's restatement alone (cnx_deltas grows with R: the fp32 evaluation of t decides fewer roundings)."""
    from test_cnx_kernels import EPS, _ln_weights, _mlp_weights
    C, B, H, W = 32, 2, 5, 3
    gen = _gen('cond-cnx')
    x = _q(torch.randn(B, C, H, W, generator=gen, dtype=F64), BF16)
    dw, dwb, lnw, lnb = _ln_weights(gen, C)
    mlp = _mlp_weights(gen, C)
    std = F.conv2d(x, dw.double(), None, 1, 3, 1, C).std(1, unbiased=False).median().item()
    if R == 'const':
        dw, dwb = (dw * (2.0 ** -10 / std)).float(), torch.ones(C)
    else:
        dwb = torch.full((C,), R * std).float()
    ln = (dw, dwb, lnw, lnb)
    if R == 'const':                                       # compared for finiteness only (test_cnx_block_ladder)
        return dict(x=x, ln=ln, mlp=mlp)
    y, st = ref_cnx_block(x, *ln, EPS, *mlp, stages=True)
    deltas = cnx_deltas(st, mlp[0], mlp[1], mlp[4], mlp[5], ln=(x, *ln, EPS))
    allow, count = cnx_allowance(st, deltas, mlp[0], mlp[1], mlp[2], mlp[5])
    return dict(x=x, ln=ln, mlp=mlp, y=y, allow=allow, count=count, deltas=deltas)


@gpu
@pytest.mark.parametrize('R', [8, 64, 'const'], ids=lambda r: f'R{r}')
def test_cnx_block_ladder(R):
    """The cnx_block launch (bf16) against ref_cnx_block plus the flip allowance, as test_cnx_kernels.test_cnx_block compares it; on the near-constant
    map every output must be finite and nothing more is compared.  The compared rungs stop at 64:
    the kernel rounds t = LayerNorm(...) to bf16 as pwconv1's operand, the allowance of that rounding comes from the float32 restatement's own distance
    (delta_t = 1e-5 at R = 8, 1e-4 at 64, 1e-3 at 512 and on the near-constant map), and from R = 512 on it exceeds half the plain bound on 99 % of the
    outputs (26 % at R = 64, 1 % at R = 8) - a comparison there would see nothing.  The LayerNorm arithmetic itself is held on every rung by
    test_dwconv7_ln_ladder."""
    from mgdt_yolo_amd import ops
    from test_cnx_kernels import EPS, _dev_mlp, _dw49
    k = cnx_case(R)
    gen = torch.Generator().manual_seed(5)
    xv, _ = _nhwc(k['x'], BF16, 8, 8, gen)
    dwb, lnw, lnb = (t.to(DEV) for t in k['ln'][1:])
    pk, gamma, beta = _dev_mlp(k['mlp'])
    out = ops.cnx_block(xv, _dw49(k['ln'][0]), dwb, lnw, lnb, EPS, pk, gamma, beta)
    if R == 'const':
        assert out.dtype == BF16 and torch.isfinite(out.float()).all(), 'cnx_block: non-finite output on the near-constant map'
        return
    print(f'delta_s {k["deltas"]}, undecided {k["count"]} of {k["y"].numel()} outputs')
    _close_allow(out, k['y'], k['allow'], f'cnx_block R{R}')


@gpu
@pytest.mark.parametrize('use_vfl', [True, False], ids=['vfl', 'focal'])
def test_saturation_detr_loss(use_vfl):
    """detr_loss (class / bbox / giou per layer, gt_score, d_boxes, d_logits) with saturating class logits and a given assignment, against
    rtdetr_loss_ref.losses in float64 and its autograd; the bound of test_rtdetr_loss.py: max(8 x the float32 CPU run's distance, 1e-6 x max|want|)."""
    import rtdetr_loss_ref as LR
    from mgdt_yolo_amd import ops
    l, B, nq, nc, G = 2, 2, 12, 5, 4
    gen = _gen('sat-detr')
    boxes = torch.cat([torch.rand(l, B, nq, 2, generator=gen, dtype=F64) * 0.6 + 0.2, torch.rand(l, B, nq, 2, generator=gen, dtype=F64) * 0.3 + 0.05], -1).float().double()
    logits = saturating(('detr',), l, B, nq, nc)
    gt_boxes = torch.cat([torch.rand(G, 2, generator=gen, dtype=F64) * 0.6 + 0.2, torch.rand(G, 2, generator=gen, dtype=F64) * 0.3 + 0.05], -1).float().double()
    gt_cls = torch.tensor([0, nc - 1, 2, 2])
    assign = torch.full((l, B, nq), -1, dtype=torch.long)
    for li in range(l):
        for b in range(B):
            q = torch.randperm(nq, generator=gen)[:2]
            assign[li, b, q] = torch.tensor([2 * b, 2 * b + 1])
    gain = {'cls': 1.0, 'bbox': 5.0, 'giou': 2.0}

    def run(ev):
        bx, lg = boxes.to(ev).clone().requires_grad_(True), logits.to(ev).clone().requires_grad_(True)
        out, score = LR.losses(bx, lg, gt_boxes.to(ev), gt_cls, assign, G, use_vfl=use_vfl, gain=gain)
        out.sum().backward()
        return dict(out=out.detach(), gt_score=score.detach(), d_boxes=bx.grad, d_logits=lg.grad)
    r64, r32 = run(F64), run(F32)
    out, score, d_boxes, d_logits = ops.detr_loss(boxes.float().to(DEV), logits.float().to(DEV), gt_boxes.float().to(DEV), gt_cls.to(torch.int32).to(DEV),
                                                  assign.to(torch.int32).to(DEV), G, gains=(1.0, 5.0, 2.0), use_vfl=use_vfl, want_grads=True)
    for k, got in (('out', out[:l]), ('gt_score', score), ('d_boxes', d_boxes), ('d_logits', d_logits)):
        want = r64[k]
        bound = max(8 * (r32[k].double() - want).abs().max().item(), 1e-6 * want.abs().max().item())
        got = got.cpu().double()
        d = (got - want).abs().max().item()
        print(f'detr_loss {"vfl" if use_vfl else "focal"} {k}: max |d| {d:.3e}, bound {bound:.3e}')
        assert torch.isfinite(got).all() and d <= bound, (k, d, bound)


@functools.lru_cache(maxsize=None)
def sat_loss_case(dt, underflow=False):
    """One level 13 x 11 (stride 8), B 2, reg_max 4, nc 8: kernel_ref.loss_maps with one logit in eight - class and DFL alike - replaced by +-20, +-90,
    +-200, and random boxes.  The decision margins of test_loss_kernels.py (kernel_ref.loss_margins) are conditions on the inputs: whole draws are
    redrawn (salt 0, 1, ...) until the float64 reference meets them (a sigmoid of -200 puts an align metric below the fp32 normal range)."""
    from kernel_ref import loss_gt_random, loss_maps, loss_margins, loss_reference
    B, R, nc, N = 2, 4, 8, 4
    for salt in range(64):
        gen = _gen('sat-loss', salt)
        gt = loss_gt_random(gen, B, N, nc, 11 * 8, 13 * 8, (4, 2), 10.0, 60.0)
        base = loss_maps(gen, B, R, nc, ((13, 11, 8),), dt)[0]
        sat = saturating(('loss', salt), *base.shape, dt=dt)
        m = torch.where(sat.abs() >= 20, sat, base)
        ref = loss_reference([m], gt, [8], R, nc, 0)
        try:
            loss_margins(ref, gt, R, f'saturating loss salt {salt}')
        except AssertionError:
            continue
        # one more condition of the same kind: loss_margins (e) keeps the ALIGN metric of every in-box top-k member above 1e-30, but the metric is
        # score^0.5 x iou^6 and the score itself must be an fp32 number too.  sigmoid(-90) = 8e-40 is not: fp32 has 1 / (1 + exp(90)) = 1 / inf = 0 (as
        # torch's own fp32 sigmoid on the device), the members' metrics tie at 0 and the top-k is undecided.  Measured on the MI355X on salt 0: two anchors
        # with float64 metrics 1.2e-23 and 1.1e-23 (9th and 10th of their box) not assigned.
        aux = ref['aux']
        topk, valid = aux['topk'], aux['mask_gt'].bool().squeeze(-1)
        inbox_k = torch.gather(aux['in_gts'], 2, topk) & valid[..., None]
        cls = m[:, 4 * R:].reshape(B, nc, -1)
        lab = gt[..., 0].long().clamp(0, nc - 1)
        logit_k = torch.gather(torch.gather(cls, 1, lab[..., None].expand(B, N, cls.shape[2])), 2, topk)
        under = (logit_k < -87.0) & inbox_k
        if under.any() != underflow:
            continue
        # underflow = True: the first draw that HAS such members.  Their boxes' top-k is undecided; every anchor outside those boxes is no candidate
        # of theirs whichever way the ties fall, and keeps its assignment: `decided` (B, anchors).
        decided = ~(aux['in_gts'] & under.any(-1)[..., None]).any(1)
        return m, gt, ref, (B, R, nc), decided
    raise AssertionError('no saturating draw meets the decision margins')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_saturation_detection_loss(dt):
    """detect_loss_fwd + detect_loss_bwd on saturating class and DFL logits, compared as test_loss_kernels.py compares a case: fg / gt_idx exact, tscore,
    items, total and max(sum tscore, 1) under the fp32 bound, the gradient under the bound of the map dtype against float64 autograd."""
    from mgdt_yolo_amd import ops
    from kernel_ref import _exact
    m, gt, ref, (B, R, nc), decided = sat_loss_case(dt)
    assert ref['fg'].any() and torch.isfinite(ref['grads'][0]).all() and decided.all()
    st = ops.detect_loss_fwd([_nhwc(m, dt)[0]], [8], R, nc, gt.to(DEV), 0, (7.5, 0.5, 1.5), want_assignment=True)
    _exact(st.fg, ref['fg'], 'fg')
    _exact(st.gt_idx, ref['gt_idx'], 'gt_idx')
    _check(st.tscore, ref['tscore'], F32, 'saturating loss tscore')
    _check(st.out5[1:4], ref['items'], F32, 'saturating loss items')
    _check(st.out5[0:1], ref['total'].reshape(1), F32, 'saturating loss total*B')
    _check(st.out5[4:5], ref['tss'].reshape(1), F32, 'saturating loss max(sum tscore, 1)')
    g = ops.detect_loss_bwd(st, 1.0)[0]
    assert g.dtype == dt
    _check(g, ref['grads'][0], dt, 'saturating loss grad')


@gpu
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_saturation_detection_loss_underflowing_score(dt):
    """The assigner with class scores that underflow: a draw in which top-k in-box anchors have a label-class logit below -87, so that their fp32 score
    and align metric are 0 and their box's top-k ties.  Either tie order is accepted: fg / gt_idx must be exact on every anchor outside the boxes with
    such members, and every output - tscore, the loss items, the gradient - finite (no 0 / 0 from the tied metrics' normalisation)."""
    from mgdt_yolo_amd import ops
    m, gt, ref, (B, R, nc), decided = sat_loss_case(dt, True)
    assert not decided.all() and decided.any()
    st = ops.detect_loss_fwd([_nhwc(m, dt)[0]], [8], R, nc, gt.to(DEV), 0, (7.5, 0.5, 1.5), want_assignment=True)
    fg, gt_idx = st.fg.cpu().reshape(decided.shape), st.gt_idx.cpu().reshape(decided.shape)
    rfg = ref['fg'].reshape(decided.shape)
    assert torch.equal(fg.bool()[decided], rfg.bool()[decided]), 'fg differs outside the undecided boxes'
    both = decided & rfg.bool()
    assert torch.equal(gt_idx[both].long(), ref['gt_idx'].reshape(decided.shape)[both].long()), 'gt_idx differs outside the undecided boxes'
    print(f'undecided anchors: {int((~decided).sum())} of {decided.numel()}, fg there: kernel {int(fg.bool()[~decided].sum())}, float64 {int(rfg.bool()[~decided].sum())}')
    g = ops.detect_loss_bwd(st, 1.0)[0]
    for name, t in (('tscore', st.tscore), ('out5', st.out5), ('grad', g)):
        assert torch.isfinite(t.float()).all(), f'saturating loss with underflowing scores: non-finite {name}'
