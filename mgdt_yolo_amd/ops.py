"""Thin torch-tensor wrappers over the C ABI (include/mgdt.h).  PyTorch is plumbing here: device memory,
the current HIP stream, nn.Parameter containers.  Every compute step goes through libmgdt_hip.so.

Activations are torch tensors shaped (B, C, H, W) in channels_last memory format (NHWC in memory); channel
slices `t[:, a:b]` are passed as strided views - the reference's chunk()/split()/cat() never copy here.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU, BF16, F32, View  # noqa: F401

U8 = 2    # uint8 image input of the stem only (divided by 255 in the kernel)
_DT = {torch.float32: F32, torch.bfloat16: BF16}


def dtype_code(dt):
    try:
        return _DT[dt]
    except KeyError:
        raise RuntimeError(f'mgdt_yolo_amd computes in float32 or bfloat16, not {dt}') from None


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError('mgdt_yolo_amd runs on MI355X (HIP) only: got a CPU tensor and there is no CPU/PyTorch fallback')


def version_of(t):
    """`t._version` as a cache key.  A tensor made under torch.inference_mode() has no version counter (reading it raises); it can only be
    written in place inside that mode, where nothing counts the write, so its key is the constant -1 and whoever writes into such a parameter
    moves PARAM_EPOCH (BaseModel.load_state_dict does)."""
    return -1 if t.is_inference() else t._version


def refuse_inference_mode(what):
    """Training calls keep activations and gradients across calls; tensors made under torch.inference_mode() cannot be written outside it,
    and a train-mode forward keeps nothing for the reverse pass there (autograd is off).  Refused before any launch."""
    if torch.is_inference_mode_enabled():
        raise RuntimeError(f'{what} under torch.inference_mode(): training calls are made outside it (the mode is for eval forwards, NMS and '
                           'validation)')


_PROF = None   # list collecting (name, meta, start_event, end_event) while ops.profile() is active


def _launch(name, symbol, *args, meta=None):
    """Call one C-ABI entry point on the current stream; raise on a non-zero status."""
    fn = getattr(L.lib(), symbol)
    if _PROF is None:
        L.check(fn(*args), name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.check(fn(*args), name)
    e1.record()
    _PROF.append((name, meta or _META.pop(name, None), e0, e1))


_META = {}


class profile:
    """with ops.profile() as p: ...  -> p.rows = [(name, meta, ms)] measured with HIP events on the launch stream."""

    def __enter__(self):
        global _PROF
        _PROF = self._raw = []
        return self

    def __exit__(self, *exc):
        global _PROF
        _PROF = None
        torch.cuda.synchronize()
        self.rows = [(n, m, a.elapsed_time(b)) for n, m, a, b in self._raw]
        return False


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


SIDE_STREAM = os.environ.get('MGDT_SIDE_STREAM', '1') != '0'      # inference: layers that do not depend on their predecessors run on a second HIP stream (BaseModel._side_branch)
_SIDE = {}


def side_stream(device):
    """The second launch stream of `device` (one per process, device and lane - see ops.lane; created outside graph capture on first use)."""
    dev = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    key = (dev, _LANE[0])
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=dev)
    return _SIDE[key]


_FORCE_CTX = [0]


def ctx_enabled():
    """True when a train-mode forward should keep activations for backward(): autograd is recording, or the model-level
    autograd Function (which runs its forward under no_grad) asked for it."""
    return _FORCE_CTX[0] > 0 or torch.is_grad_enabled()


class force_ctx:
    def __enter__(self):
        _FORCE_CTX[0] += 1

    def __exit__(self, *exc):
        _FORCE_CTX[0] -= 1
        return False


def view(t):
    """(B,C,H,W) tensor of any strides -> mgdt_view (NHWC-ordered sizes/strides)."""
    _need_gpu(t)
    b, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    return View(t.data_ptr(), b, h, w, c, sn, sh, sw, sc)


def vp(t):
    return C.byref(view(t)) if t is not None else None


def ptr(t):
    if t is None:
        return None
    _need_gpu(t)
    return C.c_void_p(t.data_ptr())


def _same(*ts):
    """Views that one kernel addresses with ONE dtype code must really share it: a bf16 map read as fp32 is an out-of-bounds access on the device,
    so the mismatch is refused here."""
    ts = [t for t in ts if t is not None]
    for t in ts[1:]:
        if t.dtype != ts[0].dtype:
            raise RuntimeError(f'mgdt_yolo_amd: operands of one kernel must share a dtype, got {[str(u.dtype) for u in ts]}')


def new_act(b, c, h, w, dtype, device):
    """NHWC activation buffer presented with NCHW shape semantics."""
    return torch.empty((b, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def is_nhwc(t):
    return t.stride(1) == 1


def grad_buf(p):
    """The gradient tensor of parameter p (allocated on first use; the trainer points it into its flat gradient buffer)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def like(t):
    """Dense NHWC buffer with t's shape/dtype (torch.empty_like would inherit a channel-slice view's odd strides)."""
    return new_act(t.shape[0], t.shape[1], t.shape[2], t.shape[3], t.dtype, t.device)


# ------------------------------------------------------------------ conv
class PackedConv:
    """Caller-owned packed weights of one convolution (BN folded) for one compute dtype."""
    __slots__ = ('w', 'bias', 'k', 'cin', 'cout', 'dtype', 'direct', 'groups', 'src', 'epoch', '__weakref__')

    def __init__(self, weight, conv_bias, bn, k, dtype, direct=False, groups=1):
        """weight: (cout, cin/groups, k, k) fp32 cuda; bn: None or (gamma, beta, mean, var, eps)."""
        lib = L.lib()
        weight = weight.detach().float().contiguous()
        _need_gpu(weight)
        cout, cin_g = weight.shape[0], weight.shape[1]
        dev = weight.device
        g, b, mu, var, eps = (None, None, None, None, 0.0) if bn is None else bn
        f = lambda t: None if t is None else t.detach().float().contiguous()
        g, b, mu, var, cb = f(g), f(b), f(mu), f(var), f(conv_bias)
        self.k, self.cin, self.cout, self.dtype, self.direct, self.groups = k, cin_g * groups, cout, dtype, direct, groups
        if direct:
            self.w = torch.empty(k * k * cin_g * cout, dtype=torch.float32, device=dev)
            self.bias = torch.empty(cout, dtype=torch.float32, device=dev)
            _launch('conv_pack_direct', 'mgdt_conv_pack_direct', ptr(weight), ptr(cb), ptr(g), ptr(b), ptr(mu), ptr(var), eps, cin_g, cout, k,
                                              ptr(self.w), ptr(self.bias), stream())
        else:
            code = dtype_code(dtype)
            nbytes = lib.mgdt_conv_packed_bytes(cin_g, cout, k, code)
            self.w = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.bias = torch.empty((cout + 15) // 16 * 16, dtype=torch.float32, device=dev)
            _launch('conv_pack', 'mgdt_conv_pack', ptr(weight), ptr(cb), ptr(g), ptr(b), ptr(mu), ptr(var), eps, cin_g, cout, k, code,
                                       ptr(self.w), ptr(self.bias), stream())
            if groups == 1:
                _register_pack(self, (weight, cb, g, b, mu, var, float(eps), cin_g, cout, k, code, 0))


class PackedConvFp8:
    """e4m3 panel of one convolution (BN folded, per-output-channel weight scales) for the activation multiplier `xq` - mgdt_conv_pack_fp8."""
    __slots__ = ('w', 'bias', 'oscale', 'xq', 'k', 'cin', 'cout', 'dtype', 'direct', 'groups', '__weakref__')

    def __init__(self, weight, conv_bias, bn, k, xq):
        lib = L.lib()
        weight = weight.detach().float().contiguous()
        _need_gpu(weight)
        cout, cin = weight.shape[0], weight.shape[1]
        dev = weight.device
        g, b, mu, var, eps = (None, None, None, None, 0.0) if bn is None else bn
        f = lambda t: None if t is None else t.detach().float().contiguous()
        g, b, mu, var, cb = f(g), f(b), f(mu), f(var), f(conv_bias)
        self.k, self.cin, self.cout, self.dtype, self.direct, self.groups, self.xq = k, cin, cout, torch.bfloat16, False, 1, float(xq)
        self.w = torch.empty(lib.mgdt_conv_packed_bytes_fp8(cin, cout, k), dtype=torch.uint8, device=dev)
        cpad = (cout + 15) // 16 * 16
        self.bias = torch.empty(cpad, dtype=torch.float32, device=dev)
        self.oscale = torch.empty(cpad, dtype=torch.float32, device=dev)
        _launch('conv_pack_fp8', 'mgdt_conv_pack_fp8', ptr(weight), ptr(cb), ptr(g), ptr(b), ptr(mu), ptr(var), eps, cin, cout, k, self.xq,
                ptr(self.w), ptr(self.bias), ptr(self.oscale), stream())


Q8_CALIB = None    # dict module -> running max|input| while BaseModel.quantize_fp8() runs its calibration batches
Q8_CALIB_PCT = None  # None: the maximum of |input|; a number: that percentile of |input| (per batch, the largest over the batches)


def conv2d_fp8(x, pk, stride, act, out=None, x2=None, r1=None, r2=None, in_scale=None, in_shift=None):
    """mgdt_conv2d_fp8_fwd: bf16 views, e4m3 operands on the MFMA, fp32 accumulation."""
    _need_gpu(x)
    b, _, h, w = x.shape
    ho, wo = conv_out_hw(h, w, pk.k, stride)
    if out is None:
        out = new_act(b, pk.cout, ho, wo, torch.bfloat16, x.device)
    _same(x, x2, r1, r2, out)
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f'conv2d_fp8: activations are bf16 in HBM, the input is {x.dtype}')
    if _PROF is not None:
        _META['conv2d_fp8_fwd'] = dict(shape=(b, pk.cin, h, w, pk.cout, pk.k, stride), flops=2.0 * b * ho * wo * pk.cout * pk.cin * pk.k * pk.k,
                                       bytes=float(b * h * w * pk.cin * 2 + b * ho * wo * pk.cout * 2 + pk.cout * pk.cin * pk.k * pk.k))
    _launch('conv2d_fp8_fwd', 'mgdt_conv2d_fp8_fwd', vp(x), vp(x2), ptr(in_scale), ptr(in_shift), ptr(pk.w), ptr(pk.bias), ptr(pk.oscale), pk.xq,
            pk.k, stride, act, vp(r1), vp(r2), vp(out), stream())
    return out


# ---- batched re-pack after an optimizer step -------------------------------------------------------------------------------------
# Every packed panel built from live parameter storage registers (weakly) what it was built from.  `repack_all()` - called by the trainer
# right after the HIP optimizer moved the weights - refreshes all panels that were valid for the step that just ran with
# mgdt_conv_pack_batch (a handful of launches instead of one per convolution) and stamps them with the new PARAM_EPOCH; the caches that
# hold them (HipModule._cached, the data-gradient cache below) accept a stamped panel instead of rebuilding it.
_PACK_REGISTRY = None
LIVE_STORAGES = set()          # storages that hold the parameters / buffers the HIP optimizer updates in place (FlatState registers its buffer)


def _register_pack(obj, src):
    """Only panels built directly from live parameter storage can be refreshed in place: a panel packed from a derived copy (torch.cat of two
    branches, zero-padded rows) must be rebuilt from a fresh copy, so it is never registered."""
    global _PACK_REGISTRY
    import weakref
    if not all(t is None or t.untyped_storage().data_ptr() in LIVE_STORAGES for t in src[:6]):
        return
    if _PACK_REGISTRY is None:
        _PACK_REGISTRY = weakref.WeakSet()
    obj.src, obj.epoch = src, PARAM_EPOCH[0]
    _PACK_REGISTRY.add(obj)


def repack_all():
    """Refresh every registered panel that was current before the last optimizer step (PARAM_EPOCH - 1); returns them."""
    if not _PACK_REGISTRY:
        return []
    live = [o for o in _PACK_REGISTRY if getattr(o, 'epoch', -2) == PARAM_EPOCH[0] - 1]
    if not live:
        return []
    arr = (L.PackDesc * len(live))()
    for d, o in zip(arr, live):
        w, cb, g, b, mu, var, eps, cin, cout, k, code, mode = o.src
        d.w, d.conv_bias, d.bn_gamma, d.bn_beta, d.bn_mean, d.bn_var = ptr(w), ptr(cb), ptr(g), ptr(b), ptr(mu), ptr(var)
        d.bn_eps, d.cin, d.cout, d.k, d.dtype, d.mode = eps, cin, cout, k, code, mode
        d.packed, d.bias_out = ptr(o.w), ptr(o.bias)
    _launch('conv_pack_batch', 'mgdt_conv_pack_batch', arr, len(live), stream())
    for o in live:
        o.epoch = PARAM_EPOCH[0]
    return live


def fresh_epoch_for_capture():
    """Move PARAM_EPOCH although no weight changed, and take the registered panels that were current along.  Afterwards every cache entry that
    only the epoch keeps valid - a derived copy of the weights, a panel packed from one: nothing refreshes those in place - misses, so a graph
    capture that follows rebuilds them with captured launches instead of reading, on every replay, what an eval forward of the same epoch left
    in memory the graph does not own."""
    cur = [o for o in (_PACK_REGISTRY or ()) if pack_is_current(o)]
    PARAM_EPOCH[0] += 1
    for o in cur:
        o.epoch = PARAM_EPOCH[0]


def pack_is_current(obj):
    return getattr(obj, 'epoch', None) == PARAM_EPOCH[0]


def conv_can_mfma(x, cin, cout, k, s, groups, dtype):
    pe = 8 if dtype == torch.bfloat16 else 4
    return (groups == 1 and k in (1, 3) and s in (1, 2) and cin % pe == 0 and cout % 4 == 0 and x.dtype == dtype
            and is_nhwc(x) and x.stride(3) % pe == 0 and x.stride(2) % pe == 0 and x.stride(0) % pe == 0
            and x.data_ptr() % 16 == 0)


def conv_out_hw(h, w, k, s):
    p = k // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def conv2d(x, pk, stride, act, out=None, x2=None, r1=None, r2=None, in_scale=None, in_shift=None):
    """Fused conv (see mgdt_conv2d_fwd).  Returns `out` (allocated NHWC when None)."""
    _need_gpu(x)
    b, _, h, w = x.shape
    ho, wo = conv_out_hw(h, w, pk.k, stride)
    if out is None:
        out = new_act(b, pk.cout, ho, wo, pk.dtype, x.device)
    if _PROF is not None:
        es = out.element_size()
        _META['conv2d_direct_fwd' if pk.direct else 'conv2d_fwd'] = dict(
            shape=(b, pk.cin, h, w, pk.cout, pk.k, stride), flops=2.0 * b * ho * wo * pk.cout * pk.cin // pk.groups * pk.k * pk.k,
            bytes=float(b * h * w * pk.cin * x.element_size() + b * ho * wo * pk.cout * es + pk.w.numel() * pk.w.element_size()))
    if pk.direct:
        if x2 is not None or r1 is not None or r2 is not None or in_scale is not None or in_shift is not None:
            raise RuntimeError('direct convolution path has no fused extras')
        _launch('conv2d_direct_fwd', 'mgdt_conv2d_direct_fwd', vp(x), U8 if x.dtype == torch.uint8 else dtype_code(x.dtype), ptr(pk.w), ptr(pk.bias), pk.k, stride, pk.groups, act,
                                           vp(out), dtype_code(out.dtype), stream())
    else:
        _same(x, x2, r1, r2, out)
        if x.dtype != pk.dtype:
            raise RuntimeError(f'conv2d: the weights are packed for {pk.dtype}, the input is {x.dtype}')
        _launch('conv2d_fwd', 'mgdt_conv2d_fwd', vp(x), vp(x2), ptr(in_scale), ptr(in_shift), ptr(pk.w), ptr(pk.bias), pk.k, stride, act,
                                    vp(r1), vp(r2), vp(out), dtype_code(pk.dtype), stream())
    return out


def conv2d_route(x, y, k, stride, dtype=None, act=ACT_SILU, x2=False, in_scale=False, in_shift=False, r1=False, r2=False, fp8=False):
    """mgdt_conv2d_route: the plan conv2d / conv2d_fp8 would launch for the views x -> y with these fused extras, as a dict.  Launches nothing and needs
    no device: x and y may live anywhere (CPU or meta tensors included), only their sizes and strides count.  'family' is 'igemm' (keys NT, MT, D, extra,
    nseg, seg_chunks, waves, gx, gy, numTiles, ragged, nchunks, lds_bytes) or 'lds3x3' (NBW, tile_rows, ncg, nwg, ntiles, waves, nchunks, lds_bytes)."""
    def shape_view(t):
        b, c, h, w = t.shape
        sn, sc, sh, sw = t.stride()
        return View(None, b, h, w, c, sn, sh, sw, sc)
    flags = sum(f for on, f in ((x2, L.ROUTE_X2), (in_scale, L.ROUTE_IN_SCALE), (in_shift, L.ROUTE_IN_SHIFT), (r1, L.ROUTE_R1), (r2, L.ROUTE_R2),
                                (fp8, L.ROUTE_FP8)) if on)
    r = L.ConvRoute()
    L.check(L.lib().mgdt_conv2d_route(C.byref(shape_view(x)), C.byref(shape_view(y)), k, stride, dtype_code(dtype or x.dtype), flags, act, C.byref(r)),
            'conv2d_route')
    keys = (('NT', 'MT', 'D', 'extra', 'nseg', 'seg_chunks', 'gx', 'gy', 'numTiles', 'ragged') if r.family == L.ROUTE_IGEMM
            else ('NBW', 'tile_rows', 'ncg', 'nwg', 'ntiles'))
    out = {'family': 'igemm' if r.family == L.ROUTE_IGEMM else 'lds3x3'}
    out.update((n, getattr(r, n)) for n in keys + ('waves', 'nchunks', 'lds_bytes'))
    return out


def _route_view(t):
    """mgdt_view of a tensor for a host-side route query: sizes, strides and a pointer that is never dereferenced, only tested for alignment.  A meta tensor
    has no address: its byte offset inside its storage stands in (device allocations start on 256-byte boundaries)."""
    b, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    p = 4096 + t.storage_offset() * t.element_size() if t.device.type == 'meta' else t.data_ptr()
    return View(p, b, h, w, c, sn, sh, sw, sc)


def _image_code(dt):
    return dt if isinstance(dt, int) else (U8 if dt == torch.uint8 else dtype_code(dt))


def conv2d_direct_route(x, y, k, stride, groups=1, x_dtype=None, dtype=None):
    """mgdt_conv2d_direct_route: what mgdt_conv2d_direct_fwd would launch for the views x -> y, as a dict: family 'stem' / 'generic' with its grid
    (gx, gy), or 'refused' with the status the launch would fail with.  Launches nothing and needs no device: x and y may be CPU or meta tensors; only
    sizes, strides, dtypes and the alignment of y's address count.  x_dtype / dtype override the tensors' dtypes (torch dtypes or C-ABI codes)."""
    out = (C.c_int * 4)()
    L.check(L.lib().mgdt_conv2d_direct_route(C.byref(_route_view(x)), _image_code(x.dtype if x_dtype is None else x_dtype), C.byref(_route_view(y)),
                                             _image_code(y.dtype if dtype is None else dtype), int(k), int(stride), int(groups), out), 'conv2d_direct_route')
    return dict(family=('stem', 'generic', 'refused')[out[0]], gx=out[1], gy=out[2], status=out[3])


# ------------------------------------------------------------------ MSPA attention
def spr_attention(x, fc1_w, fc1_b, fc2_w, fc2_b, groups, softmax=True):
    """softmax_over_groups(SPR(x_group)) -> attn fp32 [B, C] (softmax=False: the bare sigmoid weights)."""
    b, c, h, w = x.shape
    lib = L.lib()
    part = torch.empty(b * L.SPR_SPLITS * c * 5, dtype=torch.float32, device=x.device)
    _launch('spr_pool_fwd', 'mgdt_spr_pool_fwd', vp(x), ptr(part), dtype_code(x.dtype), stream())
    attn = torch.empty(b, c, dtype=torch.float32, device=x.device)
    _launch('spr_attn_fwd', 'mgdt_spr_attn_fwd', ptr(part), ptr(fc1_w), ptr(fc1_b), ptr(fc2_w), ptr(fc2_b), b, c, groups, h, w, int(bool(softmax)),
            ptr(attn), stream())
    return attn


def spr_attention_scale(x, fc1_w, fc1_b, fc2_w, fc2_b, groups, out=None, part=None, nsplit=0, tiles=(0, 0), pools=()):
    """out = x * softmax_over_groups(SPR(x_group)): pooling pass (skipped when the producing kernel already left its per-tile sums in
    `part`, fp32 [b][nsplit][c] over a tiles[0] x tiles[1] (x, y) tile grid), then attention MLP + scaling in one launch.  `pools`: up to two
    NHWC views (b, c, h / F, w / F) that receive adaptive_avg_pool2d(out) in the same launch."""
    b, c, h, w = x.shape
    if part is None:
        part = torch.empty(b * L.SPR_SPLITS * c * 5, dtype=torch.float32, device=x.device)
        _launch('spr_pool_fwd', 'mgdt_spr_pool_fwd', vp(x), ptr(part), dtype_code(x.dtype), stream())
        nsplit, tiles = L.SPR_SPLITS, (0, 0)
    out = like(x) if out is None else out
    pools = list(pools)
    if len(pools) > 2:
        raise RuntimeError('spr_attention_scale: at most two pooled outputs')
    _same(x, out, *pools)
    pa, pb = (pools + [None, None])[:2]
    _launch('spr_attn_scale_fwd', 'mgdt_spr_attn_scale_fwd', ptr(part), int(nsplit), int(tiles[0]), int(tiles[1]), ptr(fc1_w), ptr(fc1_b), ptr(fc2_w), ptr(fc2_b), groups, vp(x), vp(out),
            vp(pa), vp(pb), dtype_code(x.dtype), stream())
    return out


FUSED_NECK = True     # tests flip this: SimFusion inputs delivered by their producers (pooled copies / direct concat-slot writes) vs separate launches


# ------------------------------------------------------------------ layers 0 + 1 in one launch
FUSED_STEM = True        # tests flip this to compare against the two conv launches


class PackedStem2:
    """Layer-0 weights (3 -> 16, k3 s2, BN folded exactly as fuse_conv_and_bn) in the fragment order of mgdt_stem2_fwd + bias."""

    def __init__(self, weight, bn):
        g, b, mu, var, eps = bn
        scale = (g.detach().float() / torch.sqrt(eps + var.detach().float()))
        wf = (weight.detach().float() * scale.view(-1, 1, 1, 1)).contiguous()
        self.bias = (b.detach().float() - g.detach().float() * mu.detach().float() / torch.sqrt(var.detach().float() + eps)).contiguous()
        self.blob = torch.empty(L.lib().mgdt_stem2_packed_bytes(), dtype=torch.uint8, device=weight.device)
        L.check(L.lib().mgdt_stem2_pack(ptr(wf), ptr(self.blob), stream()), 'stem2_pack')


def stem2(x, pk0, pk1):
    """x (B, 3, H, W) NCHW image (bf16 / fp32 / uint8) -> SiLU(conv1(SiLU(conv0(x)))) as (B, 32, H/4, W/4) bf16 NHWC."""
    _need_gpu(x)
    b, _, h, w = x.shape
    h0, w0 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    h1, w1 = (h0 - 1) // 2 + 1, (w0 - 1) // 2 + 1
    y = new_act(b, 32, h1, w1, torch.bfloat16, x.device)
    if _PROF is not None:
        _META['stem2_fwd'] = dict(shape=(b, 3, h, w, 32, 3, 4), flops=2.0 * b * (h0 * w0 * 16 * 27 + h1 * w1 * 32 * 144),
                                  bytes=float(x.numel() * x.element_size() + y.numel() * 2))
    _launch('stem2_fwd', 'mgdt_stem2_fwd', vp(x), U8 if x.dtype == torch.uint8 else dtype_code(x.dtype), ptr(pk0.blob), ptr(pk0.bias), ptr(pk1.w), ptr(pk1.bias),
            vp(y), stream())
    return y


def stem2_route(x, y, cu_count=0, x_dtype=None):
    """mgdt_stem2_route: what mgdt_stem2_fwd would launch for the image view x and the output view y on a device with cu_count compute units (<= 0: the
    current device's), as a dict: loader 'fast' (16-byte row loads, next patch prefetched) / 'generic', tiles_x, tiles_y, tiles, grid, per_xcd; or
    loader 'refused' with the status of the launch.  Launches nothing; with cu_count > 0 it needs no device (CPU or meta tensors)."""
    out = (C.c_int * 7)()
    L.check(L.lib().mgdt_stem2_route(C.byref(_route_view(x)), _image_code(x.dtype if x_dtype is None else x_dtype), C.byref(_route_view(y)), int(cu_count), out),
            'stem2_route')
    if out[6]:
        return dict(loader='refused', status=out[6])
    return dict(loader='fast' if out[0] else 'generic', tiles_x=out[1], tiles_y=out[2], tiles=out[3], grid=out[4], per_xcd=out[5])


# ------------------------------------------------------------------ the 6x6 / stride 2 / padding 2 stem (YOLOv5) as space-to-depth + 3x3
def space_to_depth2_channels(c, dtype):
    """channels of the space-to-depth map of a c-channel image in `dtype`: 4c rounded up to whole 16-byte stores (3 -> 12 fp32, 16 bf16)"""
    v = 8 if dtype == torch.bfloat16 else 4
    return (4 * c + v - 1) // v * v


def space_to_depth2(x, dtype, out=None):
    """x (B, C <= 4, H, W) image of any strides (uint8 is divided by 255 / fp32 / bf16), H and W even -> S (B, Cp, H/2, W/2) NHWC in `dtype` with
    S[b, (dy*2+dx)*C + ci, i, j] = x[b, ci, 2i+dy, 2j+dx] and channels 4C.. zero (mgdt_space_to_depth2_fwd)."""
    b, c, h, w = x.shape
    if c > 4 or h % 2 or w % 2:
        raise RuntimeError(f'space_to_depth2: an image of at most 4 channels with even height and width, got {tuple(x.shape)}')
    _need_gpu(x)
    if x.dtype != torch.uint8 and dtype_code(x.dtype) == BF16 and dtype != torch.bfloat16:
        raise RuntimeError('space_to_depth2: a bf16 image goes to a bf16 map')
    if out is None:
        out = new_act(b, space_to_depth2_channels(c, dtype), h // 2, w // 2, dtype, x.device)
    if _PROF is not None:
        _META['space_to_depth2_fwd'] = dict(shape=tuple(x.shape), flops=0.0, bytes=float(x.numel() * x.element_size() + out.numel() * out.element_size()))
    _launch('space_to_depth2_fwd', 'mgdt_space_to_depth2_fwd', vp(x), U8 if x.dtype == torch.uint8 else dtype_code(x.dtype), vp(out), dtype_code(out.dtype), stream())
    return out


class PackedStem6(PackedConv):
    """Panel of the 3x3 / stride 1 form of the 6x6 / stride 2 / padding 2 stem over the space-to-depth map (BN folded, zero rows for the map's pad
    channels), packed straight from the live 6x6 weight (mgdt_conv_pack_stem6): repack_all() refreshes it in place like every other panel."""
    __slots__ = ()

    def __init__(self, weight6, conv_bias, bn, dtype):
        """weight6: (cout, c6 <= 4, 6, 6) fp32 cuda; bn: None or (gamma, beta, mean, var, eps)."""
        lib = L.lib()
        weight = weight6.detach().float().contiguous()
        _need_gpu(weight)
        cout, c6 = weight.shape[0], weight.shape[1]
        if tuple(weight.shape[2:]) != (6, 6) or c6 > 4:
            raise RuntimeError(f'PackedStem6: a (cout, <= 4, 6, 6) weight, got {tuple(weight.shape)}')
        g, b, mu, var, eps = (None, None, None, None, 0.0) if bn is None else bn
        f = lambda t: None if t is None else t.detach().float().contiguous()
        g, b, mu, var, cb = f(g), f(b), f(mu), f(var), f(conv_bias)
        code = dtype_code(dtype)
        cp = space_to_depth2_channels(c6, dtype)
        self.k, self.cin, self.cout, self.dtype, self.direct, self.groups = 3, cp, cout, dtype, False, 1
        self.w = torch.empty(lib.mgdt_conv_packed_bytes(cp, cout, 3, code), dtype=torch.uint8, device=weight.device)
        self.bias = torch.empty((cout + 15) // 16 * 16, dtype=torch.float32, device=weight.device)
        _launch('conv_pack', 'mgdt_conv_pack_stem6', ptr(weight), ptr(cb), ptr(g), ptr(b), ptr(mu), ptr(var), eps, c6, cout, code, ptr(self.w), ptr(self.bias), stream())
        _register_pack(self, (weight, cb, g, b, mu, var, float(eps), c6, cout, 3, code, 5 + c6))


def stem6_w3(w6, cp=None):
    """The 3x3 weight over the space-to-depth map that equals the 6x6 / stride 2 / padding 2 weight w6 (cout, C, 6, 6):
    W3[co, (dy*2+dx)*C + ci, a, b] = W6[co, ci, 2a+dy, 2b+dx]; rows 4C..cp zero.  A derived copy (plain tensor indexing, any device)."""
    co, c = w6.shape[0], w6.shape[1]
    w3 = w6.detach().reshape(co, c, 3, 2, 3, 2).permute(0, 3, 5, 1, 2, 4).reshape(co, 4 * c, 3, 3)
    if cp is not None and cp > 4 * c:
        w3 = torch.cat([w3, w3.new_zeros(co, cp - 4 * c, 3, 3)], 1)
    return w3.contiguous()


def stem6_w6(w3, c):
    """Inverse of stem6_w3 on the first 4c rows: (cout, >= 4c, 3, 3) -> (cout, c, 6, 6)."""
    co = w3.shape[0]
    return w3[:, :4 * c].reshape(co, 2, 2, c, 3, 3).permute(0, 3, 4, 1, 5, 2).reshape(co, c, 6, 6).contiguous()


def stem6_wgrad_unpack(dw3, dw6):
    """dw6 (cout, C, 6, 6) fp32 <- the final sums dw3 (cout, cp, 3, 3) fp32 of the 3x3 weight gradient over the space-to-depth map (mgdt_stem6_wgrad_unpack).
    Pending deferred weight-gradient sums are flushed first: the permutation reads final sums, never partials."""
    flush_wgrad()
    if not (dw3.is_contiguous() and dw6.is_contiguous() and dw3.dtype == dw6.dtype == torch.float32 and dw3.shape[0] == dw6.shape[0]
            and tuple(dw3.shape[2:]) == (3, 3) and tuple(dw6.shape[2:]) == (6, 6) and dw3.shape[1] >= 4 * dw6.shape[1]):
        raise RuntimeError(f'stem6_wgrad_unpack: contiguous fp32 (cout, cp, 3, 3) -> (cout, c, 6, 6), got {tuple(dw3.shape)} -> {tuple(dw6.shape)}')
    _launch('stem6_wgrad_unpack', 'mgdt_stem6_wgrad_unpack', ptr(dw3), dw6.shape[0], dw6.shape[1], dw3.shape[1], ptr(dw6), stream())
    return dw6


# ------------------------------------------------------------------ whole CSP block (MSPA_C2f / C2f) in one launch
FUSED_CSP_BLOCK = True   # tests flip this to compare against the per-conv launch chain
CSP_MSPA, CSP_C2F, CSP_C3 = 0, 1, 2
# C3 blocks (mode CSP_C3): the (wd, n) classes that take the one-launch route.  Decided by measurement (tools/c3_bench.py): a class is
# listed only where its median beat the composed route's by more than the run-to-run spread of the two.  None: every class the kernel covers (tests, the tool).
C3_FUSED_CLASSES = ((16, 1), (32, 1), (32, 2), (64, 1))      # the yolov5n blocks at B = 32, 640 x 640; (16, 2) and (64, 2) are covered by the kernel but unmeasured: composed


def c3_fused_route(wd, nbtl):
    return FUSED_CSP_BLOCK and (C3_FUSED_CLASSES is None or (int(wd), int(nbtl)) in C3_FUSED_CLASSES)


def csp_block_supported(mode, x, cout, wd, nbtl, dtype):
    """channel counts / dtype covered AND a tile decomposition exists for this map (tiles must divide it: none for e.g. a 37-row map)"""
    if not (FUSED_CSP_BLOCK and dtype == torch.bfloat16 and x.dtype == dtype and is_nhwc(x)):
        return False
    lib = L.lib()
    if not lib.mgdt_csp_block_supported(mode, x.shape[1], int(cout), int(wd), int(nbtl), x.shape[2], x.shape[3], dtype_code(dtype)):
        return False
    return lib.mgdt_csp_block_tiles(mode, x.shape[0], x.shape[1], int(cout), int(wd), int(nbtl), x.shape[2], x.shape[3], None) > 0


def csp_block(mode, x, front, front_bias, mids, shortcut, back, wd, act, cout, want_pool):
    """mgdt_csp_block_fwd: `front` = PackedPwChain.blob (MSPA) or PackedConv (C2f); `mids` = PackedConv list of the bottlenecks' 3x3 convs;
    `back` = PackedConv of the 1x1 over the concat.  Returns (y, per-tile channel sums or None, pool slots, (tiles_x, tiles_y))."""
    lib = L.lib()
    b, cin, h, w = x.shape
    nb = len(mids) // 2
    geom = (C.c_int * 8)()
    slots = lib.mgdt_csp_block_tiles(mode, b, cin, cout, wd, nb, h, w, geom)
    if slots <= 0:
        raise RuntimeError('csp_block: configuration not covered')
    y = new_act(b, cout, h, w, x.dtype, x.device)
    pool = torch.empty(b * slots * cout, dtype=torch.float32, device=x.device) if want_pool else None
    marr = (C.c_void_p * len(mids))(*[m.w.data_ptr() for m in mids])
    barr = (C.c_void_p * len(mids))(*[m.bias.data_ptr() for m in mids])
    if _PROF is not None:
        es = x.element_size()
        catc = 2 * wd if mode == CSP_C3 else (3 if mode == CSP_MSPA else 2) * wd + nb * wd
        fl = 2.0 * b * h * w * ((3 * wd * wd if mode == CSP_MSPA else 0) + (10 if mode == CSP_C3 else 18) * nb * wd * wd + catc * cout)
        _META['csp_block_fwd'] = dict(shape=(b, cin, h, w, cout, wd, nb), flops=fl, bytes=float(b * h * w * (cin + cout) * es))
    _launch('csp_block_fwd', 'mgdt_csp_block_fwd', mode, vp(x), ptr(front), ptr(front_bias), marr, barr, nb, int(bool(shortcut)), ptr(back.w), ptr(back.bias),
            int(wd), act, vp(y), ptr(pool), dtype_code(x.dtype), stream())
    return y, pool, slots, (geom[6], geom[7])


def scale_channels(x, attn, out=None):
    out = like(x) if out is None else out
    _same(x, out)
    _launch('scale_channels_fwd', 'mgdt_scale_channels_fwd', vp(x), ptr(attn), vp(out), dtype_code(x.dtype), stream())
    return out


# ------------------------------------------------------------------ pools / resamplers
def sppf_pools(x, y1, y2, y3):
    _launch('sppf_pool_fwd', 'mgdt_sppf_pool_fwd', vp(x), vp(y1), vp(y2), vp(y3), dtype_code(x.dtype), stream())


def adaptive_avgpool(x, out):
    _same(x, out)
    _launch('adaptive_avgpool_fwd', 'mgdt_adaptive_avgpool_fwd', vp(x), vp(out), dtype_code(x.dtype), stream())
    return out


def bilinear(x, out):
    _same(x, out)
    _launch('bilinear_fwd', 'mgdt_bilinear_fwd', vp(x), vp(out), dtype_code(x.dtype), stream())
    return out


def nearest(x, out):
    _same(x, out)
    _launch('nearest_fwd', 'mgdt_nearest_fwd', vp(x), vp(out), dtype_code(x.dtype), stream())
    return out


def copy(x, out):
    """Strided copy with cast (channel concat, NCHW<->NHWC, fp32<->bf16)."""
    _launch('copy_fwd', 'mgdt_copy_fwd', vp(x), U8 if x.dtype == torch.uint8 else dtype_code(x.dtype), vp(out), dtype_code(out.dtype), stream())
    return out


# ------------------------------------------------------------------ ConvNeXtV2 pieces, Injection, Detect
def dwconv7_ln(x, dw_w49c, dw_b, ln_w, ln_b, eps, out=None):
    out = like(x) if out is None else out
    _launch('dwconv7_ln_fwd', 'mgdt_dwconv7_ln_fwd', vp(x), ptr(dw_w49c), ptr(dw_b), ptr(ln_w), ptr(ln_b), eps, vp(out), dtype_code(x.dtype),
                                        stream())
    return out


def dwconv7_ln_route(n, h, w, c, dtype):
    """mgdt_dwconv7_ln_route: the launch dwconv7_ln / dwconv7_ln_train would make, as a dict (family 'row8' / 'row10' / 'generic', ts, nwg, lds_bytes,
    threads).  Launches nothing and needs no device."""
    out = (C.c_int * 5)()
    L.check(L.lib().mgdt_dwconv7_ln_route(int(n), int(h), int(w), int(c), dtype_code(dtype), out), 'dwconv7_ln_route')
    return dict(family=('row8', 'row10', 'generic')[out[0]], ts=out[1], nwg=out[2], lds_bytes=out[3], threads=out[4])


def grn_scale(t, gamma):
    """scale[n,c] = gamma[c]*Nx[n,c] + 1 (fp32) for the GRN-folded pwconv2."""
    b, c = t.shape[:2]
    ws = torch.empty(b * L.GRN_SPLITS * c, dtype=torch.float32, device=t.device)
    sc = torch.empty(b, c, dtype=torch.float32, device=t.device)
    _launch('grn_stats_fwd', 'mgdt_grn_stats_fwd', vp(t), ptr(gamma), ptr(ws), ptr(sc), dtype_code(t.dtype), stream())
    return sc


FUSED_PW_CHAIN = True   # tests flip this to compare against three conv launches


def pw_chain_supported(wd, dtype):
    return FUSED_PW_CHAIN and L.lib().mgdt_pw_chain_packed_bytes(int(wd), dtype_code(dtype)) > 0


class PackedPwChain:
    """Three wd->wd 1x1 convs (BN folded) in the fragment order of mgdt_pw_chain3_fwd."""

    def __init__(self, convs, dtype):
        """convs: three (weight (wd, wd, 1, 1), conv_bias or None, bn tuple or None)."""
        wd = convs[0][0].shape[0]
        self.wd, self.dtype = wd, dtype
        self.blob = torch.empty(L.lib().mgdt_pw_chain_packed_bytes(wd, dtype_code(dtype)), dtype=torch.uint8, device=convs[0][0].device)
        f = lambda t: None if t is None else t.detach().float().contiguous()
        for i, (w, cb, bn) in enumerate(convs):
            g, b, mu, var, eps = (None, None, None, None, 0.0) if bn is None else bn
            w, cb, g, b, mu, var = f(w), f(cb), f(g), f(b), f(mu), f(var)
            L.check(L.lib().mgdt_pw_chain_pack(i, ptr(w), ptr(cb), ptr(g), ptr(b), ptr(mu), ptr(var), eps, wd, dtype_code(dtype), ptr(self.blob), stream()),
                    'pw_chain_pack')


def pw_chain3(x, pk, act, out):
    """out[:, i*wd:(i+1)*wd] = sp_i of the MSPA point-wise chain (mgdt_pw_chain3_fwd); x, out: (B, 3*wd, H, W) NHWC views."""
    if _PROF is not None:
        b, c, h, w = x.shape
        _META['pw_chain3_fwd'] = dict(shape=(b, pk.wd, h, w, pk.wd, 1, 1), flops=2.0 * b * h * w * pk.wd * pk.wd * 3, bytes=float(2 * b * h * w * c * x.element_size()))
    _launch('pw_chain3_fwd', 'mgdt_pw_chain3_fwd', vp(x), ptr(pk.blob), pk.wd, act, vp(out), dtype_code(x.dtype), stream())
    return out


FUSED_CNX_MLP = True    # tests flip this to compare against the three-launch chain


def cnx_mlp_supported(c, dtype):
    """True when the fused ConvNeXtV2 MLP kernels cover (c, dtype); otherwise callers keep the conv/GRN chain."""
    return FUSED_CNX_MLP and L.lib().mgdt_cnx_mlp_packed_bytes(int(c), dtype_code(dtype)) > 0


class PackedCnxMlp:
    """pwconv1/pwconv2 weights + biases in the fragment order of the fused MLP kernels (see mgdt_cnx_mlp_pack)."""

    def __init__(self, w1, b1, w2, b2, dtype):
        c = w2.shape[0]
        dev = w1.device
        self.c, self.dtype = c, dtype
        self.blob = torch.empty(L.lib().mgdt_cnx_mlp_packed_bytes(c, dtype_code(dtype)), dtype=torch.uint8, device=dev)
        f = lambda t: t.detach().float().contiguous()
        w1, b1, w2, b2 = f(w1), f(b1), f(w2), f(b2)
        L.check(L.lib().mgdt_cnx_mlp_pack(ptr(w1), ptr(b1), ptr(w2), ptr(b2), c, ptr(self.blob), dtype_code(dtype), stream()))


def cnx_mlp(t, res, pk, gamma, beta, out=None):
    """out = res + pwconv2(GRN(gelu(pwconv1(t)))) with the hidden map kept on chip (mgdt_cnx_mlp_fwd)."""
    b, c, h, w = t.shape
    out = like(t) if out is None else out
    ws = torch.empty(L.lib().mgdt_cnx_mlp_workspace_bytes(b, h, w, c), dtype=torch.uint8, device=t.device)
    if _PROF is not None:
        _META['cnx_mlp_fwd'] = dict(shape=(b, c, h, w, c, 1, 1), flops=2.0 * b * h * w * c * 4 * c * 3, bytes=float(4 * b * h * w * c * t.element_size()))
    _launch('cnx_mlp_fwd', 'mgdt_cnx_mlp_fwd', vp(t), vp(res), ptr(pk.blob), ptr(gamma), ptr(beta), ptr(ws), vp(out), dtype_code(t.dtype), stream())
    return out


FUSED_CNX_BLOCK = True  # tests flip this to compare against dwconv7_ln + the two-pass MLP
FUSED_CNX_TAIL = True   # ... and the IFM's closing 1x1 conv inside the last block's launch vs a launch of its own
_CNX_WS = {}            # (device, shape, lane) -> zero-initialised workspace of mgdt_cnx_block_fwd (its barrier words live across calls)
_LANE = [0]


class lane:
    """with ops.lane(i): forwards whose launches may run CONCURRENTLY with those of another lane (several captured graph instances replayed on
    different streams) - kernels that keep state in a cached workspace (the block barrier of mgdt_cnx_block_fwd) get one workspace per lane."""

    def __init__(self, i):
        self.i = int(i)

    def __enter__(self):
        self.prev, _LANE[0] = _LANE[0], self.i

    def __exit__(self, *exc):
        _LANE[0] = self.prev
        return False


def cnx_block_supported(x, dtype):
    b, c, h, w = x.shape
    return bool(FUSED_CNX_BLOCK and x.dtype == dtype and is_nhwc(x) and L.lib().mgdt_cnx_block_supported(b, h, w, c, dtype_code(dtype)))


def cnx_block_geometry(h, w, c):
    """mgdt_cnx_block_geometry: the tiling of cnx_block for an h x w map of c channels, as a dict (TH, TW, SEGS, tiles_x, tiles, NWT = 16-pixel groups
    per tile, lds_bytes).  Launches nothing and needs no device."""
    out = (C.c_int * 7)()
    L.check(L.lib().mgdt_cnx_block_geometry(int(h), int(w), int(c), out), 'cnx_block_geometry')
    return dict(zip(('TH', 'TW', 'SEGS', 'tiles_x', 'tiles', 'NWT', 'lds_bytes'), out))


def cnx_block(x, dw_w49c, dw_b, ln_w, ln_b, eps, pk, gamma, beta, out=None, tail=None, tail_act=0):
    """out = x + pwconv2(GRN(gelu(pwconv1(LayerNorm(dwconv7x7(x)))))) in one launch (mgdt_cnx_block_fwd); `tail`: PackedConv (input channels in
    `acc_order_index` order) of a 1x1 Conv+BN+act applied to that result inside the launch - `out` then has the conv's channels."""
    b, c, h, w = x.shape
    if out is None:
        out = like(x) if tail is None else new_act(b, tail.cout, h, w, x.dtype, x.device)
    if out.data_ptr() == x.data_ptr():
        raise RuntimeError('cnx_block: the output may not alias the input (tiles read their neighbours\' halo)')
    nbytes = L.lib().mgdt_cnx_block_workspace_bytes(b, h, w, c)
    key = (x.device, b, c, h, w, _LANE[0])
    ws = _CNX_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('cnx_block: run the model once before capturing it into a graph (the kernel\'s barrier words are allocated and zeroed on first use)')
        ws = _CNX_WS[key] = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
    if _PROF is not None:
        _META['cnx_block_fwd'] = dict(shape=(b, c, h, w, c, 7, 1), flops=2.0 * b * h * w * c * (4 * c * 2 + 49), bytes=float(2 * b * h * w * c * x.element_size()))
    _launch('cnx_block_fwd', 'mgdt_cnx_block_fwd', vp(x), ptr(dw_w49c), ptr(dw_b), ptr(ln_w), ptr(ln_b), float(eps), ptr(pk.blob), ptr(gamma), ptr(beta),
            None if tail is None else ptr(tail.w), None if tail is None else ptr(tail.bias), int(tail_act), ptr(ws), nbytes, vp(out), dtype_code(x.dtype), stream())
    return out


FUSED_INJECT = True     # tests flip this to compare against conv + inject


def conv1x1_inject_supported(x, cout, ga, dtype):
    return bool(FUSED_INJECT and x.dtype == dtype and ga.dtype == dtype and is_nhwc(x) and is_nhwc(ga) and
                L.lib().mgdt_conv1x1_inject_supported(x.shape[1], cout, x.shape[2], x.shape[3], ga.shape[2], ga.shape[3], dtype_code(dtype)))


def acc_order_index(c, device):
    """Input-channel permutation that turns an ordinary packed 1x1 panel into one whose K runs in the MFMA ACCUMULATOR order of the conv in
    front of it: packed channel (j*4 + g)*8 + e <- channel (2*j + e//4)*16 + 4*g + e%4."""
    k = torch.arange(c, device=device)
    j, g, e = k // 32, (k // 8) % 4, k % 8
    return (2 * j + e // 4) * 16 + 4 * g + e % 4


def conv1x1_inject_conv_supported(x, cmid, cout2, ga, dtype):
    return bool(FUSED_INJECT and FUSED_INJECT_CONV and x.dtype == dtype and ga.dtype == dtype and is_nhwc(x) and is_nhwc(ga) and
                L.lib().mgdt_conv1x1_inject_conv_supported(x.shape[1], cmid, cout2, x.shape[2], x.shape[3], ga.shape[2], ga.shape[3], dtype_code(dtype)))


def conv1x1_inject_conv(x, pk, ga, gf, pk2, act2, out, gsrc=None, pkg=None):
    """out = act2(conv1x1_2(conv1x1(x) * bilinear(h_sigmoid(ga)) + bilinear(gf))) in one launch (mgdt_conv1x1_inject_conv_fwd); pk2: the second
    conv packed with its input channels in `acc_order_index` order.  With (gsrc, pkg) instead of (ga, gf): the two global 1x1 convs (merged
    panel pkg over the 32-channel gsrc) run inside the launch as well."""
    b, _, h, w = x.shape
    _same(x, ga, gf, gsrc, out)
    if _PROF is not None:
        _META['conv1x1_inject_conv_fwd'] = dict(shape=(b, pk.cin, h, w, pk2.cout, 1, 1), flops=2.0 * b * h * w * (pk.cout * pk.cin + pk2.cout * pk2.cin),
                                                bytes=float(b * h * w * (pk.cin + pk2.cout) * x.element_size() + (2 * ga.numel() * ga.element_size() if gsrc is None else gsrc.numel() * 2)))
    _launch('conv1x1_inject_conv_fwd', 'mgdt_conv1x1_inject_conv_fwd', vp(x), ptr(pk.w), ptr(pk.bias), vp(ga), vp(gf), vp(gsrc), None if pkg is None else ptr(pkg.w),
            None if pkg is None else ptr(pkg.bias), pk.cout, ptr(pk2.w), ptr(pk2.bias), int(act2), vp(out), dtype_code(pk.dtype), stream())
    return out


FUSED_INJECT_CONV = True   # tests flip this: injection + C2f.cv1 in one launch vs two
FUSED_INJECT_GCONV = True  # ... and the injection's two global 1x1 convs inside that launch vs a launch of their own


def conv1x1_inject(x, pk, ga, gf, out=None):
    """out = conv1x1(x) * bilinear(h_sigmoid(ga)) + bilinear(gf) in one launch (mgdt_conv1x1_inject_fwd)."""
    b, _, h, w = x.shape
    if out is None:
        out = new_act(b, pk.cout, h, w, pk.dtype, x.device)
    if _PROF is not None:
        _META['conv1x1_inject_fwd'] = dict(shape=(b, pk.cin, h, w, pk.cout, 1, 1), flops=2.0 * b * h * w * pk.cout * pk.cin,
                                           bytes=float(b * h * w * (pk.cin + pk.cout) * x.element_size() + 2 * ga.numel() * ga.element_size()))
    _launch('conv1x1_inject_fwd', 'mgdt_conv1x1_inject_fwd', vp(x), ptr(pk.w), ptr(pk.bias), vp(ga), vp(gf), vp(out), dtype_code(pk.dtype), stream())
    return out


FUSED_LAF = True        # tests flip this: SimFusion_3in's cv1, bilinear and cv_fuse in one launch vs three


def laf_fuse_supported(p0, x1, x2, oc2, act1, act2, dtype):
    return bool(FUSED_LAF and p0.dtype == dtype and x1.dtype == dtype and x2.dtype == dtype and is_nhwc(p0) and is_nhwc(x1) and is_nhwc(x2) and
                x2.shape[1] == x1.shape[1] and p0.shape[0] == x1.shape[0] == x2.shape[0] and p0.shape[2:] == x1.shape[2:] and
                all(t.stride(0) % 8 == 0 and t.stride(2) % 8 == 0 and t.stride(3) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (p0, x1, x2)) and
                L.lib().mgdt_laf_fuse_supported(p0.shape[1], x1.shape[1], oc2, x1.shape[2], x1.shape[3], x2.shape[2], x2.shape[3], int(act1), int(act2),
                                                dtype_code(dtype)))


def laf_fuse(p0, x1, x2, pk1, act1, pk2, act2, out=None):
    """out = act2(conv1x1_2([act1(conv1x1_1(p0)) | x1 | bilinear(x2)])) in one launch (mgdt_laf_fuse_fwd): SimFusion_3in with cv2 = cv3 = Identity.
    pk1 / pk2: the ordinary packed panels of cv1 (c0 -> oc) and cv_fuse (3 oc -> oc); x1 may be a channel slice of the concat buffer."""
    b, oc, h, w = x1.shape
    if out is None:
        out = new_act(b, pk2.cout, h, w, pk2.dtype, x1.device)
    _same(p0, x1, x2, out)
    if _PROF is not None:
        _META['laf_fuse_fwd'] = dict(shape=(b, pk1.cin, h, w, pk2.cout, 1, 1), flops=2.0 * b * h * w * (pk1.cout * pk1.cin + pk2.cout * pk2.cin),
                                     bytes=float((b * h * w * (pk1.cin + oc + pk2.cout) + x2.numel()) * x1.element_size()))
    _launch('laf_fuse_fwd', 'mgdt_laf_fuse_fwd', vp(p0), vp(x1), vp(x2), ptr(pk1.w), ptr(pk1.bias), int(act1), ptr(pk2.w), ptr(pk2.bias), int(act2), vp(out),
            dtype_code(pk2.dtype), stream())
    return out


FUSED_SPPF = True       # tests flip this: SPPF's cv1, three max-pools and cv2 in one launch vs three


def sppf_fuse_supported(x, cm, c2, act1, act2, dtype):
    return bool(FUSED_SPPF and x.dtype == dtype and is_nhwc(x) and
                x.stride(0) % 8 == 0 and x.stride(2) % 8 == 0 and x.stride(3) % 8 == 0 and x.data_ptr() % 16 == 0 and
                L.lib().mgdt_sppf_fuse_supported(x.shape[1], cm, c2, x.shape[2], x.shape[3], int(act1), int(act2), dtype_code(dtype)))


def sppf_fuse(x, pk1, act1, pk2, act2, out=None):
    """out = act2(conv1x1_2([x0 | mp(x0) | mp(mp(x0)) | mp(mp(mp(x0)))])), x0 = act1(conv1x1_1(x)), mp = MaxPool2d(5, 1, 2), in one launch
    (mgdt_sppf_fuse_fwd).  pk1 / pk2: the ordinary packed panels of cv1 (c1 -> c1 / 2) and cv2 (2 c1 -> c2); x and out may be channel slices."""
    b, _, h, w = x.shape
    if out is None:
        out = new_act(b, pk2.cout, h, w, pk2.dtype, x.device)
    _same(x, out)
    if _PROF is not None:
        _META['sppf_fuse_fwd'] = dict(shape=(b, pk1.cin, h, w, pk2.cout, 1, 1), flops=2.0 * b * h * w * (pk1.cout * pk1.cin + pk2.cout * pk2.cin),
                                      bytes=float(b * h * w * (pk1.cin + pk2.cout) * x.element_size()))
    _launch('sppf_fuse_fwd', 'mgdt_sppf_fuse_fwd', vp(x), ptr(pk1.w), ptr(pk1.bias), int(act1), ptr(pk2.w), ptr(pk2.bias), int(act2), vp(out),
            dtype_code(pk2.dtype), stream())
    return out


# ------------------------------------------------------------------ TOODHead pieces
def groupnorm(x, gamma, beta, groups, eps, act, out=None):
    """out = act(GroupNorm(x)) on NHWC (mgdt_groupnorm_fwd)."""
    b, c = x.shape[:2]
    out = like(x) if out is None else out
    ws = torch.empty(L.lib().mgdt_groupnorm_workspace_bytes(b, c), dtype=torch.uint8, device=x.device)
    _launch('groupnorm_fwd', 'mgdt_groupnorm_fwd', vp(x), ptr(gamma), ptr(beta), groups, float(eps), act, ptr(ws), vp(out), dtype_code(x.dtype), stream())
    return out


def tood_layer_attn(feat, w1, b1, w2, b2, stacked, sums=None):
    """TaskDecomposition's layer attention as a per-(image, input channel) scale fp32 [B, C] for the reduction conv."""
    b, c, h, w = feat.shape
    sums = nc_reduce(feat) if sums is None else sums
    scale = torch.empty(b, c, dtype=torch.float32, device=feat.device)
    _launch('tood_layer_attn_fwd', 'mgdt_tood_layer_attn_fwd', ptr(sums), b, c, h * w, ptr(w1), ptr(b1), ptr(w2), ptr(b2), w1.shape[0], stacked, ptr(scale), stream())
    return scale


def dcnv2(x, offset_mask, w_gemm, bias, cout):
    b, _, h, w = x.shape
    out = new_act(b, cout, h, w, x.dtype, x.device)
    _launch('dcnv2_fwd', 'mgdt_dcnv2_fwd', vp(x), vp(offset_mask), ptr(w_gemm), ptr(bias), vp(out), dtype_code(x.dtype), stream())
    return out


def dcnv2_mfma(x, offset_mask, pk, out=None):
    """DCNv2 on the MFMA path (bf16): pk = PackedConv(weight, None, None, 3, bfloat16)."""
    b, _, h, w = x.shape
    out = new_act(b, pk.cout, h, w, x.dtype, x.device) if out is None else out
    _same(x, offset_mask, out)
    _launch('dcnv2_mfma_fwd', 'mgdt_dcnv2_mfma_fwd', vp(x), vp(offset_mask), ptr(pk.w), vp(out), dtype_code(x.dtype), stream())
    return out


def pixel_gate(x, gate, out=None):
    out = like(x) if out is None else out
    _launch('pixel_gate_fwd', 'mgdt_pixel_gate_fwd', vp(x), vp(gate), vp(out), dtype_code(x.dtype), stream())
    return out


# ---- TOODHead training (tood_train.hip) ----
def _gn_affine(y, gamma, beta, groups, eps):
    """gn_affine plus the (b, groups, 2) double (mean, rstd) view of its workspace, which gn_bwd_coef centres its sums with."""
    b, c, h, w = y.shape
    dev = y.device
    A, B = torch.empty(b, c, dtype=torch.float32, device=dev), torch.empty(b, c, dtype=torch.float32, device=dev)
    mean, rstd = torch.empty(b, groups, dtype=torch.float32, device=dev), torch.empty(b, groups, dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().mgdt_gn_affine_workspace_bytes(b, c, groups), dtype=torch.uint8, device=dev)
    _launch('gn_affine', 'mgdt_gn_affine', vp(y), ptr(gamma), ptr(beta), groups, float(eps), ptr(mean), ptr(rstd), ptr(A), ptr(B), ptr(ws), dtype_code(y.dtype), stream())
    return A, B, mean, rstd, ws[ws.numel() - b * groups * 16:].view(torch.float64).view(b, groups, 2)


def gn_affine(y, gamma, beta, groups, eps):
    """GroupNorm of the conv output y as the per-(image, channel) affine u = y*A + B; returns (A, B, mean, rstd) fp32.  The sums of y and y*y are
    kept in double (mgdt_gn_affine), as in the forward kernel."""
    return _gn_affine(y, gamma, beta, groups, eps)[:4]


def nc_affine_act_bwd(g, y, A, B, act, out=None):
    gu = like(y) if out is None else out
    _same(g, y, gu)
    _launch('nc_affine_act_bwd', 'mgdt_nc_affine_act_bwd', vp(g), vp(y), ptr(A), ptr(B), act, vp(gu), dtype_code(y.dtype), stream())
    return gu


def relu_mask(g, out_act):
    """g * (out_act > 0): backward of a fused ReLU from its OUTPUT."""
    return nc_affine_act_bwd(g, out_act, None, None, ACT_RELU)


def nc_axpby(a, sa, b=None, sb=None, shift=None, out=None):
    out = like(a) if out is None else out
    _same(a, b, out)
    _launch('nc_axpby', 'mgdt_nc_axpby', vp(a), ptr(sa), vp(b), ptr(sb), ptr(shift), vp(out), dtype_code(a.dtype), stream())
    return out


def gn_act_bwd(g, y, gamma, beta, groups, eps, act, dgamma, dbeta, accumulate=False):
    """Backward of z = act(GroupNorm(y)): returns dy; dgamma / dbeta written or accumulated."""
    b, c, h, w = y.shape
    stats = _gn_affine(y, gamma, beta, groups, eps)[4]
    gu = like(y)
    _same(g, y)
    _launch('gn_act_grad', 'mgdt_gn_act_grad', vp(g), vp(y), ptr(stats), ptr(gamma), ptr(beta), groups, act, vp(gu), dtype_code(y.dtype), stream())
    P, Q, R = (torch.empty(b, c, dtype=torch.float32, device=y.device) for _ in range(3))
    ws = torch.empty(L.lib().mgdt_gn_bwd_workspace_bytes(b, c), dtype=torch.uint8, device=y.device)
    _launch('gn_bwd_coef', 'mgdt_gn_bwd_coef', vp(gu), vp(y), ptr(stats), ptr(gamma), groups, ptr(P), ptr(Q), ptr(R), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(ws),
            dtype_code(y.dtype), stream())
    return nc_axpby(gu, P, y, Q, R, out=gu)


def pixel_gate_bwd(g, x, logit, glogit=None):
    """-> (gx, glogit); `glogit` may be a one-channel view of a wider zero-filled buffer (the padded gradient of a 1-output conv)."""
    gx = like(x)
    gl = like(logit) if glogit is None else glogit
    _same(g, x, logit, gl)
    _launch('pixel_gate_bwd', 'mgdt_pixel_gate_bwd', vp(g), vp(x), vp(logit), vp(gx), vp(gl), dtype_code(x.dtype), stream())
    return gx, gl


def tood_layer_attn_bwd(sums, dscale, hw, w1, b1, w2, b2, stacked, dw1, db1, dw2, db2, accumulate=False):
    n, c = sums.shape
    hid = w1.shape[0]
    dsums = torch.empty_like(sums)
    ws = torch.empty(L.lib().mgdt_tood_layer_attn_bwd_workspace_bytes(n, c, hid, stacked), dtype=torch.uint8, device=sums.device)
    _launch('tood_layer_attn_bwd', 'mgdt_tood_layer_attn_bwd', ptr(sums), ptr(dscale), n, c, hw, ptr(w1), ptr(b1), ptr(w2), ptr(b2), hid, stacked, ptr(dsums),
            ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), int(accumulate), ptr(ws), stream())
    return dsums


def dcn_im2col(x, om):
    b, c, h, w = x.shape
    col = new_act(b, 9 * c, h, w, x.dtype, x.device)
    _same(x, om)
    _launch('dcn_im2col', 'mgdt_dcn_im2col', vp(x), vp(om), vp(col), dtype_code(x.dtype), stream())
    return col


def dcn_col2im_bwd(gcol, x, om, gom=None):
    """-> (gx in x's dtype, gom like om: every channel written, the padding channels past the 27th with zeros)."""
    b, c, h, w = x.shape
    gx32 = torch.zeros(b, h, w, c, dtype=torch.float32, device=x.device)
    gom = like(om) if gom is None else gom
    _same(gcol, x, om, gom)
    _launch('dcn_col2im_bwd', 'mgdt_dcn_col2im_bwd', vp(gcol), vp(x), vp(om), ptr(gx32), vp(gom), dtype_code(x.dtype), stream())
    gx = gx32.permute(0, 3, 1, 2)                          # (B,C,H,W) view of the NHWC buffer = channels_last
    return (gx if x.dtype == torch.float32 else copy(gx, like(x))), gom


def ew_add_nc(a, b):
    """Sum of two small fp32 [n, c] coefficient arrays (torch element-wise on a few hundred values)."""
    return a + b


def inject(local, ga, gf, out=None):
    out = like(local) if out is None else out
    _same(local, ga, gf, out)
    _launch('inject_fwd', 'mgdt_inject_fwd', vp(local), vp(ga), vp(gf), vp(out), dtype_code(local.dtype), stream())
    return out


def detect_decode(feat, reg_max, nc, stride, a_off, y, aug=None, best=None):
    """feat (B,no,H,W) NHWC -> y[B, 4+nc, A_total] fp32 at anchor offset a_off.  aug = (scale, flip, img_w): the test-time augmentation
    epilogue (mgdt_detect_decode_aug_fwd: xywh / scale, x = img_w - x when flipped), with the best-class NMS keys into `best` (int64 [B][A_total])."""
    if aug is None:
        _launch('detect_decode_fwd', 'mgdt_detect_decode_fwd', vp(feat), reg_max, nc, float(stride), a_off, y.shape[2], ptr(y), dtype_code(feat.dtype),
                stream())
        return
    s, flip, img_w = aug
    _launch('detect_decode_aug_fwd', 'mgdt_detect_decode_aug_fwd', vp(feat), reg_max, nc, float(stride), a_off, y.shape[2], ptr(y), ptr(best), float(s),
            int(bool(flip)), float(img_w), dtype_code(feat.dtype), stream())


FUSED_DETECT_TAIL = True   # tests flip this to compare against conv + conv + decode


def detect_tail_supported(tb, tc, nc, reg_max, dtype):
    return bool(FUSED_DETECT_TAIL and dtype == torch.bfloat16 and tb.dtype == dtype and tc.dtype == dtype and is_nhwc(tb) and is_nhwc(tc) and
                L.lib().mgdt_detect_tail_supported(tb.shape[1], tc.shape[1], int(nc), int(reg_max), dtype_code(dtype)))


FUSED_DETECT_BOX3 = True   # tests flip this: the box branch's second 3x3 conv inside the Detect tail launch vs a launch of its own


def detect_tail(tb, tc, pkb, pkc, nc, stride, a_off, feat, y, best=None, pk3=None, aug=None):
    """mgdt_detect_tail_fwd: final 1x1 convs of both branches + raw map `feat` + decode into y (+ per-anchor best-class NMS keys into `best`,
    int64 [B][A], when given).  pk3: PackedConv of the box branch's second 3x3 conv - `tb` is then that conv's 16-channel input and `pkb` the
    final 1x1 packed over 32 zero-padded input channels.  aug = (scale, flip, img_w): mgdt_detect_tail_aug_fwd, the test-time augmentation
    epilogue (xywh / scale, x = img_w - x when flipped)."""
    if _PROF is not None:
        b, _, h, w = tb.shape
        _META['detect_tail_fwd'] = dict(shape=(b, tb.shape[1] + tc.shape[1], h, w, 16 + nc, 1, 1), flops=2.0 * b * h * w * (tb.shape[1] * 16 + tc.shape[1] * nc),
                                        bytes=float((tb.numel() + tc.numel() + feat.numel()) * 2 + b * (4 + nc) * h * w * 4))
    args = (vp(tb), vp(tc), ptr(pkb.w), ptr(pkb.bias), ptr(pkc.w), ptr(pkc.bias), int(nc), float(stride), int(a_off), y.shape[2], vp(feat), ptr(y), ptr(best),
            None if pk3 is None else ptr(pk3.w), None if pk3 is None else ptr(pk3.bias))
    if aug is None:
        _launch('detect_tail_fwd', 'mgdt_detect_tail_fwd', *args, stream())
    else:
        _launch('detect_tail_aug_fwd', 'mgdt_detect_tail_aug_fwd', *args, float(aug[0]), int(bool(aug[1])), float(aug[2]), stream())


# ------------------------------------------------------------------ test-time augmentation input
TTA_PAD = 0.447          # scale_img's padding value (yolo/utils/torch_utils.py:270, the ImageNet mean)


def scale_img(x, hs, ws, hp, wp, flip, dtype):
    """mgdt_scale_img_fwd: x (B, 3, H, W) image (uint8 / fp32 / bf16, any strides; uint8 / 255) -> (B, 3, hp, wp) contiguous `dtype` image: the
    (left-right flipped when `flip`) image resized to hs x ws (bilinear, align_corners=False), padded with TTA_PAD to hp x wp."""
    _need_gpu(x)
    y = torch.empty(x.shape[0], 3, hp, wp, dtype=dtype, device=x.device)
    if _PROF is not None:
        _META['scale_img_fwd'] = dict(shape=(x.shape[0], 3, x.shape[2], x.shape[3], 3, hp, wp), flops=0.0,
                                      bytes=float(x.numel() * x.element_size() + y.numel() * y.element_size()))
    _launch('scale_img_fwd', 'mgdt_scale_img_fwd', vp(x), U8 if x.dtype == torch.uint8 else dtype_code(x.dtype), int(bool(flip)), int(hs), int(ws),
            float(TTA_PAD), vp(y), dtype_code(dtype), stream())
    return y


# ------------------------------------------------------------------ NMS
NMS_USE_BEST_KEYS = True      # tests flip this to compare against the scan of the score rows (nms_best_kernel)


def attach_best_keys(y, best):
    """The Detect tail kernel left the NMS key of every anchor's best class in `best`; remember it on the prediction tensor together with
    the tensor's version, so that `nms(y)` can skip its own scan over the nc score rows as long as nobody wrote into y since.  A prediction made
    under torch.inference_mode() has no version counter, so a later write into it could not be seen: it carries no keys and NMS scans its rows."""
    if y.is_inference():
        return
    y._mgdt_best = (best, y._version)


def _best_keys_of(pred, b, a):
    bk = getattr(pred, '_mgdt_best', None)
    if not NMS_USE_BEST_KEYS or bk is None or pred.is_inference():
        return None
    best, ver = bk
    if ver != pred._version or best.shape != (b, a) or best.dtype != torch.int64 or best.device != pred.device or not best.is_contiguous():
        return None
    return best
def nms(pred, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh):
    """pred (B, 4+nc, A) fp32 cuda contiguous -> (out [B,max_det,6], kept_anchor [B,max_det] int32, counts [B] int32)."""
    _need_gpu(pred)
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        raise RuntimeError('nms: prediction must be a contiguous float32 tensor')
    b, ch, a = pred.shape
    nc = ch - 4
    lib = L.lib()
    ml = 1 if (multi_label and nc > 1) else 0
    ws_bytes = lib.mgdt_nms_workspace_bytes(b, nc, a, ml, max_nms)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=pred.device)
    # rows past counts[i] are never written (and never read: callers slice by counts); counts[i] is written for every image
    out = torch.empty(b, max_det, 6, dtype=torch.float32, device=pred.device)
    kept = torch.empty(b, max_det, dtype=torch.int32, device=pred.device)
    counts = torch.empty(b, dtype=torch.int32, device=pred.device)
    cls_t = None
    if classes is not None:
        cls_t = torch.as_tensor(list(classes), dtype=torch.int32).to(pred.device)
    best = None if ml else _best_keys_of(pred, b, a)
    _launch('nms_fwd', 'mgdt_nms_fwd', ptr(pred), b, nc, a, float(conf_thres), float(iou_thres), ptr(cls_t), 0 if cls_t is None else cls_t.numel(),
                             int(bool(agnostic)), ml, max_det, max_nms, float(max_wh), ptr(out), ptr(kept), ptr(counts), ptr(best), ptr(ws),
                             ws_bytes, stream())
    return out, kept, counts


def nms_masks(pred, nm, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms, max_wh):
    """pred (B, 4+nc+nm, A) fp32 cuda contiguous -> (out [B,max_det,6+nm], kept_anchor [B,max_det] int32, counts [B] int32): mgdt_nms_masks_fwd,
    the selection of `nms` on rows 0 .. 4+nc with the kept anchors' nm mask coefficients behind the six detection columns."""
    _need_gpu(pred)
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        raise RuntimeError('nms: prediction must be a contiguous float32 tensor')
    b, ch, a = pred.shape
    nc = ch - 4 - nm
    if nm < 1 or nc < 1:
        raise RuntimeError(f'nms_masks: {ch} prediction rows cannot hold 4 box rows, classes and nm={nm} mask coefficients')
    lib = L.lib()
    ml = 1 if (multi_label and nc > 1) else 0
    ws_bytes = lib.mgdt_nms_workspace_bytes(b, nc, a, ml, max_nms)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=pred.device)
    out = torch.empty(b, max_det, 6 + nm, dtype=torch.float32, device=pred.device)
    kept = torch.empty(b, max_det, dtype=torch.int32, device=pred.device)
    counts = torch.empty(b, dtype=torch.int32, device=pred.device)
    cls_t = None
    if classes is not None:
        cls_t = torch.as_tensor(list(classes), dtype=torch.int32).to(pred.device)
    best = None if ml else _best_keys_of(pred, b, a)
    if _PROF is not None:
        _META['nms_masks_fwd'] = dict(shape=(b, nc, nm, a, max_det), flops=0.0, bytes=float(b * (4 + nc) * a * 4))
    _launch('nms_masks_fwd', 'mgdt_nms_masks_fwd', ptr(pred), b, nc, nm, a, float(conf_thres), float(iou_thres), ptr(cls_t),
            0 if cls_t is None else cls_t.numel(), int(bool(agnostic)), ml, max_det, max_nms, float(max_wh), ptr(out), ptr(kept), ptr(counts), ptr(best),
            ptr(ws), ws_bytes, stream())
    return out, kept, counts


# ------------------------------------------------------------------ instance segmentation (Segment head, Proto, masks)
class PackedDeconv2x2:
    """The four 1x1 panels of one nn.ConvTranspose2d(cin, cout, 2, 2, 0) (weight (cin, cout, 2, 2)): panel 2*dy + dx = W[:, :, dy, dx]^T."""
    __slots__ = ('panels', 'ptrs', 'bias', 'cin', 'cout', 'dtype', '__weakref__')

    def __init__(self, weight, bias, dtype):
        check_deconv2x2(weight.shape[2:], (2, 2), (0, 0), 1)
        w = weight.detach().float()
        self.cin, self.cout, self.dtype = w.shape[0], w.shape[1], dtype
        self.panels = [PackedConv(w[:, :, dy, dx].t().reshape(self.cout, self.cin, 1, 1), bias, None, 1, dtype) for dy in (0, 1) for dx in (0, 1)]
        self.ptrs = (C.c_void_p * 4)(*[p.w.data_ptr() for p in self.panels])
        self.bias = self.panels[0].bias


def check_deconv2x2(kernel_size, stride, padding, groups, output_padding=(0, 0), dilation=(1, 1)):
    """Only the geometry of Proto.upsample is built (kernel 2, stride 2, padding 0, one group): anything else raises before a launch."""
    if (tuple(kernel_size) != (2, 2) or tuple(stride) != (2, 2) or tuple(padding) != (0, 0) or groups != 1 or tuple(output_padding) != (0, 0)
            or tuple(dilation) != (1, 1)):
        raise RuntimeError(f'transposed convolution: only kernel 2, stride 2, padding 0, groups 1 is built (Proto.upsample), got kernel {tuple(kernel_size)} '
                           f'stride {tuple(stride)} padding {tuple(padding)} groups {groups}')


def deconv2x2(x, pk, out=None):
    """mgdt_deconv2x2_fwd: x (B, cin, H, W) NHWC -> (B, cout, 2H, 2W) NHWC = conv_transpose2d(x, W, b, stride 2)."""
    _need_gpu(x)
    b, c, h, w = x.shape
    if c != pk.cin or x.dtype != pk.dtype:
        raise RuntimeError(f'deconv2x2: panels are packed for {pk.cin} channels of {pk.dtype}, the input has {c} of {x.dtype}')
    if not conv_can_mfma(x, pk.cin, pk.cout, 1, 1, 1, pk.dtype):
        raise RuntimeError(f'deconv2x2: needs an NHWC input with cin % {8 if pk.dtype == torch.bfloat16 else 4} == 0 and cout % 4 == 0 (cin {pk.cin}, cout {pk.cout})')
    if out is None:
        out = new_act(b, pk.cout, 2 * h, 2 * w, pk.dtype, x.device)
    _same(x, out)
    if _PROF is not None:
        es = x.element_size()
        _META['deconv2x2_fwd'] = dict(shape=(b, pk.cin, h, w, pk.cout, 2, 2), flops=2.0 * b * h * w * 4 * pk.cout * pk.cin,
                                      bytes=float(b * h * w * (pk.cin + 4 * pk.cout) * es + 4 * pk.cin * pk.cout * es))
    _launch('deconv2x2_fwd', 'mgdt_deconv2x2_fwd', vp(x), pk.ptrs, ptr(pk.bias), vp(out), dtype_code(pk.dtype), stream())
    return out


class _DeconvPanel:
    """One phase panel of PackedDeconv2x2Live: the fields repack_all() refreshes."""
    __slots__ = ('w', 'bias', 'src', 'epoch', '__weakref__')


class PackedDeconv2x2Live:
    """The four 1x1 panels of one nn.ConvTranspose2d(cin, cout, 2, 2, 0), packed straight from the live (cin, cout, 2, 2) weight
    (mgdt_conv_pack_deconv2x2), so under the trainer repack_all() refreshes them in place like every other panel (PackedDeconv2x2 packs from
    transposed copies, which are never registered).  Same fields as PackedDeconv2x2: ops.deconv2x2 takes either."""
    __slots__ = ('panels', 'ptrs', 'bias', 'cin', 'cout', 'dtype', '__weakref__')

    def __init__(self, weight, bias, dtype):
        check_deconv2x2(weight.shape[2:], (2, 2), (0, 0), 1)
        if bias is None:
            raise RuntimeError('transposed convolution: only the form with a bias is built')
        lib = L.lib()
        w = weight.detach().float().contiguous()
        cb = bias.detach().float().contiguous()
        _need_gpu(w)
        self.cin, self.cout, self.dtype = w.shape[0], w.shape[1], dtype
        code = dtype_code(dtype)
        nbytes = lib.mgdt_conv_packed_bytes(self.cin, self.cout, 1, code)
        self.panels = []
        for ph in range(4):
            pn = _DeconvPanel()
            pn.w = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
            pn.bias = torch.empty((self.cout + 15) // 16 * 16, dtype=torch.float32, device=w.device)
            pn.src, pn.epoch = None, None
            _launch('conv_pack', 'mgdt_conv_pack_deconv2x2', ptr(w), ptr(cb), self.cin, self.cout, ph, code, ptr(pn.w), ptr(pn.bias), stream())
            _register_pack(pn, (w, cb, None, None, None, None, 0.0, self.cin, self.cout, 1, code, 10 + ph))
            self.panels.append(pn)
        self.ptrs = (C.c_void_p * 4)(*[pn.w.data_ptr() for pn in self.panels])
        self.bias = self.panels[0].bias

    @property
    def epoch(self):
        """the oldest panel's stamp (None: not refreshable in place) - what pack_is_current() compares"""
        ep = [pn.epoch for pn in self.panels]
        return None if any(e is None for e in ep) else min(ep)


# The ConvTranspose2d layer's reverse pass: dx and dW in one launch each (mgdt_deconv2x2_dgrad / mgdt_deconv2x2_wgrad) or composed from four strided-view
# 1x1 launches per gradient.  None: per (cin, cout) class, the one-launch route where tools/yolov6_bench.py measured it faster than the composed one by more
# than the run-to-run spread of the two; True: wherever the kernels cover the case (tests, the tool); False: composed everywhere.
DECONV_BWD_FUSED = None
DECONV_DX_FUSED_CLASSES = ((32, 32),)
DECONV_DW_FUSED_CLASSES = ((32, 32), (64, 64), (128, 128))


def _deconv_fused(classes, cin, cout):
    return (int(cin), int(cout)) in classes if DECONV_BWD_FUSED is None else bool(DECONV_BWD_FUSED)


def _deconv_bwd_views(small, dy):
    if small.shape[0] != dy.shape[0] or dy.shape[2] != 2 * small.shape[2] or dy.shape[3] != 2 * small.shape[3]:
        raise RuntimeError(f'transposed convolution (kernel 2, stride 2): dy {tuple(dy.shape)} does not match the input {tuple(small.shape)}')


def _deconv_vec_ok(t):
    return (is_nhwc(t) and t.shape[1] % 4 == 0 and t.stride(0) % 4 == 0 and t.stride(2) % 4 == 0 and t.stride(3) % 4 == 0
            and t.data_ptr() % (4 * t.element_size()) == 0)


def deconv2x2_dgrad(dy, weight, dx, accumulate=False, r2=None):
    """dx (+)= d loss / d x of conv_transpose2d(x, weight (cin, cout, 2, 2), stride 2) [+ r2]: dx[b, y, x, ci] = sum_{ky, kx, co} W[ci, co, ky, kx] *
    dy[b, 2y+ky, 2x+kx, co].  One launch (mgdt_deconv2x2_dgrad, K = 4 cout over the 2x2 gather of dy), or the four phases as strided-view 1x1
    convolutions over panels packed from the live weight, the later three accumulating (DECONV_BWD_FUSED chooses; a case the one-launch kernel does
    not take composes)."""
    _deconv_bwd_views(dx, dy)
    _same(dy, dx, r2)
    cin, cout = weight.shape[0], weight.shape[1]
    if dx.shape[1] != cin or dy.shape[1] != cout or tuple(weight.shape[2:]) != (2, 2) or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise RuntimeError(f'deconv2x2_dgrad: weight {tuple(weight.shape)} {weight.dtype} does not fit dy {tuple(dy.shape)} -> dx {tuple(dx.shape)}')
    fits = ((cout + 15) // 16 * 16 + 4) * 256 <= 65536                  # w's LDS tile for 16 input channels (cout <= 240)
    vec = _deconv_vec_ok(dy) and is_nhwc(dx) and cin % 4 == 0 and (r2 is None or is_nhwc(r2))
    if _deconv_fused(DECONV_DX_FUSED_CLASSES, cin, cout) and fits and vec:      # a case the kernel does not take composes, like the block kernels' refusals
        if _PROF is not None:
            es = dy.element_size()
            _META['deconv2x2_dgrad'] = dict(shape=(dx.shape[0], cin, dx.shape[2], dx.shape[3], cout, 2, 2), flops=2.0 * dy.numel() * cin,
                                            bytes=float((dy.numel() + dx.numel() * (1 + bool(accumulate) + (r2 is not None))) * es + weight.numel() * 4))
        _launch('deconv2x2_dgrad', 'mgdt_deconv2x2_dgrad', vp(dy), ptr(weight), vp(dx if accumulate else None), vp(r2), vp(dx), dtype_code(dy.dtype), stream())
        return dx
    pks = None
    if is_nhwc(dx) and cin % 4 == 0 and conv_can_mfma(dy[:, :, ::2, ::2], cout, cin, 1, 1, 1, dy.dtype) and (r2 is None or is_nhwc(r2)):
        pks = _deconv_dgrad_panels(weight, dy.dtype)
    for ph in range(4):
        ky, kx = ph >> 1, ph & 1
        sub = dy[:, :, ky::2, kx::2]
        if pks is not None:            # the MFMA 1x1 convolution over the phase view, its panel packed from the live weight (4 launches in all)
            res = [t for t in (dx if (accumulate or ph) else None, r2 if ph == 0 else None) if t is not None]
            conv2d(sub, pks[ph], 1, ACT_NONE, out=dx, r1=(res + [None, None])[0], r2=(res + [None, None])[1])
        else:                          # shapes the MFMA kernel does not take (e.g. bf16 with cout % 8): the direct data-gradient kernel on a transposed copy
            conv_dgrad(sub, weight.detach()[:, :, ky, kx].t().contiguous(), 1, 1, dx, accumulate=bool(accumulate or ph), r2=r2 if ph == 0 else None)
    return dx


class _PackedDeconvDgrad:
    """Panel of one phase of the layer's composed data gradient (a 1x1 convolution cout -> cin), packed from the live (cin, cout, 2, 2) weight
    (mgdt_conv_pack_deconv2x2_dgrad) and refreshed by repack_all(); same fields as PackedConv."""
    __slots__ = ('w', 'bias', 'k', 'cin', 'cout', 'dtype', 'direct', 'groups', 'key', 'owner', 'src', 'epoch', '__weakref__')

    def __init__(self, weight, phase, dtype, key):
        import weakref
        self.owner = weakref.ref(weight)
        cin, cout = weight.shape[0], weight.shape[1]
        code = dtype_code(dtype)
        self.k, self.cin, self.cout, self.dtype, self.direct, self.groups, self.key = 1, cout, cin, dtype, False, 1, key       # a conv cout -> cin
        self.w = torch.empty(L.lib().mgdt_conv_packed_bytes(cout, cin, 1, code), dtype=torch.uint8, device=weight.device)
        self.bias = torch.empty((cin + 15) // 16 * 16, dtype=torch.float32, device=weight.device)
        self.src, self.epoch = None, None
        wf = weight.detach().float().contiguous()
        _launch('conv_pack', 'mgdt_conv_pack_deconv2x2_dgrad', ptr(wf), cin, cout, phase, code, ptr(self.w), ptr(self.bias), stream())
        if wf.data_ptr() == weight.data_ptr():
            _register_pack(self, (wf, None, None, None, None, None, 0.0, cin, cout, 1, code, 14 + phase))


_DECONV_DGRAD_PK = {}


def _deconv_dgrad_panels(weight, dtype):
    """the four phase panels of `weight`, rebuilt only when the weight changed and repack_all() did not refresh them (as conv_dgrad keeps its panels)"""
    key = (PARAM_EPOCH[0], version_of(weight), dtype)
    ck = (weight.data_ptr(), dtype)
    pks = _DECONV_DGRAD_PK.get(ck)
    if pks is not None and pks[0].owner() is weight and pks[0].key[1:] == key[1:] and all(pack_is_current(q) for q in pks):
        for q in pks:
            q.key = key
    if pks is None or pks[0].owner() is not weight or pks[0].key != key:
        pks = _DECONV_DGRAD_PK[ck] = [_PackedDeconvDgrad(weight, ph, dtype, key) for ph in range(4)]
    return pks


def deconv2x2_wgrad(x, dy, dw, accumulate=False):
    """dw (cin, cout, 2, 2) fp32 contiguous (+)= sum_{b, y, x} x[b, y, x, ci] * dy[b, 2y+ky, 2x+kx, co] - the parameter's own layout.  One launch
    (mgdt_deconv2x2_wgrad) whose per-split partial sums join the batched final sum inside `with defer_wgrad():`, bit-identical to the immediate
    form; or - DECONV_BWD_FUSED off - four strided-view 1x1 weight-gradient launches into a scratch (4, cout, cin) and one permuting copy (their
    final sums are taken at once: the other pending sums stay pending)."""
    _deconv_bwd_views(x, dy)
    _same(x, dy)
    cin, cout = x.shape[1], dy.shape[1]
    if tuple(dw.shape) != (cin, cout, 2, 2) or dw.dtype != torch.float32 or not dw.is_contiguous():
        raise RuntimeError(f'deconv2x2_wgrad: dw must be a contiguous fp32 ({cin}, {cout}, 2, 2) tensor, got {tuple(dw.shape)} {dw.dtype}')
    if _deconv_fused(DECONV_DW_FUSED_CLASSES, cin, cout) and _deconv_vec_ok(x) and _deconv_vec_ok(dy):      # views the kernel's vector loads do not take compose
        lib = L.lib()
        ws = torch.empty(lib.mgdt_deconv2x2_wgrad_workspace_bytes(cin, cout), dtype=torch.uint8, device=x.device)
        if _PROF is not None:
            _META['deconv2x2_wgrad'] = dict(shape=(x.shape[0], cin, x.shape[2], x.shape[3], cout, 2, 2), flops=2.0 * dy.numel() * cin,
                                            bytes=float((x.numel() + dy.numel()) * x.element_size() + ws.numel()))
        if _WGRAD_DEFER[0] > 0 and accumulate:
            flush_wgrad()                                  # an accumulating gradient must see the value the pending jobs will write
        defer = _WGRAD_DEFER[0] > 0 and not accumulate
        _launch('deconv2x2_wgrad', 'mgdt_deconv2x2_wgrad', vp(x), vp(dy), None if defer else ptr(dw), int(accumulate), ptr(ws), dtype_code(dy.dtype), stream())
        if defer:
            _WGRAD_PENDING.append((ws, dw, dw.numel(), lib.mgdt_deconv2x2_wgrad_splits(cin, cout)))
        return dw
    if _WGRAD_DEFER[0] > 0 and accumulate:
        flush_wgrad()
    scratch = torch.empty((4, cout, cin, 1, 1), dtype=torch.float32, device=x.device)
    for ph in range(4):
        conv_wgrad(x, dy[:, :, ph >> 1::2, ph & 1::2], 1, 1, scratch[ph], defer=False)
    perm = scratch.view(2, 2, cout, cin).permute(3, 2, 0, 1)          # (cin, cout, ky, kx) view of the four (cout, cin) matrices
    if accumulate:
        return add(dw, copy(perm, torch.empty_like(dw)), out=dw)
    return copy(perm, dw)


def seg_concat(y, mcs):
    """mgdt_seg_concat_fwd: y (B, 4+nc, A) fp32 + per-level cv4 maps (B, nm, h, w) NHWC -> (B, 4+nc+nm, A) fp32 (torch.cat([y, mc], 1) of
    head.py:212 with mc = cat of the levels' .view(bs, nm, -1))."""
    _need_gpu(y)
    b, rows, a = y.shape
    nm = mcs[0].shape[1]
    _same(*mcs)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise RuntimeError('seg_concat: the prediction must be a contiguous float32 tensor')
    out = torch.empty(b, rows + nm, a, dtype=torch.float32, device=y.device)
    arr, keep = _view_array(mcs)
    if _PROF is not None:
        _META['seg_concat_fwd'] = dict(shape=(b, rows, nm, a), flops=0.0, bytes=float(b * a * (2 * rows * 4 + nm * (4 + mcs[0].element_size()))))
    _launch('seg_concat_fwd', 'mgdt_seg_concat_fwd', ptr(y), b, rows, a, arr, len(mcs), nm, ptr(out), dtype_code(mcs[0].dtype), stream())
    return out


# ------------------------------------------------------------------ pose estimation (Pose head, keypoint decode, post-NMS scaling)
POSE_PAD_MFMA = True     # tests / tools/pose_bench.py flip this: Pose.cv4 convolutions whose channel counts the MFMA kernel does not take (51) run on it over
#                          zero-padded panels (56 / 52 channels) vs through mgdt_conv2d_direct_fwd


def pose_concat(y, kps, strides, nk, ndim):
    """mgdt_pose_concat_fwd: y (B, 4+nc, A) fp32 + per-level cv4 maps (B, >= nk, h, w) NHWC + the levels' strides (host floats) ->
    (cat(y, kpts_decode(kpt)) (B, 4+nc+nk, A) fp32, kpt (B, nk, A) fp32 raw) (head.py:236-253, non-export decode)."""
    _need_gpu(y)
    b, rows, a = y.shape
    _same(*kps)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise RuntimeError('pose_concat: the prediction must be a contiguous float32 tensor')
    if len(strides) != len(kps) or any(t.shape[1] < nk or not is_nhwc(t) for t in kps):
        raise RuntimeError(f'pose_concat: one NHWC map with at least nk={nk} channels and one stride per level expected')
    out = torch.empty(b, rows + nk, a, dtype=torch.float32, device=y.device)
    raw = torch.empty(b, nk, a, dtype=torch.float32, device=y.device)
    arr, keep = _view_array(kps)
    st = (C.c_float * len(kps))(*[float(s) for s in strides])
    if _PROF is not None:
        _META['pose_concat_fwd'] = dict(shape=(b, rows, nk, a), flops=0.0, bytes=float(b * a * (2 * rows * 4 + nk * (8 + kps[0].element_size()))))
    _launch('pose_concat_fwd', 'mgdt_pose_concat_fwd', ptr(y), b, rows, a, arr, st, len(kps), int(nk), int(ndim), ptr(out), ptr(raw), dtype_code(kps[0].dtype),
            stream())
    return out, raw


def pose_scale_meta(img1_shape, img0_shape, normalize=False):
    """Host side of mgdt_pose_scale_fwd for one image: [gain, kpt_pad_x, kpt_pad_y, h0, w0, box_pad_x, box_pad_y, normalize] with the gain and the
    fractional padding of scale_coords (ops.py:653-655) and the rounded padding of scale_boxes (ops.py:104-105), in Python floats like the reference."""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    return [gain, pad[0], pad[1], float(img0_shape[0]), float(img0_shape[1]), float(round(pad[0] - 0.1)), float(round(pad[1] - 0.1)), float(bool(normalize))]


def pose_scale(rows, counts_dev, meta, nk, ndim, lead=6):
    """mgdt_pose_scale_fwd, in place: rows (B, max_det, lead+nk) fp32 contiguous, counts (B,) int32 on the device, meta (B, 8) fp32 on the device (one
    `pose_scale_meta` row per image).  lead = 6: boxes scaled, clipped and rounded, keypoints scaled and clipped; lead = 0: keypoints only."""
    _need_gpu(rows)
    if rows.dtype != torch.float32 or rows.dim() != 3 or not rows.is_contiguous() or rows.shape[2] != lead + nk:
        raise RuntimeError(f'pose_scale: rows must be a contiguous float32 (B, max_det, {lead} + nk={nk}) tensor, got {tuple(rows.shape)} {rows.dtype}')
    b, md, _ = rows.shape
    if (counts_dev.dtype != torch.int32 or counts_dev.numel() != b or not counts_dev.is_contiguous() or meta.dtype != torch.float32 or tuple(meta.shape) != (b, 8)
            or not meta.is_contiguous()):
        raise RuntimeError('pose_scale: counts (B,) int32 and meta (B, 8) float32 expected')
    _need_gpu(counts_dev)
    _need_gpu(meta)
    if md == 0:
        return rows
    if _PROF is not None:
        _META['pose_scale_fwd'] = dict(shape=(b, md, lead, nk), flops=0.0, bytes=float(2 * rows.numel() * 4))
    _launch('pose_scale_fwd', 'mgdt_pose_scale_fwd', ptr(rows), ptr(counts_dev), ptr(meta), b, md, int(lead), int(nk), int(ndim), stream())
    return rows


SEG_MASK_SKIP = True     # tests flip this: (detection, tile) pairs outside the detection's box store zeros without the GEMM vs computing every pair
MASK_MODES = ('process_mask', 'process_mask_up', 'process_mask_upsample', 'process_mask_native')


def seg_mask_plan(mode, mh, mw, shape):
    """Host-side parameters of one mgdt_seg_masks_fwd launch for the reference routine `mode` (yolo/utils/ops.py:560-636) on mh x mw protos and
    the image shape (h, w) the routine is given: (top, left, win_h, win_w, out_h, out_w, crop_before, box_sx, box_sy, crop_after)."""
    import numpy as np
    ih, iw = int(shape[0]), int(shape[1])
    if mode not in MASK_MODES:
        raise RuntimeError(f'mask mode {mode!r} is not one of {MASK_MODES}')
    if ih < 1 or iw < 1:
        raise RuntimeError(f'mask assembly: image shape {tuple(shape)}')
    if mode in ('process_mask', 'process_mask_up'):
        # `downsampled_bboxes[:, 0] *= mw / iw`: a Python double, rounded to the tensor's float32 for the multiplication
        sx, sy = float(np.float32(mw / iw)), float(np.float32(mh / ih))
        oh, ow = (mh, mw) if mode == 'process_mask' else (ih, iw)
        return 0, 0, mh, mw, oh, ow, 1, sx, sy, 0
    if mode == 'process_mask_upsample':
        return 0, 0, mh, mw, ih, iw, 0, 1.0, 1.0, 1
    gain = min(mh / ih, mw / iw)
    pad = (mw - iw * gain) / 2, (mh - ih * gain) / 2
    top, left = int(pad[1]), int(pad[0])
    bottom, right = int(mh - pad[1]), int(mw - pad[0])
    if bottom <= top or right <= left:
        raise RuntimeError(f'process_mask_native: the letter-box window of {mh}x{mw} protos for shape {tuple(shape)} is empty')
    return top, left, bottom - top, right - left, ih, iw, 0, 1.0, 1.0, 1


def seg_skip_share(rows, counts, mh, mw, shape, mode):
    """Host-side count of the (detection, tile) pairs mgdt_seg_masks_fwd skips for these NMS rows (a CPU tensor (B, max_det, 6+nm)) and counts:
    (skipped, all pairs), by the kernel's own rule in float32 on the tile grid of mgdt_seg_mask_geometry.  Reporting / tests only."""
    import numpy as np
    f = np.float32
    top, left, wh, ww, oh, ow, cb, bsx, bsy, ca = seg_mask_plan(mode, mh, mw, shape)
    geom = (C.c_int * 4)()
    if L.lib().mgdt_seg_mask_geometry(wh, ww, oh, ow, geom) != 1:
        raise RuntimeError(f'mask assembly: {wh}x{ww} -> {oh}x{ow} is not covered')
    th, tw, ny, nx = list(geom)

    def tap(scale, o, n_in):
        s = max(f(f(scale) * f(f(o) + f(0.5))) - f(0.5), f(0))
        i0 = min(int(s), n_in - 1)
        return i0, i0 + (1 if i0 < n_in - 1 else 0)
    sy, sx = f(wh) / f(oh), f(ww) / f(ow)
    r = rows.detach().float().cpu().numpy()
    skipped = pairs = 0
    for ty in range(ny):
        oy0, oy1 = ty * th, min(ty * th + th, oh)
        ry0, ry1 = tap(sy, oy0, wh)[0], tap(sy, oy1 - 1, wh)[1]
        for tx in range(nx):
            ox0, ox1 = tx * tw, min(tx * tw + tw, ow)
            rx0, rx1 = tap(sx, ox0, ww)[0], tap(sx, ox1 - 1, ww)[1]
            for b, n in enumerate(counts):
                x1, y1, x2, y2 = (r[b, :n, k] for k in range(4))
                dead = np.zeros(n, bool)
                if ca:
                    dead |= (f(ox1 - 1) < x1) | ~(f(ox0) < x2) | (f(oy1 - 1) < y1) | ~(f(oy0) < y2)
                if cb:
                    dead |= ((f(left + rx1) < x1 * f(bsx)) | ~(f(left + rx0) < x2 * f(bsx)) | (f(top + ry1) < y1 * f(bsy)) | ~(f(top + ry0) < y2 * f(bsy)))
                skipped += int(dead.sum())
                pairs += int(n)
    return skipped, pairs


def seg_masks(protos, rows, counts_dev, counts, shape, mode, out_dtype=torch.uint8, out=None):
    """mgdt_seg_masks_fwd: the masks of a whole batch in one launch.  protos (B, nm, mh, mw) NHWC activation (fp32 / bf16), rows (B, max_det, 6+nm)
    fp32 + counts_dev (B,) int32 as `nms_masks` returns them, counts = the host copy of counts_dev -> (sum(counts), H, W) 0 / 1 masks of
    `out_dtype` (uint8 or float32), image after image.  `out`: a caller's buffer of at least that many elements (tests: guard bytes behind)."""
    b, nm, mh, mw = protos.shape
    if rows.dim() != 3 or rows.shape[0] != b or rows.shape[2] != 6 + nm or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise RuntimeError(f'mask assembly: rows must be a contiguous float32 (B={b}, max_det, 6+nm={6 + nm}) tensor for protos with nm={nm} channels, '
                           f'got {tuple(rows.shape)} {rows.dtype}')
    if nm != 32:
        raise RuntimeError(f'mask assembly: the kernel is built for nm = 32 mask coefficients, got {nm}')
    if out_dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f'mask assembly: masks are uint8 or float32, not {out_dtype}')
    _need_gpu(protos)
    _need_gpu(rows)
    if not is_nhwc(protos):
        raise RuntimeError('mask assembly: protos must be NHWC-backed (the Proto module output, or ops.copy into ops.new_act)')
    counts = [int(c) for c in counts]
    if len(counts) != b or any(c < 0 or c > rows.shape[1] for c in counts):
        raise RuntimeError(f'mask assembly: counts {counts} do not fit (B={b}, max_det={rows.shape[1]})')
    top, left, wh, ww, oh, ow, cb, sx, sy, ca = seg_mask_plan(mode, mh, mw, shape)
    total = sum(counts)
    if out is None:
        out = torch.empty(total, oh, ow, dtype=out_dtype, device=protos.device)
    elif out.dtype != out_dtype or out.numel() < total * oh * ow or not out.is_contiguous():
        raise RuntimeError('mask assembly: `out` must be a contiguous buffer of out_dtype holding sum(counts) x H x W elements')
    if total == 0:
        return out
    offs = [0] * b
    for i in range(1, b):
        offs[i] = offs[i - 1] + counts[i - 1]
    offsets = torch.tensor(offs, dtype=torch.int32).to(protos.device, non_blocking=True)
    if _PROF is not None:
        _META['seg_masks_fwd'] = dict(shape=(b, total, mh, mw, oh, ow), flops=2.0 * total * wh * ww * nm,
                                      bytes=float(total * oh * ow * out.element_size() + (total + 15) // 16 * wh * ww * nm * protos.element_size()))
    _launch('seg_masks_fwd', 'mgdt_seg_masks_fwd', vp(protos), ptr(rows), ptr(counts_dev), ptr(offsets), rows.shape[1], nm, top, left, wh, ww, oh, ow,
            cb, sx, sy, ca, 0 if SEG_MASK_SKIP else 1, ptr(out), 1 if out_dtype == torch.uint8 else 0, dtype_code(protos.dtype), stream())
    return out


def val_match(det, ndet, labels, nlab, iouv):
    """Validator matching for a batch (mgdt_val_match_fwd): det (B, max_det, 6) fp32 + ndet (B,) int32 as returned by `nms`, labels
    (B, max_lab, 5) fp32 [cls, x1, y1, x2, y2] + nlab (B,) int32, iouv (T,) fp32 -> correct (B, max_det, T) bool."""
    _need_gpu(det)
    b, md, _ = det.shape
    ml = labels.shape[1]
    correct = torch.empty(b, md, iouv.numel(), dtype=torch.uint8, device=det.device)
    _launch('val_match_fwd', 'mgdt_val_match_fwd', ptr(det), ptr(ndet), b, md, ptr(labels), ptr(nlab), ml, ptr(iouv), iouv.numel(), ptr(correct), stream())
    return correct.view(torch.bool)


COUNT_SLOTS = 10                   # == MGDT_COUNT_SLOTS: images, sum t, sum p, sum t^2, sum t*p, sum (t-p)^2, sum |t-p|, TP, FP, FN
VAL_CONFUSION_MAX_DET, VAL_CONFUSION_MAX_LAB, VAL_CONFUSION_MAX_NC = 1024, 256, 4096


def val_confusion(det, ndet, labels, nlab, nc, matrix=None, counts=None, cm_conf=0.25, cm_iou=0.45, cnt_conf=0.25, cnt_iou=0.5, trunc_labels=True):
    """Confusion matrix and counting metrics of a batch in one launch (mgdt_val_confusion_fwd): det (B, max_det, 6) fp32 + ndet (B,) int32 as returned
    by `nms`, labels (B, max_lab, 5) fp32 [cls, x1, y1, x2, y2] + nlab (B,) int32, in one pixel frame.  `matrix` ((nc+1, nc+1) int32, row = predicted
    class, column = true class, nc = background) and `counts` ((nc, COUNT_SLOTS) int64) are ADDED to on the device; either may be None, not both.
    Returns (matrix, counts)."""
    _need_gpu(det)
    _need_gpu(labels)
    nc = int(nc)
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous():
        raise RuntimeError(f'val_confusion: det must be a contiguous float32 (B, max_det, 6) tensor, got {tuple(det.shape)} {det.dtype}')
    b, md = det.shape[0], det.shape[1]
    if labels.dim() != 3 or labels.shape[0] != b or labels.shape[2] != 5 or labels.dtype != torch.float32 or not labels.is_contiguous():
        raise RuntimeError(f'val_confusion: labels must be a contiguous float32 (B={b}, max_lab, 5) tensor, got {tuple(labels.shape)} {labels.dtype}')
    _i32(ndet, b, 'val_confusion: ndet')
    _i32(nlab, b, 'val_confusion: nlab')
    if matrix is None and counts is None:
        raise RuntimeError('val_confusion: neither a matrix nor counts to add to')
    if matrix is not None:
        _need_gpu(matrix)
        if matrix.dtype != torch.int32 or matrix.numel() != (nc + 1) * (nc + 1) or not matrix.is_contiguous():
            raise RuntimeError(f'val_confusion: matrix must be a contiguous int32 tensor of (nc + 1)^2 = {(nc + 1) ** 2} elements, got {tuple(matrix.shape)} {matrix.dtype}')
    if counts is not None:
        _need_gpu(counts)
        if counts.dtype != torch.int64 or counts.numel() != nc * COUNT_SLOTS or not counts.is_contiguous():
            raise RuntimeError(f'val_confusion: counts must be a contiguous int64 tensor of nc x {COUNT_SLOTS} = {nc * COUNT_SLOTS} elements, got {tuple(counts.shape)} {counts.dtype}')
    ml = labels.shape[1]
    if _PROF is not None:
        _META['val_confusion_fwd'] = dict(shape=(b, md, ml, nc), flops=16.0 * b * md * ml * ((matrix is not None) + (counts is not None)),
                                          bytes=float(4 * (det.numel() + labels.numel())))
    _launch('val_confusion_fwd', 'mgdt_val_confusion_fwd', ptr(det), ptr(ndet), b, md, ptr(labels), ptr(nlab), ml, nc, float(cm_conf), float(cm_iou),
            float(cnt_conf), float(cnt_iou), 1 if trunc_labels else 0, ptr(matrix), ptr(counts), stream())
    return matrix, counts


# ------------------------------------------------------------------ instance-segmentation validation (mask IoU, matching from an IoU matrix)
MASK_IOU_MAX_DET, MASK_IOU_MAX_LAB, MASK_IOU_MAX_HW = 1024, 256, 1 << 24


def _i32(t, n, what):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise RuntimeError(f'{what} must be a contiguous int32 tensor of {n} elements, got {tuple(t.shape)} {t.dtype}')
    _need_gpu(t)
    return t


def exclusive_offsets(counts_dev):
    """(B,) int32 counts on the device -> their exclusive prefix sums (int32), without a host sync."""
    c = torch.cumsum(counts_dev, 0, dtype=torch.int32)
    return c - counts_dev


def _gt_check(gt, index_map, b, what):
    if gt.dtype != torch.uint8 or gt.dim() != 3 or not gt.is_contiguous():
        raise RuntimeError(f'{what}: the ground truth is a contiguous uint8 tensor, (B, H, W) index maps or (sum(nlab), H, W) instance masks, got '
                           f'{tuple(gt.shape)} {gt.dtype}')
    if index_map and gt.shape[0] != b:
        raise RuntimeError(f'{what}: {gt.shape[0]} index maps for a batch of {b}')
    _need_gpu(gt)


def mask_iou_batch(masks, counts_dev, offsets, max_det, gt, nlab, max_lab, index_map=True, lab_offsets=None, eps=1e-7, out=None):
    """mgdt_mask_iou_fwd: masks (sum(counts), H, W) uint8 0 / 1 as `seg_masks` lays them out + counts_dev / offsets (B,) int32 on the device; gt the
    (B, H, W) uint8 index maps (index_map=True: pixel value j + 1 = label j of that image) or (sum(nlab), H, W) uint8 instance masks with
    lab_offsets; nlab (B,) int32 -> iou (B, max_lab, max_det) float32, zero past nlab[i] / counts[i].  `out`: a caller's buffer (tests: guards)."""
    _need_gpu(masks)
    b = counts_dev.numel()
    if masks.dtype != torch.uint8 or masks.dim() != 3 or not masks.is_contiguous():
        raise RuntimeError(f'mask_iou: predicted masks are a contiguous uint8 (sum(counts), H, W) tensor, got {tuple(masks.shape)} {masks.dtype}')
    _gt_check(gt, index_map, b, 'mask_iou')
    if tuple(gt.shape[1:]) != tuple(masks.shape[1:]):
        raise RuntimeError(f'mask_iou: ground truth {tuple(gt.shape[1:])} and predictions {tuple(masks.shape[1:])} differ in size (ops.gt_masks_resample)')
    _i32(counts_dev, b, 'mask_iou: counts')
    _i32(offsets, b, 'mask_iou: offsets')
    _i32(nlab, b, 'mask_iou: nlab')
    if not index_map:
        if lab_offsets is None:
            raise RuntimeError('mask_iou: instance masks need lab_offsets')
        _i32(lab_offsets, b, 'mask_iou: lab_offsets')
    hw = masks.shape[1] * masks.shape[2]
    lib = L.lib()
    ws_bytes = lib.mgdt_mask_iou_workspace_bytes(b, max_det, max_lab)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=masks.device)
    if out is None:
        out = torch.empty(b, max_lab, max_det, dtype=torch.float32, device=masks.device)
    elif out.dtype != torch.float32 or out.numel() < b * max_lab * max_det or not out.is_contiguous():
        raise RuntimeError('mask_iou: `out` must be a contiguous float32 buffer of B x max_lab x max_det elements')
    if _PROF is not None:
        _META['mask_iou_fwd'] = dict(shape=(b, max_lab, max_det, hw), flops=2.0 * b * max_lab * max_det * hw, bytes=float(masks.numel() + gt.numel()))
    _launch('mask_iou_fwd', 'mgdt_mask_iou_fwd', ptr(masks), ptr(counts_dev), ptr(offsets), b, max_det, ptr(gt), 1 if index_map else 0, ptr(nlab),
            ptr(lab_offsets), max_lab, hw, float(eps), ptr(out), ptr(ws), ws_bytes, stream())
    return out


def gt_masks_resample(gt, nlab, lab_offsets, total, max_lab, shape, index_map=True):
    """mgdt_gt_masks_resample_fwd: ground truth of either form -> (total = sum(nlab), *shape) uint8 instance masks, each binary mask resampled
    bilinearly (align_corners=False) and thresholded > 0.5 as val.py:146-148 does when the sizes differ."""
    b = nlab.numel()
    _gt_check(gt, index_map, b, 'gt_masks_resample')
    _i32(nlab, b, 'gt_masks_resample: nlab')
    _i32(lab_offsets, b, 'gt_masks_resample: lab_offsets')
    oh, ow = int(shape[0]), int(shape[1])
    out = torch.empty(int(total), oh, ow, dtype=torch.uint8, device=gt.device)
    if int(total) == 0:
        return out
    _launch('gt_masks_resample_fwd', 'mgdt_gt_masks_resample_fwd', ptr(gt), 1 if index_map else 0, ptr(nlab), ptr(lab_offsets), b, max_lab,
            gt.shape[1], gt.shape[2], oh, ow, ptr(out), stream())
    return out


def val_match_iou(iou, det_rows, ndet, labels, nlab, iouv):
    """mgdt_val_match_iou_fwd: iou (B, max_lab, max_det) fp32, det_rows (B, max_det, >= 6) fp32 (class at column 5: the rows of `nms` / `nms_masks`
    read in place), labels (B, max_lab, >= 1) fp32 (class at column 0) -> correct (B, max_det, T) bool by the rule of `val_match`."""
    _need_gpu(iou)
    b, ml, md = iou.shape
    if (det_rows.dim() != 3 or det_rows.shape[0] != b or det_rows.shape[1] != md or det_rows.shape[2] < 6 or det_rows.dtype != torch.float32
            or not det_rows.is_contiguous()):
        raise RuntimeError(f'val_match_iou: det_rows must be contiguous float32 (B={b}, max_det={md}, >= 6), got {tuple(det_rows.shape)} {det_rows.dtype}')
    if labels.dim() != 3 or labels.shape[0] != b or labels.shape[1] != ml or labels.dtype != torch.float32 or not labels.is_contiguous():
        raise RuntimeError(f'val_match_iou: labels must be contiguous float32 (B={b}, max_lab={ml}, >= 1), got {tuple(labels.shape)} {labels.dtype}')
    if iou.dtype != torch.float32 or not iou.is_contiguous() or iouv.dtype != torch.float32:
        raise RuntimeError('val_match_iou: iou and iouv are contiguous float32 tensors')
    _i32(ndet, b, 'val_match_iou: ndet')
    _i32(nlab, b, 'val_match_iou: nlab')
    correct = torch.empty(b, md, iouv.numel(), dtype=torch.uint8, device=iou.device)
    _launch('val_match_iou_fwd', 'mgdt_val_match_iou_fwd', ptr(iou), b, ml, md, C.c_void_p(det_rows.data_ptr() + 20), det_rows.shape[2], ptr(ndet),
            ptr(labels), labels.shape[2], ptr(nlab), ptr(iouv), iouv.numel(), ptr(correct), stream())
    return correct.view(torch.bool)


# ------------------------------------------------------------------ pose validation (object keypoint similarity)
KPT_IOU_MAX_DET, KPT_IOU_MAX_LAB, KPT_IOU_MAX_NKPT = 1024, 256, 120


def kpt_iou_batch(pred, counts_dev, max_det, gt_kpts, area, nlab, sigma, eps=1e-7, out=None):
    """mgdt_kpt_iou_fwd: pred the padded NMS rows (B, max_det, 6 + nkpt * ndim) fp32 of `nms_masks` (keypoints read in place behind the six
    detection columns) or a dense (B, max_det, nkpt, ndim) fp32 tensor, ndim 2 or 3, + counts_dev (B,) int32; gt_kpts (B, max_lab, nkpt, 3) fp32
    [x, y, visibility] zero-padded, area (B, max_lab) fp32, nlab (B,) int32, sigma (nkpt,) fp32 on the device -> oks (B, max_lab, max_det)
    float32, zero past nlab[i] / counts[i] (the layout `val_match_iou` takes).  `out`: a caller's buffer (tests: guards)."""
    _need_gpu(pred)
    _need_gpu(gt_kpts)
    b = counts_dev.numel()
    if gt_kpts.dtype != torch.float32 or gt_kpts.dim() != 4 or gt_kpts.shape[0] != b or gt_kpts.shape[3] != 3 or not gt_kpts.is_contiguous():
        raise RuntimeError(f'kpt_iou: label keypoints are a contiguous float32 (B={b}, max_lab, nkpt, 3) tensor, got {tuple(gt_kpts.shape)} {gt_kpts.dtype}')
    max_lab, nkpt = gt_kpts.shape[1], gt_kpts.shape[2]
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() not in (3, 4) or pred.shape[0] != b or pred.shape[1] != max_det:
        raise RuntimeError(f'kpt_iou: predictions are a contiguous float32 (B={b}, max_det={max_det}, 6 + nk) or (B, max_det, nkpt, ndim) tensor, got '
                           f'{tuple(pred.shape)} {pred.dtype}')
    if pred.dim() == 4:
        lead, stride, ndim, ok = 0, pred.shape[2] * pred.shape[3], pred.shape[3], pred.shape[2] == nkpt
    else:
        lead, stride = 6, pred.shape[2]
        ndim, ok = (stride - 6) // max(nkpt, 1), nkpt > 0 and stride > 6 and (stride - 6) % nkpt == 0
    if not ok or ndim not in (2, 3):
        raise RuntimeError(f'kpt_iou: predictions {tuple(pred.shape)} do not hold nkpt={nkpt} keypoints of 2 or 3 values')
    if area.dtype != torch.float32 or tuple(area.shape) != (b, max_lab) or not area.is_contiguous():
        raise RuntimeError(f'kpt_iou: area must be a contiguous float32 (B={b}, max_lab={max_lab}) tensor, got {tuple(area.shape)} {area.dtype}')
    if not torch.is_tensor(sigma) or sigma.dtype != torch.float32 or sigma.numel() != nkpt or not sigma.is_contiguous():
        raise RuntimeError(f'kpt_iou: sigma must be a contiguous float32 tensor of nkpt={nkpt} values on the device')
    _need_gpu(area)
    _need_gpu(sigma)
    _i32(counts_dev, b, 'kpt_iou: counts')
    _i32(nlab, b, 'kpt_iou: nlab')
    if out is None:
        out = torch.empty(b, max_lab, max_det, dtype=torch.float32, device=pred.device)
    elif out.dtype != torch.float32 or out.numel() < b * max_lab * max_det or not out.is_contiguous():
        raise RuntimeError('kpt_iou: `out` must be a contiguous float32 buffer of B x max_lab x max_det elements')
    if _PROF is not None:
        _META['kpt_iou_fwd'] = dict(shape=(b, max_lab, max_det, nkpt, ndim), flops=8.0 * b * max_lab * max_det * nkpt,
                                    bytes=float(4 * (b * max_det * nkpt * ndim + gt_kpts.numel() + b * max_lab * max_det)))
    _launch('kpt_iou_fwd', 'mgdt_kpt_iou_fwd', C.c_void_p(pred.data_ptr() + 4 * lead), stride, ndim, ptr(counts_dev), b, max_det, ptr(gt_kpts), ptr(area),
            ptr(nlab), max_lab, nkpt, ptr(sigma), float(eps), ptr(out), stream())
    return out


# ------------------------------------------------------------------ detection loss (assigner + BCE/CIoU/DFL)
def _view_array(ts):
    views = [view(t) for t in ts]
    arr = (C.POINTER(View) * len(views))(*[C.pointer(v) for v in views])
    return arr, views


class DetectLossState:
    """Device buffers of one v8DetectionLoss evaluation (kept for the backward call)."""
    __slots__ = ('feats', 'strides', 'gt', 'n_gt', 'out5', 'ws', 'ws_bytes', 'reg_max', 'nc', 'gains', 'fg', 'gt_idx', 'tscore')


def detect_loss_fwd(feats, strides, reg_max, nc, gt, call_count, gains, want_assignment=False, call_count_dev=None):
    """feats: list of (B, 4R+nc, H, W) NHWC tensors; gt: (B, N, 5) fp32 cuda [cls, x1, y1, x2, y2] px.  Returns DetectLossState."""
    lib = L.lib()
    for f in feats:
        _need_gpu(f)
        if not is_nhwc(f):
            raise RuntimeError('detect_loss: head maps must be channels_last (NHWC) tensors')
    dev = feats[0].device
    b = feats[0].shape[0]
    a_total = sum(f.shape[2] * f.shape[3] for f in feats)
    n_gt = int(gt.shape[1])
    st = DetectLossState()
    st.feats, st.reg_max, st.nc, st.gains, st.n_gt = feats, reg_max, nc, gains, n_gt
    st.strides = torch.tensor([float(s) for s in strides], dtype=torch.float32)      # host array for the C call
    st.gt = gt.contiguous().float()
    st.out5 = torch.zeros(5, dtype=torch.float32, device=dev)
    st.ws_bytes = lib.mgdt_detect_loss_workspace_bytes(b, a_total, n_gt)
    st.ws = torch.empty(st.ws_bytes, dtype=torch.uint8, device=dev)
    st.fg = torch.empty(b, a_total, dtype=torch.uint8, device=dev) if want_assignment else None
    st.gt_idx = torch.empty(b, a_total, dtype=torch.int32, device=dev) if want_assignment else None
    st.tscore = torch.empty(b, a_total, dtype=torch.float32, device=dev) if want_assignment else None
    arr, keep = _view_array(feats)
    sarr = (C.c_float * len(feats))(*st.strides.tolist())
    if call_count_dev is not None:              # int32[1] on the device: the captured training step (hipGraph) replays with the host's counter
        _launch('detect_loss_fwd', 'mgdt_detect_loss_fwd_dev', arr, sarr, len(feats), reg_max, nc, ptr(st.gt) if n_gt else None, n_gt, ptr(call_count_dev),
                float(gains[0]), float(gains[1]), float(gains[2]), ptr(st.out5), ptr(st.fg), ptr(st.gt_idx), ptr(st.tscore), ptr(st.ws), st.ws_bytes,
                dtype_code(feats[0].dtype), stream())
        return st
    _launch('detect_loss_fwd', 'mgdt_detect_loss_fwd', arr, sarr, len(feats), reg_max, nc, ptr(st.gt) if n_gt else None, n_gt, int(call_count),
            float(gains[0]), float(gains[1]), float(gains[2]), ptr(st.out5), ptr(st.fg), ptr(st.gt_idx), ptr(st.tscore), ptr(st.ws), st.ws_bytes,
            dtype_code(feats[0].dtype), stream())
    return st


def detect_loss_bwd(st, gscale=1.0):
    """d(loss*B)/d feats for the state of a previous detect_loss_fwd; returns a list of NHWC grads."""
    grads = [like(f) for f in st.feats]
    arr, keep = _view_array(st.feats)
    garr, gkeep = _view_array(grads)
    sarr = (C.c_float * len(st.feats))(*st.strides.tolist())
    _launch('detect_loss_bwd', 'mgdt_detect_loss_bwd', arr, garr, sarr, len(st.feats), st.reg_max, st.nc, ptr(st.gt) if st.n_gt else None, st.n_gt,
            float(st.gains[0]), float(st.gains[1]), float(st.gains[2]), float(gscale), ptr(st.out5), ptr(st.ws), st.ws_bytes,
            dtype_code(st.feats[0].dtype), stream())
    return grads


# ------------------------------------------------------------------ training side (BN batch stats, backward kernels)
def _red_ws(c, dev):
    return torch.empty(L.lib().mgdt_reduce_workspace_bytes(c), dtype=torch.uint8, device=dev)


def bn_stats(y, eps, momentum, running_mean=None, running_var=None):
    """Batch mean / rstd (biased variance) of an NHWC map; updates the running stats in place when given."""
    c = y.shape[1]
    mean = torch.empty(c, dtype=torch.float32, device=y.device)
    rstd = torch.empty(c, dtype=torch.float32, device=y.device)
    ws = _red_ws(c, y.device)
    _launch('bn_stats_fwd', 'mgdt_bn_stats_fwd', vp(y), float(eps), float(momentum), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var),
            ptr(ws), dtype_code(y.dtype), stream())
    return mean, rstd


def bn_act(y, mean, rstd, gamma, beta, act, out=None, r1=None, r2=None):
    out = like(y) if out is None else out
    _same(y, out, r1, r2)
    _launch('bn_act_fwd', 'mgdt_bn_act_fwd', vp(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, vp(r1), vp(r2), vp(out), dtype_code(y.dtype), stream())
    return out


def bn_act_bwd(gz, y, mean, rstd, gamma, beta, act, dgamma=None, dbeta=None):
    """Returns dy (NHWC, same dtype); writes dgamma/dbeta (fp32) when given."""
    dy = like(y)
    _same(gz, y)
    ws = _red_ws(y.shape[1], y.device)
    _launch('bn_act_bwd', 'mgdt_bn_act_bwd', vp(gz), vp(y), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), act, ptr(dgamma), ptr(dbeta), vp(dy), ptr(ws),
            dtype_code(y.dtype), stream())
    return dy


class _PackedDgrad:
    """Weights of one conv packed for its stride-1 data gradient (mgdt_conv_pack_dgrad); same fields as PackedConv."""
    __slots__ = ('w', 'bias', 'k', 'cin', 'cout', 'dtype', 'direct', 'groups', 'key', 'owner', 'src', 'epoch', '__weakref__')

    def __init__(self, weight, k, dtype, key, phase=-1):
        import weakref
        self.owner = weakref.ref(weight)      # the address may be recycled by another parameter: the entry is valid for THIS tensor only
        cout, cin = weight.shape[0], weight.shape[1]
        code = dtype_code(dtype)
        self.k, self.cin, self.cout, self.dtype, self.direct, self.groups, self.key = k, cout, cin, dtype, False, 1, key   # a conv cout -> cin
        self.w = torch.empty(L.lib().mgdt_conv_packed_bytes(cout, cin, k, code), dtype=torch.uint8, device=weight.device)
        self.bias = torch.empty((cin + 15) // 16 * 16, dtype=torch.float32, device=weight.device)
        wf = weight.detach().float().contiguous()
        L.check(L.lib().mgdt_conv_pack_dgrad(ptr(wf), cin, cout, k, phase, code, ptr(self.w), ptr(self.bias), stream()), 'conv_pack_dgrad')
        if wf.data_ptr() == weight.data_ptr():                      # built from the live parameter storage: refreshable in place
            _register_pack(self, (wf, None, None, None, None, None, 0.0, cin, cout, k, code, 1 if phase < 0 else 2 + phase))


_DGRAD_PK = {}


def conv_dgrad(dy, weight, k, stride, dx, accumulate=False, r2=None):
    """dx (+)= d loss / d x of conv(x, weight).  Stride 1 on NHWC maps: the forward MFMA kernel on the flipped / transposed weights
    (re-packed once per optimizer epoch); otherwise the direct kernel.  `r2`: one more addend shaped like dx (a shortcut's gradient), fused
    into the convolution's epilogue where the MFMA path applies."""
    cout, cin = weight.shape[0], weight.shape[1]
    res = [t for t in (dx if accumulate else None, r2) if t is not None]
    r1_, r2_ = (res + [None, None])[:2]
    if (stride == 1 and (weight.dim() == 2 and k == 1 or weight.dim() == 4 and weight.shape[2] == k) and k in (1, 3) and dx.dtype == dy.dtype
            and is_nhwc(dx) and cin % 4 == 0
            and conv_can_mfma(dy, cout, cin, k, 1, 1, dy.dtype)):
        key = (PARAM_EPOCH[0], version_of(weight), dy.dtype)
        pk = _DGRAD_PK.get(weight.data_ptr())
        if pk is not None and pk.owner() is weight and pk.key[1:] == key[1:] and pack_is_current(pk):
            pk.key = key                                   # refreshed by repack_all() for this epoch
        if pk is None or pk.owner() is not weight or pk.key != key:
            pk = _DGRAD_PK[weight.data_ptr()] = _PackedDgrad(weight, k, dy.dtype, key)
        return conv2d(dy, pk, 1, ACT_NONE, out=dx, r1=r1_, r2=r2_)
    if (stride == 2 and k == 3 and weight.dim() == 4 and weight.shape[2] == 3 and dx.dtype == dy.dtype and is_nhwc(dx) and cin % 4 == 0
            and dx.shape[2] == 2 * dy.shape[2] and dx.shape[3] == 2 * dy.shape[3] and conv_can_mfma(dy, cout, cin, 3, 1, 1, dy.dtype)):
        # four phases (input-pixel parities), each a 3x3 convolution over dy written to a strided view of dx
        key = (PARAM_EPOCH[0], version_of(weight), dy.dtype)
        pks = _DGRAD_PK.get((weight.data_ptr(), 2))
        if pks is not None and pks[0].owner() is weight and pks[0].key[1:] == key[1:] and all(pack_is_current(q) for q in pks):
            for q in pks:
                q.key = key
        if pks is None or pks[0].owner() is not weight or pks[0].key != key:
            pks = _DGRAD_PK[(weight.data_ptr(), 2)] = [_PackedDgrad(weight, 3, dy.dtype, key, phase=ph) for ph in range(4)]
        for ph in range(4):
            sub = dx[:, :, ph >> 1::2, ph & 1::2]
            ra = None if r1_ is None else r1_[:, :, ph >> 1::2, ph & 1::2]
            rb = None if r2_ is None else r2_[:, :, ph >> 1::2, ph & 1::2]
            _same(dy, sub, ra, rb)
            if _PROF is not None:
                ntap = (1 + (ph >> 1)) * (1 + (ph & 1))
                _META['conv2d_fwd'] = dict(shape=(dy.shape[0], cout, dy.shape[2], dy.shape[3], cin, 3, 1), flops=2.0 * dy.shape[0] * dy.shape[2] * dy.shape[3] * cin * cout * ntap,
                                           bytes=float(dy.numel() * dy.element_size() + sub.numel() * sub.element_size() + pks[ph].w.numel()))
            _launch('conv2d_fwd', 'mgdt_conv2d_phase_fwd', vp(dy), ptr(pks[ph].w), ptr(pks[ph].bias), ph, vp(ra), vp(rb), vp(sub), dtype_code(dy.dtype), stream())
        return dx
    _same(dy, dx)
    _launch('conv_dgrad', 'mgdt_conv_dgrad', vp(dy), ptr(weight), k, stride, vp(dx), int(accumulate), dtype_code(dy.dtype), stream())
    return dx if r2 is None else add(dx, r2, out=dx)


def gconv_dgrad(dy, weight, k, stride, groups, dx, accumulate=False):
    """Grouped / depth-wise data gradient (DWConv, conv.py:82-86).  weight: [cout][cin/groups][k][k] fp32."""
    _same(dy, dx)
    _launch('conv_dgrad', 'mgdt_gconv_dgrad', vp(dy), ptr(weight), k, stride, groups, vp(dx), int(accumulate), dtype_code(dy.dtype), stream())
    return dx


def gconv_wgrad(x, dy, k, stride, groups, dw, accumulate=False):
    """Grouped / depth-wise weight gradient into dw ([cout][cin/groups][k][k] fp32)."""
    _same(x, dy)
    assert dw.is_contiguous() and dw.dtype == torch.float32 and dw.numel() == dy.shape[1] * (x.shape[1] // groups) * k * k
    flush_wgrad()                                   # deferred final sums of earlier convolutions read their own workspaces: keep the order simple
    ws = torch.empty(L.lib().mgdt_gconv_wgrad_workspace_bytes(x.shape[1], dy.shape[1], k, groups), dtype=torch.uint8, device=x.device)
    _launch('conv_wgrad', 'mgdt_gconv_wgrad', vp(x), vp(dy), k, stride, groups, ptr(dw), int(accumulate), ptr(ws), dtype_code(dy.dtype), stream())
    return dw


def conv_wgrad(x, dy, k, stride, dw, dbias=None, x2=None, accumulate=False, defer=True):
    """`defer=False`: the final sum is taken now even inside `with defer_wgrad():` (a caller that reads dw right away)"""
    lib = L.lib()
    if (not is_nhwc(x) or x.shape[1] % 4) and x.dtype in (torch.float32, torch.uint8, torch.bfloat16) and x2 is None and not accumulate and x.shape[1] < 4:
        # the 3-channel image (NCHW): one strided copy into a 4-channel NHWC buffer (4th channel zero) puts the stem on the tiled NHWC kernel;
        # the generic kernel would scan every pixel once per weight element
        b, c, h, w = x.shape
        x4 = new_act(b, 4, h, w, dy.dtype, x.device)                   # in dy's dtype; a uint8 image is divided by 255 on the way (detect/train.py:64)
        _launch('copy_fwd', 'mgdt_image_pad4_fwd', vp(x), U8 if x.dtype == torch.uint8 else dtype_code(x.dtype), vp(x4), dtype_code(x4.dtype), stream())
        dw4 = torch.empty((dw.shape[0], 4, k, k), dtype=torch.float32, device=x.device)
        conv_wgrad(x4, dy, k, stride, dw4, dbias=dbias)
        flush_wgrad()                                  # dw4 is read right below
        copy(dw4[:, :c], dw)
        return
    if is_nhwc(x) and x.shape[1] % 4 == 0 and dy.shape[1] % 4 == 0:
        _same(x, dy, x2)
    elif x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and x2 is None and is_nhwc(x) and x.shape[1] % 4 == 0:
        # a bf16 NHWC feature map in front of a convolution whose cout is no multiple of 4 (Detect's class branch with nc = 1 or 2 under amp): the
        # generic kernel reads fp32, so the map is widened first (one cast launch over a head-sized map; the values are the same)
        x = copy(x, new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], torch.float32, x.device))
    elif x.dtype != torch.float32 or dy.dtype not in (torch.float32, torch.bfloat16):
        # the generic kernel (any layout, any channel count) reads x as fp32 whatever dy is: any other dtype would be an out-of-range read
        raise RuntimeError(f'conv_wgrad: the generic (non-NHWC / channels % 4 != 0) path takes an fp32 input, got {x.dtype} (dy {dy.dtype})')
    # the dtype code names dy's type: x is of that type too on the NHWC path (checked above) and always fp32 on the generic one
    ws = torch.empty(lib.mgdt_conv_wgrad_workspace_bytes(x.shape[1], dy.shape[1], k), dtype=torch.uint8, device=x.device)
    if _PROF is not None:
        b, ci, h, w = x.shape
        _META['conv_wgrad'] = dict(shape=(b, ci, h, w, dy.shape[1], k, stride), flops=2.0 * dy.numel() * ci * k * k,
                                   bytes=float(x.numel() * x.element_size() + dy.numel() * dy.element_size()))
    if _WGRAD_DEFER[0] > 0 and accumulate:
        flush_wgrad()                                  # an accumulating gradient must see the value the pending jobs will write
    defer = (defer and _WGRAD_DEFER[0] > 0 and dbias is None and not accumulate and is_nhwc(x) and x.shape[1] % 4 == 0 and dy.shape[1] % 4 == 0 and dw.is_contiguous())
    _launch('conv_wgrad', 'mgdt_conv_wgrad', vp(x), vp(x2), vp(dy), k, stride, None if defer else ptr(dw), ptr(dbias), int(accumulate), ptr(ws), dtype_code(dy.dtype), stream())
    if defer:
        _WGRAD_PENDING.append((ws, dw, dw.numel(), lib.mgdt_conv_wgrad_splits(x.shape[1], dy.shape[1], k)))


# Deferred final sums of the weight gradients: inside `with defer_wgrad():` (the model's reverse pass) a convolution leaves its per-split partial sums
# in its workspace and `flush_wgrad()` adds them up for all pending convolutions in one launch (bit-identical to the immediate form).
_WGRAD_DEFER = [0]
_WGRAD_PENDING = []


class defer_wgrad:
    def __enter__(self):
        _WGRAD_DEFER[0] += 1

    def __exit__(self, *exc):
        _WGRAD_DEFER[0] -= 1
        if _WGRAD_DEFER[0] == 0:
            flush_wgrad()
        return False


def flush_wgrad():
    if not _WGRAD_PENDING:
        return
    arr = (L.WgradFinalDesc * len(_WGRAD_PENDING))()
    for d, (ws, dw, n, nsplit) in zip(arr, _WGRAD_PENDING):
        d.partial, d.dw, d.n, d.nsplit, d.accumulate = ptr(ws), ptr(dw), n, nsplit, 0
    _launch('wgrad_final_batch', 'mgdt_wgrad_final_batch', arr, len(_WGRAD_PENDING), stream())
    _WGRAD_PENDING.clear()


def add(a, b, out=None):
    out = like(a) if out is None else out
    _same(a, b, out)
    _launch('add_fwd', 'mgdt_add_fwd', vp(a), vp(b), vp(out), dtype_code(a.dtype), stream())
    return out


def maxpool5_bwd(x, gy):
    """Adjoint of MaxPool2d(5,1,2): dense NHWC gradient (B,C,H,W channels_last) in the dtype of gy (computed in fp32)."""
    _same(x, gy)
    b, c, h, w = x.shape
    gx = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device).contiguous(memory_format=torch.channels_last)
    _launch('maxpool5_bwd', 'mgdt_maxpool5_bwd', vp(x), vp(gy), ptr(gx), dtype_code(x.dtype), stream())
    return gx if gy.dtype == torch.float32 else copy(gx, like(gy))


def check_maxpool2d(kernel_size, stride, padding=0, dilation=1, ceil_mode=False, return_indices=False):
    """Only the pools of models/v3/yolov3-tiny.yaml are built (kernel 2, stride 2 or 1, padding 0, dilation 1, floor mode, no indices): anything else
    raises before a launch.  Returns (kernel, stride)."""
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    k, s = pair(kernel_size), pair(kernel_size if stride is None else stride)
    if k != (2, 2) or s not in ((1, 1), (2, 2)) or pair(padding) != (0, 0) or pair(dilation) != (1, 1) or ceil_mode or return_indices:
        raise RuntimeError(f'max pooling: only kernel 2, stride 2 or 1, padding 0, dilation 1, ceil_mode=False, return_indices=False is built '
                           f'(nn.MaxPool2d rows of yolov3-tiny), got kernel {k} stride {s} padding {pair(padding)} dilation {pair(dilation)} '
                           f'ceil_mode={bool(ceil_mode)} return_indices={bool(return_indices)}')
    return 2, s[0]


def _maxpool2d_size(x, stride):
    h, w = x.shape[2], x.shape[3]
    if h < 2 or w < 2:
        raise RuntimeError(f'max pooling 2x2: the {h}x{w} input is smaller than the window (the output would be empty)')
    return (h - 2) // stride + 1, (w - 2) // stride + 1


def maxpool2d(x, k, stride, out=None):
    """mgdt_maxpool2d_fwd: nn.MaxPool2d(2, stride) of an NHWC map (any sn / sh / sw); `out`: a view to write into."""
    _need_gpu(x)
    k, stride = check_maxpool2d(k, stride)
    oh, ow = _maxpool2d_size(x, stride)
    if out is None:
        out = new_act(x.shape[0], x.shape[1], oh, ow, x.dtype, x.device)
    _same(x, out)
    if _PROF is not None:
        _META['maxpool2d_fwd'] = dict(shape=(*x.shape, k, stride), flops=0.0, bytes=float((x.numel() + out.numel()) * x.element_size()))
    _launch('maxpool2d_fwd', 'mgdt_maxpool2d_fwd', vp(x), vp(out), k, stride, dtype_code(x.dtype), stream())
    return out


def maxpool2d_bwd(x, gy, k, stride, gx=None):
    """mgdt_maxpool2d_bwd: the adjoint of maxpool2d at x applied to gy, in the dtype of x, written to `gx` (a dense NHWC map when None)."""
    _need_gpu(x)
    k, stride = check_maxpool2d(k, stride)
    _maxpool2d_size(x, stride)
    gx = like(x) if gx is None else gx
    _same(x, gy, gx)
    if _PROF is not None:
        _META['maxpool2d_bwd'] = dict(shape=(*x.shape, k, stride), flops=0.0, bytes=float((2 * x.numel() + gy.numel()) * x.element_size()))
    _launch('maxpool2d_bwd', 'mgdt_maxpool2d_bwd', vp(x), vp(gy), vp(gx), k, stride, dtype_code(x.dtype), stream())
    return gx


def spp_pool_bwd(x, g5, g9, g13):
    """mgdt_spp_pool_bwd: sum of the adjoints of MaxPool2d(5 / 9 / 13, 1, k // 2) at x applied to g5 / g9 / g13 (SPP's direct windows), one launch.
    Dense NHWC gradient in the dtype of the g's (computed in fp32), the convention of maxpool5_bwd."""
    _same(x, g5, g9, g13)
    b, c, h, w = x.shape
    gx = torch.empty((b, c, h, w), dtype=torch.float32, device=x.device).contiguous(memory_format=torch.channels_last)
    if _PROF is not None:
        _META['spp_pool_bwd'] = dict(shape=tuple(x.shape), flops=0.0, bytes=float(x.numel() * (4 * x.element_size() + 4)))
    _launch('spp_pool_bwd', 'mgdt_spp_pool_bwd', vp(x), vp(g5), vp(g9), vp(g13), ptr(gx), dtype_code(x.dtype), stream())
    return gx if g5.dtype == torch.float32 else copy(gx, like(g5))


def nearest_bwd(gy, gx):
    _same(gy, gx)
    _launch('nearest_bwd', 'mgdt_nearest_bwd', vp(gy), vp(gx), dtype_code(gy.dtype), stream())
    return gx


# ------------------------------------------------------------------ adjoints of the MSPA / GD-neck ops
EW_MUL, EW_HSIG_GRAD, EW_MUL_HSIG, EW_HSIG = 0, 1, 2, 3


def ew(a, b, mode, out=None):
    out = like(a) if out is None else out
    _same(a, b, out)
    _launch('ew_binary', 'mgdt_ew_binary', vp(a), vp(b), vp(out), mode, dtype_code(a.dtype), stream())
    return out


def channel_affine(x, scale, shift, out=None):
    out = like(x) if out is None else out
    _same(x, out)
    _launch('channel_affine', 'mgdt_channel_affine', vp(x), ptr(scale), ptr(shift), vp(out), dtype_code(x.dtype), stream())
    return out


def nc_reduce(a, b=None):
    """sum over (h, w) of a*b (or a) per (image, channel) -> fp32 [B, C]."""
    _same(a, b)
    n, c = a.shape[:2]
    out = torch.empty(n, c, dtype=torch.float32, device=a.device)
    ws = torch.empty(L.lib().mgdt_nc_reduce_workspace_bytes(n, c), dtype=torch.uint8, device=a.device)
    _launch('nc_reduce', 'mgdt_nc_reduce', vp(a), vp(b), ptr(out), ptr(ws), dtype_code(a.dtype), stream())
    return out


def adaptive_avgpool_bwd(gy, gx, accumulate=False):
    _same(gy, gx)
    _launch('adaptive_avgpool_bwd', 'mgdt_adaptive_avgpool_bwd', vp(gy), vp(gx), int(accumulate), dtype_code(gy.dtype), stream())
    return gx


def bilinear_bwd(gy, gx, accumulate=False):
    _same(gy, gx)
    _launch('bilinear_bwd', 'mgdt_bilinear_bwd', vp(gy), vp(gx), int(accumulate), dtype_code(gy.dtype), stream())
    return gx


def spr_attention_train(x, fc1_w, fc1_b, fc2_w, fc2_b, groups):
    """Like spr_attention but also returns the pooled partial sums needed by the backward."""
    b, c, h, w = x.shape
    part = torch.empty(b * L.SPR_SPLITS * c * 5, dtype=torch.float32, device=x.device)
    _launch('spr_pool_fwd', 'mgdt_spr_pool_fwd', vp(x), ptr(part), dtype_code(x.dtype), stream())
    attn = torch.empty(b, c, dtype=torch.float32, device=x.device)
    _launch('spr_attn_fwd', 'mgdt_spr_attn_fwd', ptr(part), ptr(fc1_w), ptr(fc1_b), ptr(fc2_w), ptr(fc2_b), b, c, groups, h, w, 1, ptr(attn), stream())
    return attn, part


def spr_bwd(gy, part, attn, dattn, fc1_w, fc1_b, fc2_w, fc2_b, groups, out=None):
    """Returns (grad w.r.t. the pre-scale map, flat fp32 param grads [dW1 | db1 | dW2 | db2]); `out`: where to write the latter."""
    b, c = gy.shape[:2]
    lib = L.lib()
    cw = c // groups
    hid = cw // 4
    n_pg = hid * 5 * cw + hid + cw * hid + cw
    assert out is None or (out.numel() == n_pg and out.dtype == torch.float32 and out.is_contiguous())
    pg = torch.empty(n_pg, dtype=torch.float32, device=gy.device) if out is None else out
    ws = torch.empty(lib.mgdt_spr_bwd_workspace_bytes(b, c, groups), dtype=torch.uint8, device=gy.device)
    gx = like(gy)
    _launch('spr_bwd', 'mgdt_spr_bwd', vp(gy), ptr(part), L.SPR_SPLITS, ptr(attn), ptr(dattn), ptr(fc1_w), ptr(fc1_b), ptr(fc2_w), ptr(fc2_b), groups,
            vp(gx), ptr(pg), ptr(ws), dtype_code(gy.dtype), stream())
    return gx, pg


def dwconv7_ln_train(x, dw_w49c, dw_b, ln_w, ln_b, eps):
    y, u = like(x), like(x)
    _launch('dwconv7_ln_train_fwd', 'mgdt_dwconv7_ln_train_fwd', vp(x), ptr(dw_w49c), ptr(dw_b), ptr(ln_w), ptr(ln_b), eps, vp(y), vp(u),
            dtype_code(x.dtype), stream())
    return y, u


def dwconv7_ln_bwd(x, u, gy, dw_w49c, ln_w, eps, d_dw_w, d_dw_b, d_ln_w, d_ln_b):
    c = x.shape[1]
    dx, tmp = like(x), like(x)
    _same(x, u, gy)
    ws = torch.empty(L.lib().mgdt_dwconv7_ln_bwd_workspace_bytes(c), dtype=torch.uint8, device=x.device)
    _launch('dwconv7_ln_bwd', 'mgdt_dwconv7_ln_bwd', vp(x), vp(u), vp(gy), ptr(dw_w49c), ptr(ln_w), eps, vp(tmp), vp(dx), 0, ptr(d_dw_w), ptr(d_dw_b),
            ptr(d_ln_w), ptr(d_ln_b), ptr(ws), dtype_code(x.dtype), stream())
    return dx


def grn_bwd(g, t, S, A, B, gamma, dgamma, dbeta):
    n, c = t.shape[:2]
    dt = like(t)
    _same(g, t)
    ws = torch.empty(3 * n * c, dtype=torch.float32, device=t.device)
    _launch('grn_bwd', 'mgdt_grn_bwd', vp(g), vp(t), ptr(S), ptr(A), ptr(B), ptr(gamma), vp(dt), ptr(dgamma), ptr(dbeta), ptr(ws), dtype_code(t.dtype), stream())
    return dt


# ------------------------------------------------------------------ optimizer on the flat buffers
def grad_clip_coef(flat_grad, max_norm):
    """fp32[2] on device: {total gradient norm, clip coefficient} (no host sync)."""
    out = torch.empty(2, dtype=torch.float32, device=flat_grad.device)
    ws = torch.empty(L.lib().mgdt_grad_norm_workspace_bytes(), dtype=torch.uint8, device=flat_grad.device)
    _launch('grad_clip_coef', 'mgdt_grad_clip_coef', ptr(flat_grad), flat_grad.numel(), float(max_norm), ptr(out), ptr(ws), stream())
    return out


# Parameters updated by the HIP optimizer kernels change behind torch's back (no tensor version bump): every cache of packed / folded
# weights carries this epoch in its key and is rebuilt after an optimizer step.
PARAM_EPOCH = [0]


def _step_stream():
    """stream() for the launch of an optimizer step: the parameters are about to change, so the epoch moves.  (An argument of the launch and
    not a wrapper around it: these wrappers are ~10 us of Python per ~10 us kernel, where one more frame with *args shows in tools/optim_bench.py.)"""
    PARAM_EPOCH[0] += 1
    return stream()


def sgd_step(p, g, buf, wd, lr, momentum, nesterov, first, clip=None, lr_bias=None):
    _launch('sgd_step', 'mgdt_sgd_step', ptr(p), ptr(g), ptr(buf), ptr(wd), p.numel(), float(lr), float(lr if lr_bias is None else lr_bias), float(momentum),
            int(nesterov), int(first), ptr(clip), _step_stream())


def sgd_ema_step_dev(p, g, buf, wd, ema, data, hyper, nesterov, first, clip=None):
    """SGD over the parameters `p` (= data[:p.numel()]) and EMA over all of `data`, scalars {lr, lr_bias, momentum, ema_decay} from the device
    tensor `hyper` (fp32[4]): the form a captured training step uses."""
    _launch('sgd_ema_step_dev', 'mgdt_sgd_ema_step_dev', ptr(p), ptr(g), ptr(buf), ptr(wd), p.numel(), ptr(ema), data.numel(), ptr(hyper),
            int(nesterov), int(first), ptr(clip), _step_stream())


def ema_update(ema, p, decay):
    _launch('ema_update', 'mgdt_ema_update', ptr(ema), ptr(p), p.numel(), float(decay), stream())


OPT_HYPER_LEN = 8        # MGDT_OPT_HYPER_LEN: {lr, lr_bias, beta1 | momentum, ema_decay, lr / bc1, lr_bias / bc1, sqrt(bc2), 1 - beta1}


def adam_hyper(lr, lr_bias, beta1, beta2, step, ema_decay):
    """The fp32[8] vector of the captured Adam / AdamW step as a list of Python floats: bias corrections in double, as torch computes them
    (and as mgdt_adam_step derives them from the same arguments), rounded to fp32 when the list is copied to the device."""
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return [lr, lr_bias, beta1, ema_decay, lr / bc1, lr_bias / bc1, bc2 ** 0.5, 1 - beta1]


def rmsprop_hyper(lr, lr_bias, momentum, ema_decay):
    return [lr, lr_bias, momentum, ema_decay, 0.0, 0.0, 1.0, 0.0]


def adam_step(p, g, m, v, wd, lr, beta1, beta2, eps, step, decoupled, clip=None, lr_bias=None):
    """torch.optim.Adam (decoupled False) / AdamW (True) over the flat buffers; `step` is 1-based."""
    _launch('adam_step', 'mgdt_adam_step', ptr(p), ptr(g), ptr(m), ptr(v), ptr(wd), p.numel(), float(lr), float(lr if lr_bias is None else lr_bias),
            float(beta1), float(beta2), float(eps), int(step), int(decoupled), ptr(clip), _step_stream())


def adam_ema_step_dev(p, g, m, v, wd, ema, data, hyper, beta2, eps, decoupled, clip=None):
    """Adam / AdamW over the parameters `p` (= data[:p.numel()]) and EMA over all of `data`, per-step scalars from the device tensor `hyper`
    (fp32[8], adam_hyper): the form a captured training step uses."""
    _launch('adam_ema_step_dev', 'mgdt_adam_ema_step_dev', ptr(p), ptr(g), ptr(m), ptr(v), ptr(wd), p.numel(), ptr(ema), data.numel(), ptr(hyper),
            float(beta2), float(eps), int(decoupled), ptr(clip), _step_stream())


def rmsprop_step(p, g, sq, buf, wd, lr, alpha, eps, momentum, clip=None, lr_bias=None):
    """torch.optim.RMSprop(centered=False) over the flat buffers; `buf` may be None when momentum is 0."""
    _launch('rmsprop_step', 'mgdt_rmsprop_step', ptr(p), ptr(g), ptr(sq), ptr(buf), ptr(wd), p.numel(), float(lr), float(lr if lr_bias is None else lr_bias),
            float(alpha), float(eps), float(momentum), ptr(clip), _step_stream())


def rmsprop_ema_step_dev(p, g, sq, buf, wd, ema, data, hyper, alpha, eps, with_momentum, clip=None):
    """RMSProp + EMA with {lr, lr_bias, momentum, ema_decay} from the device tensor `hyper` (fp32[8], rmsprop_hyper)."""
    _launch('rmsprop_ema_step_dev', 'mgdt_rmsprop_ema_step_dev', ptr(p), ptr(g), ptr(sq), ptr(buf), ptr(wd), p.numel(), ptr(ema), data.numel(), ptr(hyper),
            float(alpha), float(eps), int(with_momentum), ptr(clip), _step_stream())


# ------------------------------------------------------------------ image classification (csrc/classify.hip)
FUSED_CLS_HEAD = True    # tests / tools/cls_bench.py flip this: Classify.conv + the spatial mean in one launch vs conv, pooling, linear as a 1x1 conv, softmax
CLS_FUSED_MAX_HW = None  # the fused head runs for maps of at most this many pixels (None: every size)


class PackedClsPool:
    """Classify.conv folded for mgdt_classify_pool_fwd: w (cout, c1) row-major in the compute dtype, bias fp32 (cout).  `weight` / `bias` are the
    folded fp32 parameters (fuse_conv_and_bn's arithmetic, so the panel is the same bit for bit before and after BaseModel.fuse())."""
    __slots__ = ('w', 'bias', 'cin', 'cout', 'dtype')

    def __init__(self, weight, bias, dtype):
        _need_gpu(weight)
        self.cout, self.cin, self.dtype = weight.shape[0], weight.shape[1], dtype
        self.w = weight.detach().float().reshape(self.cout, self.cin).to(dtype).contiguous()
        self.bias = (torch.zeros(self.cout, device=weight.device) if bias is None else bias.detach().float()).contiguous()


def classify_pool(x, pk, k=1, groups=1, act=ACT_SILU):
    """pooled (B, cout) fp32 = mean over the pixels of act(conv1x1(x) + bias): mgdt_classify_pool_fwd (refuses what it does not take)."""
    _need_gpu(x)
    if x.dtype != pk.dtype:
        raise RuntimeError(f'classify_pool: the weights are prepared for {pk.dtype}, the input is {x.dtype}')
    if x.shape[1] != pk.cin:
        raise RuntimeError(f'classify_pool: the input has {x.shape[1]} channels, the weights {pk.cin}')
    pooled = torch.empty(x.shape[0], pk.cout, dtype=torch.float32, device=x.device)
    _launch('classify_pool_fwd', 'mgdt_classify_pool_fwd', vp(x), ptr(pk.w), ptr(pk.bias), pk.cout, k, groups, act, ptr(pooled), dtype_code(pk.dtype), stream())
    return pooled


def classify_pool_supported(x, cin, cout, k, groups, act, dtype):
    pe = 8
    hw = x.shape[2] * x.shape[3]
    return (FUSED_CLS_HEAD and k == 1 and groups == 1 and act == ACT_SILU and cin % 8 == 0 and cout % 16 == 0 and x.dtype == dtype and is_nhwc(x)
            and (x.shape[3] == 1 or x.stride(3) % pe == 0) and (x.shape[2] == 1 or x.stride(2) % pe == 0) and (x.shape[0] == 1 or x.stride(0) % pe == 0)
            and x.data_ptr() % 16 == 0 and (CLS_FUSED_MAX_HW is None or hw <= CLS_FUSED_MAX_HW))


def classify_linear(pooled, w, bias, softmax=False):
    """(logits, probs or None): pooled (B, k) fp32 @ w (nc, k, compute dtype)^T + bias, fp32; `softmax`: the row softmax as well."""
    _need_gpu(pooled)
    if pooled.dtype != torch.float32 or not pooled.is_contiguous() or not w.is_contiguous() or w.shape[1] != pooled.shape[1]:
        raise RuntimeError('classify_linear: pooled must be a contiguous fp32 (B, k) tensor and w a contiguous (nc, k) one')
    n, k = pooled.shape
    nc = w.shape[0]
    logits = torch.empty(n, nc, dtype=torch.float32, device=pooled.device)
    probs = torch.empty_like(logits) if softmax else None
    _launch('classify_linear_fwd', 'mgdt_classify_linear_fwd', ptr(pooled), ptr(w), ptr(bias), n, k, nc, ptr(logits), ptr(probs), dtype_code(w.dtype), stream())
    return logits, probs


def cls_softmax(logits, out=None):
    _need_gpu(logits)
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous():
        raise RuntimeError('cls_softmax: logits must be a contiguous fp32 (B, nc) tensor')
    out = torch.empty_like(logits) if out is None else out
    _launch('cls_softmax_fwd', 'mgdt_cls_softmax_fwd', ptr(logits), logits.shape[0], logits.shape[1], ptr(out), stream())
    return out


def _cls_labels(labels, n, nc, device):
    """int64 (B,) labels on the device; labels that are still on the host are range-checked here (on the device the kernels give NaN / zero rows)."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(labels)
    if labels.dtype != torch.int64:
        raise RuntimeError(f"classification labels are int64 class indices (batch['cls']), got {labels.dtype}")
    labels = labels.reshape(-1)
    if labels.numel() != n:
        raise RuntimeError(f'classification labels: {labels.numel()} labels for {n} rows')
    if not labels.is_cuda:
        if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= nc):
            raise ValueError(f'classification label outside [0, {nc}): min {int(labels.min())}, max {int(labels.max())}')
        labels = labels.to(device)
    return labels.contiguous()


def _cls_logits(logits):
    _need_gpu(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise RuntimeError('classification logits must be a fp32 (B, nc) tensor')
    return logits.contiguous()


def cls_loss_fwd(logits, labels):
    """(loss fp32 scalar tensor = cross_entropy(sum) / 64, labels on the device)"""
    logits = _cls_logits(logits)
    n, nc = logits.shape
    labels = _cls_labels(labels, n, nc, logits.device)
    rows = torch.empty(n, dtype=torch.float32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    _launch('cls_loss_fwd', 'mgdt_cls_loss_fwd', ptr(logits), ptr(labels), n, nc, ptr(rows), ptr(loss), stream())
    return loss, labels


def cls_loss_bwd(logits, labels, gscale=1.0):
    logits = _cls_logits(logits)
    n, nc = logits.shape
    labels = _cls_labels(labels, n, nc, logits.device)
    d = torch.empty_like(logits)
    _launch('cls_loss_bwd', 'mgdt_cls_loss_bwd', ptr(logits), ptr(labels), n, nc, float(gscale), ptr(d), stream())
    return d


def cls_topk(probs, targets=None, matrix=None):
    """(B, min(nc, 5)) int64 indices of the largest probabilities per row, descending (equal values: lower index first).  `matrix` (nc, nc) int32 on
    the device: matrix[top1][target] += 1 in the same launch."""
    probs = _cls_logits(probs)
    n, nc = probs.shape
    out = torch.empty(n, min(nc, 5), dtype=torch.int64, device=probs.device)
    if matrix is not None:
        if targets is None:
            raise RuntimeError('cls_topk: the confusion matrix needs the targets')
        if matrix.dtype != torch.int32 or tuple(matrix.shape) != (nc, nc) or not matrix.is_contiguous() or not matrix.is_cuda:
            raise RuntimeError(f'cls_topk: matrix must be a contiguous int32 ({nc}, {nc}) device tensor')
        targets = _cls_labels(targets, n, nc, probs.device)
    _launch('cls_topk_fwd', 'mgdt_cls_topk_fwd', ptr(probs), n, nc, ptr(out), ptr(targets) if matrix is not None else None, ptr(matrix), stream())
    return out


# ---- ByteTrack (mgdt_bytetrack_*, mgdt_track_assign: csrc/track.hip) ----
TRACK_CAP = 128                    # == TK_CAP: most slots per stream, most detections above track_low_thresh per frame, most rows / columns of an assignment
TRACK_FLAG_DETS, TRACK_FLAG_TRACKS = 1, 2


def _track_cap(cap):
    if not 1 <= int(cap) <= TRACK_CAP:
        raise RuntimeError(f'bytetrack: track capacity {cap} is outside 1..{TRACK_CAP}')
    return int(cap)


def bytetrack_state(streams, cap, device):
    """A zeroed state buffer for `streams` streams of `cap` slots (uint8, mgdt_bytetrack_state_bytes)."""
    cap = _track_cap(cap)
    if torch.device(device).type != 'cuda':
        raise RuntimeError('mgdt_yolo_amd runs on MI355X (HIP) only: the tracker state lives on the device and there is no CPU/PyTorch fallback')
    return torch.zeros(L.lib().mgdt_bytetrack_state_bytes(int(streams), cap), dtype=torch.uint8, device=device)


def bytetrack_reset(state, streams, cap, which=-1):
    """Zero the state of stream `which` (-1: of every stream) on the current stream."""
    _need_gpu(state)
    _launch('bytetrack_reset', 'mgdt_bytetrack_reset', ptr(state), int(streams), _track_cap(cap), int(which), stream())


def bytetrack_update(rows, counts, state, cap, high, low, new, match, max_time_lost, active=None, out=None):
    """One frame of B streams (mgdt_bytetrack_update): rows (B, max_det, 6) fp32 + counts (B,) int32 as `nms` returns them, active (B,) uint8 / bool
    or None -> (tracks (B, cap, 8) fp32 [x1,y1,x2,y2,track_id,score,cls,idx] in ascending id, ntracks (B,) int32, flags (B,) int32).  No host read."""
    for t in (rows, counts, state):
        _need_gpu(t)
    cap = _track_cap(cap)
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] != 6 or not rows.is_contiguous():
        raise RuntimeError(f'bytetrack_update: rows must be a contiguous float32 (B, max_det, 6) tensor, got {tuple(rows.shape)} {rows.dtype}')
    b, md, _ = rows.shape
    counts = _i32(counts, b, 'bytetrack_update: counts')
    if state.dtype != torch.uint8 or state.numel() != L.lib().mgdt_bytetrack_state_bytes(b, cap) or not state.is_contiguous():
        raise RuntimeError(f'bytetrack_update: the state buffer does not belong to {b} streams of {cap} slots')
    if active is not None:
        _need_gpu(active)
        if active.dtype == torch.bool:
            active = active.view(torch.uint8)
        if active.dtype != torch.uint8 or active.shape != (b,) or not active.is_contiguous():
            raise RuntimeError('bytetrack_update: active must be a contiguous (B,) bool / uint8 tensor')
    if out is None:
        out = (torch.empty(b, cap, 8, dtype=torch.float32, device=rows.device), torch.empty(b, dtype=torch.int32, device=rows.device),
               torch.empty(b, dtype=torch.int32, device=rows.device))
    tracks, ntracks, flags = out
    _launch('bytetrack_update', 'mgdt_bytetrack_update', ptr(rows), ptr(counts), ptr(active), b, md, ptr(state), cap, float(high), float(low), float(new),
            float(match), int(max_time_lost), ptr(tracks), ptr(ntracks), ptr(flags), stream())
    return tracks, ntracks, flags


def track_assign(cost, n, m, thresh):
    """The tracker's assignment solver alone (mgdt_track_assign): cost (B, n_max, m_max) fp32, n / m (B,) int32 -> x (B, n_max) int32, -1 = unmatched."""
    _need_gpu(cost)
    if cost.dtype != torch.float32 or cost.dim() != 3 or not cost.is_contiguous():
        raise RuntimeError('track_assign: cost must be a contiguous float32 (B, n_max, m_max) tensor')
    b, nm, mm = cost.shape
    if not (1 <= nm <= TRACK_CAP and 1 <= mm <= TRACK_CAP):
        raise RuntimeError(f'track_assign: {nm} x {mm} is outside 1..{TRACK_CAP}')
    n, m = _i32(n, b, 'track_assign: n'), _i32(m, b, 'track_assign: m')
    x = torch.empty(b, nm, dtype=torch.int32, device=cost.device)
    _launch('track_assign', 'mgdt_track_assign', ptr(cost), ptr(n), ptr(m), b, nm, mm, float(thresh), ptr(x), stream())
    return x


def bytetrack_export(state, streams, cap, which):
    """The live tracks of one stream in ascending id as host arrays (mgdt_bytetrack_export + one host read)."""
    _need_gpu(state)
    cap = _track_cap(cap)
    dev = state.device
    hdr = torch.zeros(3, dtype=torch.int32, device=dev)
    ints = torch.zeros(6, cap, dtype=torch.int32, device=dev)
    sc = torch.zeros(2, cap, dtype=torch.float32, device=dev)
    mean = torch.zeros(cap, 8, dtype=torch.float64, device=dev)
    cov = torch.zeros(cap, 8, 8, dtype=torch.float64, device=dev)
    _launch('bytetrack_export', 'mgdt_bytetrack_export', ptr(state), int(streams), cap, int(which), ptr(hdr), ptr(ints), ptr(sc), ptr(mean), ptr(cov), stream())
    n, frame_id, count = hdr.tolist()
    ints, sc = ints[:, :n].cpu().numpy(), sc[:, :n].cpu().numpy()
    d = {k: ints[i] for i, k in enumerate(('id', 'state', 'is_activated', 'frame_id', 'start_frame', 'tracklet_len'))}
    d.update(score=sc[0], cls=sc[1], mean=mean[:n].cpu().numpy(), covariance=cov[:n].cpu().numpy(), tracker_frame_id=frame_id, count=count)
    return d


# ---- training augmentation (mgdt_aug_*: csrc/augment.hip) ----
AUG_IMAGE = np.dtype([('offset', '<i8'), ('h', '<i4'), ('w', '<i4'), ('label_start', '<i4'), ('label_count', '<i4')])      # == mgdt_aug_image
AUG_RECORD = np.dtype([('nrect', '<i4'), ('canvas', '<i4'), ('flags', '<i4'), ('lut', '<i4'), ('rect', '<i4', (4, 7)), ('inv', '<f4', (6,)),
                       ('m', '<f4', (6,)), ('scale', '<f4'), ('pad', '<f4', (4, 2)), ('reserved', '<i4', (3,))])                 # == mgdt_aug_record
assert AUG_IMAGE.itemsize == 24 and AUG_RECORD.itemsize == 224


def _aug_host(a, dtype, what):
    if not isinstance(a, np.ndarray) or a.dtype != dtype or a.ndim != 1 or not a.flags.c_contiguous:
        raise RuntimeError(f'{what} must be a contiguous 1-D numpy array of the {dtype.itemsize}-byte structure')
    return C.c_void_p(a.ctypes.data)


def aug_check(records, images, pool_bytes, n_labels, lut_bytes, imgsz):
    """mgdt_aug_check on the host copies of the records and the image table: raises on anything the launches would refuse.  Needs no GPU."""
    L.check(L.lib().mgdt_aug_check(_aug_host(records, AUG_RECORD, 'aug_check: records'), len(records), _aug_host(images, AUG_IMAGE, 'aug_check: images'),
                                   len(images), int(pool_bytes), int(n_labels), int(lut_bytes), int(imgsz)), 'aug_check')


def _aug_bytes(t, n, what):
    _need_gpu(t)
    if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise RuntimeError(f'{what} must be a contiguous uint8 device tensor of {n} bytes, got {tuple(t.shape)} {t.dtype}')
    return t


def aug_warp(pool, images_dev, images, records_dev, records, luts, batch, imgsz, out=None):
    """mgdt_aug_warp_fwd: placement, affine warp, HSV tables, flips and Format's channel order for `batch` images in one launch -> (B, 3, S, S) uint8
    RGB.  pool: flat uint8 device tensor; images / records: the host copies (checked), *_dev the same bytes on the device; luts: batch * 768 bytes."""
    _need_gpu(pool)
    if pool.dtype != torch.uint8 or pool.dim() != 1 or not pool.is_contiguous():
        raise RuntimeError('aug_warp: pool must be a flat contiguous uint8 tensor')
    _aug_bytes(images_dev, len(images) * AUG_IMAGE.itemsize, 'aug_warp: images_dev')
    _aug_bytes(records_dev, batch * AUG_RECORD.itemsize, 'aug_warp: records_dev')
    _aug_bytes(luts, batch * 768, 'aug_warp: luts')
    if len(records) != batch:
        raise RuntimeError(f'aug_warp: {len(records)} records for a batch of {batch}')
    if out is None:
        out = torch.empty(batch, 3, imgsz, imgsz, dtype=torch.uint8, device=pool.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (batch, 3, imgsz, imgsz) or not out.is_contiguous():
        raise RuntimeError(f'aug_warp: out must be a contiguous uint8 ({batch}, 3, {imgsz}, {imgsz}) tensor')
    _launch('aug_warp_fwd', 'mgdt_aug_warp_fwd', ptr(pool), pool.numel(), ptr(images_dev), _aug_host(images, AUG_IMAGE, 'aug_warp: images'), len(images),
            ptr(records_dev), _aug_host(records, AUG_RECORD, 'aug_warp: records'), ptr(luts), luts.numel(), int(batch), int(imgsz), ptr(out), stream())
    return out


def aug_labels(pool_labels, n_labels, images_dev, images, records_dev, records, batch, imgsz, cap, out=None):
    """mgdt_aug_labels_fwd: the boxes of `batch` output images in one launch -> (gt (B, cap, 5) [cls, x1, y1, x2, y2] px, labels (B, cap, 5)
    [cls, x, y, w, h] normalised, nlabels (B,) int32, flags (B,) int32: 1 = more than cap boxes survived, the rows are the first cap)."""
    _need_gpu(pool_labels)
    if pool_labels.dtype != torch.float32 or pool_labels.dim() != 2 or pool_labels.shape[1] != 5 or not pool_labels.is_contiguous() \
            or pool_labels.shape[0] < n_labels:
        raise RuntimeError(f'aug_labels: pool_labels must be a contiguous float32 (>= {n_labels}, 5) tensor')
    _aug_bytes(images_dev, len(images) * AUG_IMAGE.itemsize, 'aug_labels: images_dev')
    _aug_bytes(records_dev, batch * AUG_RECORD.itemsize, 'aug_labels: records_dev')
    if len(records) != batch:
        raise RuntimeError(f'aug_labels: {len(records)} records for a batch of {batch}')
    if cap < 16 or cap % 16:
        raise RuntimeError(f'aug_labels: the label capacity {cap} must be a multiple of 16')
    dev = pool_labels.device
    if out is None:
        out = (torch.empty(batch, cap, 5, dtype=torch.float32, device=dev), torch.empty(batch, cap, 5, dtype=torch.float32, device=dev),
               torch.empty(batch, dtype=torch.int32, device=dev), torch.empty(batch, dtype=torch.int32, device=dev))
    gt, labels, nlabels, flags = out
    _launch('aug_labels_fwd', 'mgdt_aug_labels_fwd', ptr(pool_labels), int(n_labels), ptr(images_dev), _aug_host(images, AUG_IMAGE, 'aug_labels: images'),
            len(images), ptr(records_dev), _aug_host(records, AUG_RECORD, 'aug_labels: records'), int(batch), int(imgsz), int(cap), ptr(gt), ptr(labels),
            ptr(nlabels), ptr(flags), stream())
    return gt, labels, nlabels, flags


# ------------------------------------------------------------------ RT-DETR decoder head (csrc/rtdetr.hip)
def _rt_shapes(shapes):
    """[(h, w)] per level -> (host int array the entry points read during the call, nl, L)"""
    flat = [int(v) for hw in shapes for v in hw]
    return (C.c_int * len(flat))(*flat), len(shapes), sum(int(h) * int(w) for h, w in shapes)


def _rt_rows(t, name, last=None, dtypes=(torch.float32,)):
    """a (..., C) fp32 cuda tensor whose rows are dense and evenly strided (a column slice of a contiguous matrix qualifies) -> (rows, row stride)"""
    _need_gpu(t)
    if t.dtype not in dtypes:
        raise RuntimeError(f'{name}: {" or ".join(str(d) for d in dtypes)} expected, got {t.dtype}')
    if last is not None and t.shape[-1] != last:
        raise RuntimeError(f'{name}: last dimension {t.shape[-1]}, expected {last}')
    rows = t.numel() // t.shape[-1]
    ld = t.stride(-2) if t.dim() > 1 else t.shape[-1]
    if t.stride(-1) != 1 or (t.dim() > 2 and any(t.stride(i) != t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 2))):
        raise RuntimeError(f'{name}: rows must be dense and evenly strided, got strides {t.stride()}')
    return rows, ld


def msdeform_attn(value, shapes, ref, offsets, weights):
    """mgdt_msdeform_attn_fwd.  value (B, L, >= 256 columns; a 256-column slice of a wider matrix is fine) fp32 or bf16, ref (B, nq, 4),
    offsets (B, nq, 8*nl*4*2) and weights (B, nq, 8*nl*4) logits (column slices of one panel are fine) -> (B, nq, 256) fp32."""
    _need_gpu(value)
    arr, nl, L = _rt_shapes(shapes)
    b, nq = ref.shape[0], ref.shape[1]
    if value.dim() != 3 or value.shape[0] != b or value.shape[1] != L or value.shape[2] != 256 or value.stride(2) != 1:
        raise RuntimeError(f'msdeform_attn: value {tuple(value.shape)} strides {value.stride()} for batch {b}, {L} tokens of 256 channels')
    _rt_rows(ref, 'msdeform_attn: ref', 4)
    if not ref.is_contiguous():
        raise RuntimeError('msdeform_attn: ref must be contiguous')
    _, ldo = _rt_rows(offsets, 'msdeform_attn: offsets', 8 * nl * 4 * 2)
    _, ldw = _rt_rows(weights, 'msdeform_attn: weights', 8 * nl * 4)
    if tuple(offsets.shape[:2]) != (b, nq) or tuple(weights.shape[:2]) != (b, nq):
        raise RuntimeError('msdeform_attn: offsets / weights must be (B, nq, ...) like ref')
    out = torch.empty(b, nq, 256, dtype=torch.float32, device=value.device)
    _launch('msdeform_attn_fwd', 'mgdt_msdeform_attn_fwd', ptr(value), value.stride(1), value.stride(0), arr, nl, b, nq, ptr(ref), ptr(offsets), ldo,
            ptr(weights), ldw, ptr(out), dtype_code(value.dtype), stream())
    return out


def mha(q, k, v):
    """mgdt_mha_fwd: q, k, v (B, nq, 256) fp32 (column slices of wider matrices are fine) -> (B, nq, 256), 8 heads, no mask."""
    (_, ldq), (_, ldk), (_, ldv) = _rt_rows(q, 'mha: q', 256), _rt_rows(k, 'mha: k', 256), _rt_rows(v, 'mha: v', 256)
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape:
        raise RuntimeError(f'mha: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} must be one (B, nq, 256) shape')
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    _launch('mha_fwd', 'mgdt_mha_fwd', ptr(q), ldq, ptr(k), ldk, ptr(v), ldv, q.shape[0], q.shape[1], ptr(out), stream())
    return out


def add_layernorm(x, res, gamma, beta, eps=1e-5, fill=None, shapes=None):
    """mgdt_add_layernorm_fwd: LayerNorm(x [+ res]) over the last dimension (256) -> fp32; x fp32 or bf16, the rest fp32.  `fill` + `shapes`: the
    masked form over (B, L, 256) tokens."""
    rows, ldx = _rt_rows(x, 'add_layernorm: x', 256, (torch.float32, torch.bfloat16))
    ldr = 0
    if res is not None:
        rr, ldr = _rt_rows(res, 'add_layernorm: res', 256)
        if rr != rows:
            raise RuntimeError('add_layernorm: x and res differ in rows')
    for t, n in ((gamma, 'gamma'), (beta, 'beta'), (fill, 'fill')):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 256 or not t.is_contiguous()):
            raise RuntimeError(f'add_layernorm: {n} must be 256 contiguous fp32 values')
    arr, nl = None, 0
    if fill is not None:
        arr, nl, L = _rt_shapes(shapes)
        if x.dim() != 3 or x.shape[1] != L:
            raise RuntimeError(f'add_layernorm: the masked form takes (B, {L}, 256) tokens, got {tuple(x.shape)}')
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _launch('add_layernorm_fwd', 'mgdt_add_layernorm_fwd', ptr(x), dtype_code(x.dtype), ldx, ptr(res), ldr, ptr(gamma), ptr(beta), float(eps), rows, ptr(fill), arr, nl, ptr(out), stream())
    return out


def rtdetr_rowmax(x):
    """mgdt_rtdetr_rowmax_fwd: (..., nc) fp32 -> (...) the maximum over the last dimension"""
    rows, ld = _rt_rows(x, 'rtdetr_rowmax: x')
    out = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _launch('rtdetr_rowmax_fwd', 'mgdt_rtdetr_rowmax_fwd', ptr(x), rows, x.shape[-1], ld, ptr(out), stream())
    return out


def rtdetr_topk(scores, k):
    """mgdt_rtdetr_topk_fwd: (B, L) fp32 -> (B, k) int64, descending score, equal scores by ascending index.  k > L raises, as torch.topk does."""
    _need_gpu(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
        raise RuntimeError(f'rtdetr_topk: contiguous (B, L) fp32 scores expected, got {tuple(scores.shape)} {scores.dtype}')
    b, L = scores.shape
    if not 1 <= k <= L:
        raise RuntimeError(f'rtdetr_topk: selected index k out of range (k = {k}, L = {L})')
    out = torch.empty(b, k, dtype=torch.int64, device=scores.device)
    _launch('rtdetr_topk_fwd', 'mgdt_rtdetr_topk_fwd', ptr(scores), b, L, k, ptr(out), stream())
    return out


def _rt_index(index, b, nq, name):
    _need_gpu(index)
    if index.dtype != torch.int64 or tuple(index.shape) != (b, nq) or not index.is_contiguous():
        raise RuntimeError(f'{name}: index must be a contiguous ({b}, {nq}) int64 tensor, got {tuple(index.shape)} {index.dtype}')


def rtdetr_gather(feat, scores, index):
    """mgdt_rtdetr_gather_fwd: feat (B, L, 256), scores (B, L, nc), index (B, nq) -> (embed (B, nq, 256), enc_scores (B, nq, nc))"""
    b, L = feat.shape[0], feat.shape[1]
    nq, nc = index.shape[1], scores.shape[-1]
    _rt_index(index, b, nq, 'rtdetr_gather')
    if feat.dtype != torch.float32 or not feat.is_contiguous() or feat.shape[2] != 256:
        raise RuntimeError('rtdetr_gather: feat must be contiguous (B, L, 256) fp32')
    rows, lds = _rt_rows(scores, 'rtdetr_gather: scores')
    if rows != b * L:
        raise RuntimeError('rtdetr_gather: scores must have one row per token')
    embed = torch.empty(b, nq, 256, dtype=torch.float32, device=feat.device)
    enc = torch.empty(b, nq, nc, dtype=torch.float32, device=feat.device)
    _launch('rtdetr_gather_fwd', 'mgdt_rtdetr_gather_fwd', ptr(feat), ptr(scores), lds, ptr(index), b, L, nq, nc, ptr(embed), ptr(enc), stream())
    return embed, enc


def rtdetr_ref_init(delta, index, shapes):
    """mgdt_rtdetr_ref_init_fwd: sigmoid(delta (B, nq, 4) + anchor(index)) -> (B, nq, 4)"""
    rows, ld = _rt_rows(delta, 'rtdetr_ref_init: delta', 4)
    b, nq = index.shape
    _rt_index(index, b, nq, 'rtdetr_ref_init')
    if rows != b * nq:
        raise RuntimeError('rtdetr_ref_init: delta must have one row per query')
    arr, nl, _ = _rt_shapes(shapes)
    out = torch.empty(b, nq, 4, dtype=torch.float32, device=delta.device)
    _launch('rtdetr_ref_init_fwd', 'mgdt_rtdetr_ref_init_fwd', ptr(delta), ld, ptr(index), b, nq, arr, nl, ptr(out), stream())
    return out


def rtdetr_refine(delta, ref):
    """mgdt_rtdetr_refine_fwd: sigmoid(delta + inverse_sigmoid(ref)), both (..., 4)"""
    rows, ld = _rt_rows(delta, 'rtdetr_refine: delta', 4)
    if ref.dtype != torch.float32 or not ref.is_contiguous() or ref.numel() != rows * 4:
        raise RuntimeError('rtdetr_refine: ref must be contiguous fp32 with one row of 4 per row of delta')
    _need_gpu(ref)
    out = torch.empty(ref.shape, dtype=torch.float32, device=ref.device)
    _launch('rtdetr_refine_fwd', 'mgdt_rtdetr_refine_fwd', ptr(delta), ld, ptr(ref), rows, ptr(out), stream())
    return out


def rtdetr_sigmoid(x):
    """mgdt_rtdetr_sigmoid_fwd: element-wise sigmoid of (..., nc) fp32 rows into a dense tensor"""
    rows, ld = _rt_rows(x, 'rtdetr_sigmoid: x')
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _launch('rtdetr_sigmoid_fwd', 'mgdt_rtdetr_sigmoid_fwd', ptr(x), rows, x.shape[-1], ld, ptr(out), stream())
    return out


def rtdetr_post(boxes, scores, conf, keep_class=None, wh=None):
    """mgdt_rtdetr_post_fwd: boxes (B, nq, 4) xywh, scores (B, nq, nc) -> (rows (B, nq, 6), counts (B,) int32), both on the device.
    keep_class: None or (nc,) uint8; wh: None or (B, 2) fp32 (w, h) each image's boxes are scaled by."""
    _need_gpu(boxes)
    b, nq, nc = scores.shape
    for t, n, sh in ((boxes, 'boxes', (b, nq, 4)), (scores, 'scores', (b, nq, nc))):
        if t.dtype != torch.float32 or tuple(t.shape) != sh or not t.is_contiguous() or not t.is_cuda:
            raise RuntimeError(f'rtdetr_post: {n} must be contiguous {sh} fp32 on the device')
    if keep_class is not None and (keep_class.dtype != torch.uint8 or keep_class.numel() != nc or not keep_class.is_contiguous() or not keep_class.is_cuda):
        raise RuntimeError(f'rtdetr_post: keep_class must be {nc} uint8 values on the device')
    if wh is not None and (wh.dtype != torch.float32 or tuple(wh.shape) != (b, 2) or not wh.is_contiguous() or not wh.is_cuda):
        raise RuntimeError(f'rtdetr_post: wh must be ({b}, 2) fp32 on the device')
    rows = torch.empty(b, nq, 6, dtype=torch.float32, device=boxes.device)
    counts = torch.empty(b, dtype=torch.int32, device=boxes.device)
    _launch('rtdetr_post_fwd', 'mgdt_rtdetr_post_fwd', ptr(boxes), ptr(scores), b, nq, nc, float(conf), ptr(keep_class), ptr(wh), ptr(rows), ptr(counts), stream())
    return rows, counts


# ------------------------------------------------------------------------------------------------ RT-DETR criterion, validator rows
DETR_GCAP = 256          # == MGDT_DETR_GCAP: most ground truths of one image, row length of the exported cost
DETR_MAX_NQ = 2048       # == MGDT_DETR_MAX_NQ
RTDETR_VAL_MAX_NQ = 4096
_DETR_WS = {}            # (device, bytes, lane) -> zero-initialised workspace of mgdt_detr_loss_fwd (its arrival counter lives across calls, at rest 0)


def _detr_inputs(boxes, logits, name):
    _need_gpu(boxes)
    if boxes.dim() != 4 or boxes.shape[-1] != 4 or boxes.dtype != torch.float32 or not boxes.is_contiguous():
        raise RuntimeError(f'{name}: boxes must be a contiguous (layers, B, nq, 4) fp32 tensor, got {tuple(boxes.shape)} {boxes.dtype}')
    l, b, nq = boxes.shape[:3]
    if logits.dim() != 4 or tuple(logits.shape[:3]) != (l, b, nq) or logits.dtype != torch.float32 or not logits.is_contiguous() or not logits.is_cuda:
        raise RuntimeError(f'{name}: logits must be a contiguous ({l}, {b}, {nq}, nc) fp32 tensor on the device, got {tuple(logits.shape)} {logits.dtype}')
    return l, b, nq, logits.shape[3]


def _detr_gts(gt_boxes, gt_cls, gt_groups, b, name):
    """gt_groups: the host's per-image counts -> (G, host int32 offsets (B + 1))."""
    if len(gt_groups) != b:
        raise RuntimeError(f'{name}: gt_groups has {len(gt_groups)} entries for a batch of {b}')
    off = np.zeros(b + 1, dtype=np.int32)
    np.cumsum(np.asarray(gt_groups, dtype=np.int64), out=off[1:])
    g = int(off[-1])
    if tuple(gt_boxes.shape) != (g, 4) or gt_boxes.dtype != torch.float32 or not gt_boxes.is_contiguous():
        raise RuntimeError(f'{name}: gt_boxes must be a contiguous ({g}, 4) fp32 tensor, got {tuple(gt_boxes.shape)} {gt_boxes.dtype}')
    if gt_cls.numel() != g or gt_cls.dtype != torch.int32 or not gt_cls.is_contiguous():
        raise RuntimeError(f'{name}: gt_cls must be {g} contiguous int32 values, got {tuple(gt_cls.shape)} {gt_cls.dtype}')
    if g:
        _need_gpu(gt_boxes)
        _need_gpu(gt_cls)
    return g, off


def detr_match(boxes, logits, gt_boxes, gt_cls, gt_groups, gt_off=None, gains=(2.0, 5.0, 2.0), alpha=0.25, gamma=2.0, layer_of_match=-1, want_cost=False):
    """mgdt_detr_match_fwd: boxes (layers, B, nq, 4), logits (layers, B, nq, nc) raw, gt_boxes (G, 4), gt_cls (G,) int32, gt_groups = the host's per-image
    counts, gt_off = their (B + 1,) exclusive offsets on the device (made here when None: one small copy, so pass it when capturing).
    -> assign (layers, B, nq) int32 [, cost (layers, B, nq, DETR_GCAP), zero where no ground truth]."""
    l, b, nq, nc = _detr_inputs(boxes, logits, 'detr_match')
    g, off = _detr_gts(gt_boxes, gt_cls, gt_groups, b, 'detr_match')
    dev = boxes.device
    if gt_off is None:
        gt_off = torch.from_numpy(off).to(dev)
    gt_off = _i32(gt_off, b + 1, 'detr_match: gt_off')
    nbytes = L.lib().mgdt_detr_match_workspace_bytes(l, g, nq)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    assign = torch.empty(l, b, nq, dtype=torch.int32, device=dev)
    cost = torch.zeros(l, b, nq, DETR_GCAP, dtype=torch.float32, device=dev) if want_cost else None
    _launch('detr_match_fwd', 'mgdt_detr_match_fwd', ptr(boxes), ptr(logits), logits.stride(2), l, b, nq, nc, ptr(gt_boxes) if g else None, ptr(gt_cls) if g else None,
            ptr(gt_off), off.ctypes.data_as(C.c_void_p), float(gains[0]), float(gains[1]), float(gains[2]), float(alpha), float(gamma), int(layer_of_match),
            ptr(ws), ws.numel(), ptr(assign), ptr(cost), stream())
    return (assign, cost) if want_cost else assign


def detr_loss(boxes, logits, gt_boxes, gt_cls, assign, num_pairs, gains=(1.0, 5.0, 2.0), use_vfl=True, gscale=1.0, want_grads=False):
    """mgdt_detr_loss_fwd: -> (out (layers + 1, 3) = class / bbox / giou per layer and, in the last row, summed over every layer but the last, gt_score
    (layers, B, nq), d_boxes, d_logits); the gradients (of gscale * out[:layers].sum()) are None unless want_grads."""
    l, b, nq, nc = _detr_inputs(boxes, logits, 'detr_loss')
    g = gt_boxes.shape[0]
    if tuple(gt_boxes.shape) != (g, 4) or gt_boxes.dtype != torch.float32 or not gt_boxes.is_contiguous() or gt_cls.numel() != g or gt_cls.dtype != torch.int32 or not gt_cls.is_contiguous():
        raise RuntimeError(f'detr_loss: gt_boxes (G, 4) fp32 and gt_cls (G,) int32 expected, got {tuple(gt_boxes.shape)} {gt_boxes.dtype}, {tuple(gt_cls.shape)} {gt_cls.dtype}')
    if tuple(assign.shape) != (l, b, nq):
        raise RuntimeError(f'detr_loss: assign must be ({l}, {b}, {nq}), got {tuple(assign.shape)}')
    assign = _i32(assign, l * b * nq, 'detr_loss: assign')
    dev = boxes.device
    nbytes = L.lib().mgdt_detr_loss_workspace_bytes(l, b, nq)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), nbytes, _LANE[0])
    ws = _DETR_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('detr_loss: run the criterion once before capturing it into a graph (the kernel\'s arrival counter is allocated and zeroed on first use)')
        ws = _DETR_WS[key] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(l + 1, 3, dtype=torch.float32, device=dev)
    gt_score = torch.empty(l, b, nq, dtype=torch.float32, device=dev)
    d_boxes = torch.empty(l, b, nq, 4, dtype=torch.float32, device=dev) if want_grads else None
    d_logits = torch.empty(l, b, nq, nc, dtype=torch.float32, device=dev) if want_grads else None
    _launch('detr_loss_fwd', 'mgdt_detr_loss_fwd', ptr(boxes), ptr(logits), logits.stride(2), l, b, nq, nc, ptr(gt_boxes) if g else None, ptr(gt_cls) if g else None, g,
            ptr(assign), int(num_pairs), float(gains[0]), float(gains[1]), float(gains[2]), 1 if use_vfl else 0, float(gscale), ptr(ws), nbytes, ptr(out), ptr(gt_score),
            ptr(d_boxes), ptr(d_logits), stream())
    return out, gt_score, d_boxes, d_logits


def rtdetr_val_post(boxes, scores, wh=None):
    """mgdt_rtdetr_val_post_fwd: boxes (B, nq, 4) xywh, scores (B, nq, nc) -> (rows (B, nq, 6) in descending confidence (ties by query index, NaN last),
    counts (B,) int32 = nq), all nq rows, no threshold.  wh: None or (B, 2) fp32 (w, h) each image's boxes are scaled by."""
    _need_gpu(boxes)
    if scores.dim() != 3:
        raise RuntimeError(f'rtdetr_val_post: scores must be (B, nq, nc), got {tuple(scores.shape)}')
    b, nq, nc = scores.shape
    for t, n, sh in ((boxes, 'boxes', (b, nq, 4)), (scores, 'scores', (b, nq, nc))):
        if t.dtype != torch.float32 or tuple(t.shape) != sh or not t.is_contiguous() or not t.is_cuda:
            raise RuntimeError(f'rtdetr_val_post: {n} must be contiguous {sh} fp32 on the device')
    if wh is not None and (wh.dtype != torch.float32 or tuple(wh.shape) != (b, 2) or not wh.is_contiguous() or not wh.is_cuda):
        raise RuntimeError(f'rtdetr_val_post: wh must be ({b}, 2) fp32 on the device')
    rows = torch.empty(b, nq, 6, dtype=torch.float32, device=boxes.device)
    counts = torch.empty(b, dtype=torch.int32, device=boxes.device)
    _launch('rtdetr_val_post_fwd', 'mgdt_rtdetr_val_post_fwd', ptr(boxes), ptr(scores), b, nq, nc, ptr(wh), ptr(rows), ptr(counts), stream())
    return rows, counts
