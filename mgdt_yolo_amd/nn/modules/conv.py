"""Convolution modules of the registry (reference: nn/modules/conv.py), compute on MI355X via libmgdt_hip.so.

Same class names, constructor signatures and parameter names as the reference (`conv.weight`,
`bn.{weight,bias,running_mean,running_var}`), so YAML graphs and state_dicts transfer unchanged.
nn.Conv2d / nn.BatchNorm2d objects are used as PARAMETER CONTAINERS only; their forward is never called.
"""
import math

import torch
import torch.nn as nn

from ... import ops

__all__ = ('Conv', 'DWConv', 'ConvTranspose2d', 'MaxPool2d', 'ZeroPad2d', 'Repeat', 'Concat', 'autopad')


def autopad(k, p=None, d=1):
    """'same' padding (reference nn/modules/conv.py:16-22)."""
    if d > 1:
        k = d * (k - 1) + 1 if isinstance(k, int) else [d * (x - 1) + 1 for x in k]
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


def act_code(m):
    if isinstance(m, nn.SiLU):
        return ops.ACT_SILU
    if isinstance(m, nn.ReLU):
        return ops.ACT_RELU
    if isinstance(m, nn.Identity):
        return ops.ACT_NONE
    if isinstance(m, nn.GELU):
        return ops.ACT_GELU
    raise RuntimeError(f'activation {type(m).__name__} has no fused HIP epilogue (SiLU, ReLU, GELU, Identity are built)')


# -- what every fused route asks of the host (DESIGN section 3a lists, route by route, which of these it consults and why) -------------------------
FUSED_ACTS = (nn.Identity, nn.SiLU, nn.ReLU, nn.GELU)  # the activations act_code() knows
EPILOGUE_ACTS = FUSED_ACTS[:3]                         # ... and the ones the one-launch SPPF / LAF kernels carry


def plain(c, k, acts=(nn.SiLU,), stride=1):
    """Conv.plain for a slot that may hold something else (nn.Identity, a bare nn.Conv2d): those are not plain"""
    return isinstance(c, Conv) and c.plain(k, acts, stride)


def watched(*modules):
    """somebody observes one of these modules (forward hooks): a fused route would skip the call the hook hangs on"""
    return any(m._forward_hooks for m in modules)


def fp8_claims(*modules):
    """fp8 owns a convolution site of these modules: quantize_fp8 is calibrating (every site must see its input), or one of them carries multipliers"""
    return ops.Q8_CALIB is not None or any(m.__dict__.get('_q8') for m in modules)


def merged_panel(owner, key, a, b, k, dt, xq=None):
    """Panel of two sibling convolutions concatenated along cout (BatchNorm folded per branch; after fuse() the folded biases ride on the merged conv): [a | b]
    in one launch.  None unless both are fused or neither, with one BatchNorm eps.  `xq`: the e4m3 panel (quantize_fp8).  Cached on `owner` under key + ..."""
    fused = not hasattr(a, 'bn')
    if fused != (not hasattr(b, 'bn')) or (not fused and a.bn.eps != b.bn.eps):
        return None
    cat = lambda fn: torch.cat([fn(a).detach().float(), fn(b).detach().float()])
    zb = lambda m: m.conv.bias if m.conv.bias is not None else torch.zeros(m.conv.out_channels, device=m.conv.weight.device)
    bn = lambda: None if fused else (cat(lambda m: m.bn.weight), cat(lambda m: m.bn.bias), cat(lambda m: m.bn.running_mean), cat(lambda m: m.bn.running_var), a.bn.eps)
    cb = lambda: cat(zb) if fused else None
    tens = [t for m in (a, b) for t in m.affine_tensors()]
    if xq is not None:
        return owner._cached(key + ('fp8', float(xq)), tens, lambda: ops.PackedConvFp8(cat(lambda m: m.conv.weight), cb(), bn(), k, xq))
    return owner._cached(key + (dt,), tens, lambda: ops.PackedConv(cat(lambda m: m.conv.weight), cb(), bn(), k, dt))


class HipModule(nn.Module):
    """Base: compute dtype bookkeeping + packed-weight cache invalidated by parameter versions."""
    _cdtype = None   # set by DetectionModel.set_compute_dtype(); None -> follow the input

    def out_dtype(self, x):
        return self._cdtype or (x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32)

    def _cached(self, key, tensors, build):
        cache = self.__dict__.setdefault('_pk', {})
        ver = (ops.PARAM_EPOCH[0],) + tuple((t.data_ptr(), ops.version_of(t)) for t in tensors if t is not None)
        hit = cache.get(key)
        if hit is not None and hit[0] != ver and hit[0][1:] == ver[1:] and ops.pack_is_current(hit[1]):
            hit = cache[key] = (ver, hit[1])             # the panel was refreshed in place by ops.repack_all() after the optimizer step
        if hit is None or hit[0] != ver:
            hit = (ver, build())
            cache[key] = hit
        return hit[1]

    def q8_site(self, key, x, x2=None):
        """fp8 bookkeeping of one implicit-GEMM convolution site of this module (`key` None: the module's own conv; merged panels name theirs).
        While BaseModel.quantize_fp8() calibrates: records the largest |input| the site sees.  Returns the site's activation multiplier, or None
        when the site runs in bf16."""
        if ops.Q8_CALIB is not None:
            xe = x if x2 is None else x.float() + x2.float()
            if ops.Q8_CALIB_PCT is None:
                amax = float(xe.abs().max())
            else:                                            # a high percentile of |input| instead of its maximum (outliers saturate at +-448)
                flat = xe.detach().abs().float().reshape(-1)
                if flat.numel() > (1 << 20):
                    flat = flat[::flat.numel() // (1 << 20)]
                k = min(flat.numel(), max(1, int(round(ops.Q8_CALIB_PCT / 100.0 * flat.numel()))))
                amax = float(flat.kthvalue(k).values)
            ops.Q8_CALIB[(self, key)] = max(ops.Q8_CALIB.get((self, key), 0.0), amax)
        q = self.__dict__.get('_q8')
        return None if q is None else q.get(key)

    @staticmethod
    def _no_train_bn(m):
        if m.training:
            raise NotImplementedError('this call path folds BatchNorm running statistics into the weights (eval); the training-mode path '
                                      '(batch statistics + backward) is Conv.train_fwd / Conv.backward - call the module in .train() mode '
                                      'through forward(), or .eval() it (raw head maps for the loss: model.model[-1].training = True)')

    def _save_ctx(self, item):
        """Keep what backward() needs.  Nothing is kept when no backward can follow (torch.no_grad() outside the model-level autograd
        Function), and DetectionModel._predict_once drops every stale context at the start of a train-mode forward, so a forward that is
        never followed by a backward cannot pin activations."""
        if ops.ctx_enabled():
            self.__dict__.setdefault('_ctx', []).append(item)


class Conv(HipModule):
    """Conv2d + BatchNorm2d + act (reference nn/modules/conv.py:25-42); BN folded at pack time (torch_utils.py:114-135)."""
    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p, d), groups=g, dilation=d, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()

    # -- the conv's affine part, before and after BaseModel.fuse() -----------------------------------
    def plain_affine(self):
        """True for the two forms the block-level kernels take: bias-free conv + BatchNorm (as built), or - after `fuse()` (tasks.py:121-146:
        `bn` deleted, the folded bias on the conv) - conv + bias.  (the fused model AutoBackend / the predictor run took none of the
        block kernels.)"""
        return (hasattr(self, 'bn') and self.conv.bias is None) or not hasattr(self, 'bn')

    def plain(self, k, acts=(nn.SiLU,), stride=1):
        """THE definition of a convolution a fused route may compute in this module's place: plain_affine(), a dense k x k kernel at `stride` with 'same' padding
        and no dilation (what Conv._geometry accepts), an activation in `acts`.  Channel counts stay at the sites.  `stride=None`: not looked at."""
        c = self.conv
        return (self.plain_affine() and c.kernel_size == (k, k) and (stride is None or c.stride == (stride, stride)) and c.padding == (k // 2, k // 2) and c.dilation == (1, 1)
                and c.groups == 1 and isinstance(self.act, acts))

    def bn_tuple(self):
        """(gamma, beta, mean, var, eps) for the pack routines, or None after fuse() (the conv then carries its bias)"""
        return (self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var, self.bn.eps) if hasattr(self, 'bn') else None

    def affine_tensors(self):
        """every tensor a packed panel of this conv depends on (cache keys)"""
        t = [self.conv.weight, self.conv.bias]
        if hasattr(self, 'bn'):
            t += [self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]
        return t

    def folded_bn_like(self):
        """the affine part as a BatchNorm tuple whatever the form: after fuse() the identity transform carrying the bias (gamma 1, mean 0,
        var 1, eps 0: exact)"""
        if hasattr(self, 'bn'):
            return self.bn_tuple()
        w = self.conv.weight
        one, zero = torch.ones(w.shape[0], device=w.device), torch.zeros(w.shape[0], device=w.device)
        return (one, self.conv.bias.detach().float() if self.conv.bias is not None else zero, zero, one, 0.0)

    # -- packed weights ------------------------------------------------------------------------------
    def _stem6(self):
        """the 6x6 / stride 2 / padding 2 stem of the YOLOv5 graphs (models/v5/yolov5.yaml row 0): runs as space-to-depth + a 3x3 / stride 1 convolution
        over the 4 * c1 channel map (ops.space_to_depth2, ops.stem6_w3), an exact identity"""
        c = self.conv
        return (c.kernel_size == (6, 6) and c.stride == (2, 2) and c.padding == (2, 2) and c.dilation == (1, 1) and c.groups == 1 and c.in_channels <= 4)

    def _geometry(self):
        c = self.conv
        if self._stem6():
            return 6, 2
        k, s = c.kernel_size[0], c.stride[0]
        if c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1] or c.dilation != (1, 1) or c.padding != (k // 2, k // 2):
            raise RuntimeError(f'Conv geometry {c} is outside the built kernels (square k, same padding, dilation 1)')
        return k, s

    def _stem6_input(self, x, dt):
        """the space-to-depth map the 3x3 form of the 6x6 stem reads; sizes it cannot take raise before any launch"""
        if x.dim() != 4 or x.shape[1] != self.conv.in_channels or x.shape[2] % 2 or x.shape[3] % 2:
            raise RuntimeError(f'Conv: the 6x6 / stride 2 / padding 2 stem takes a (B, {self.conv.in_channels}, H, W) image with even H and W '
                               f'(model inputs are multiples of the stride), got {tuple(x.shape)}')
        return ops.space_to_depth2(x, dt)

    def _stem6_packed(self, dt, direct, raw=False):
        """panel of the 3x3 form (zero rows for the map's pad channels).  On the MFMA route it is packed straight from the live 6x6 weight
        (ops.PackedStem6), so it follows ops.PARAM_EPOCH / ops.repack_all() under the trainer like every other panel; the direct kernel's panel is
        packed from the derived copy ops.stem6_w3 and rebuilt when the weights move or change.  `raw`: the bare convolution of the training forward."""
        tens = [self.conv.weight] if raw else self.affine_tensors()
        cb, bn = (None, None) if raw else (self.conv.bias, self.bn_tuple())
        if not direct:
            return self._cached(('stem6', raw, dt), tens, lambda: ops.PackedStem6(self.conv.weight, cb, bn, dt))
        cp = ops.space_to_depth2_channels(self.conv.in_channels, dt)
        return self._cached(('stem6', raw, dt, 'direct'), tens, lambda: ops.PackedConv(ops.stem6_w3(self.conv.weight, cp), cb, bn, 3, dt, direct=True))

    def packed(self, dtype, direct):
        k, _ = self._geometry()
        if k == 6:
            return self._stem6_packed(dtype, direct)
        return self._cached((dtype, direct), self.affine_tensors(),
                            lambda: ops.PackedConv(self.conv.weight, self.conv.bias, self.bn_tuple(), k, dtype, direct=direct, groups=self.conv.groups))

    def packed_fp8(self, xq):
        k, _ = self._geometry()
        return self._cached(('fp8', float(xq)), self.affine_tensors(), lambda: ops.PackedConvFp8(self.conv.weight, self.conv.bias, self.bn_tuple(), k, xq))

    def packed_acc_order(self, dt):
        """panel of this 1x1 conv with its input channels in accumulator order: it reads another kernel's accumulators in place"""
        w = self.conv.weight
        return self._cached(('acc_order', dt), self.affine_tensors(), lambda: ops.PackedConv(
            w.detach()[:, ops.acc_order_index(self.conv.in_channels, w.device)], self.conv.bias, self.bn_tuple(), 1, dt))

    # -- compute ----------------------------------------------------------------------------------------
    def fwd(self, train, x, out=None, x2=None, r1=None, r2=None):
        """train_fwd or run, by the flag the enclosing block computed once (its own mode and its first conv's `bn`)"""
        return (self.train_fwd if train else self.run)(x, out=out, x2=x2, r1=r1, r2=r2)

    def run(self, x, out=None, x2=None, r1=None, r2=None, in_scale=None, in_shift=None):
        if hasattr(self, 'bn'):
            self._no_train_bn(self.bn)
        k, s = self._geometry()
        dt = self.out_dtype(x) if out is None else out.dtype
        if k == 6:                              # the YOLOv5 stem: space-to-depth, then the 3x3 / stride 1 form on the implicit GEMM (bf16 operands under quantize_fp8 too)
            if x2 is not None or in_scale is not None or in_shift is not None:
                raise RuntimeError('Conv: the 6x6 stem reads the image (no fused pre-add or input affine)')
            sd = self._stem6_input(x, dt)
            mfma = ops.conv_can_mfma(sd, sd.shape[1], self.conv.out_channels, 3, 1, 1, dt)
            return ops.conv2d(sd, self._stem6_packed(dt, not mfma), 1, act_code(self.act), out=out, r1=r1, r2=r2)
        mfma = ops.conv_can_mfma(x, self.conv.in_channels, self.conv.out_channels, k, s, self.conv.groups, dt)
        if mfma and dt == torch.bfloat16:
            xq = self.q8_site(None, x, x2)
            if xq is not None:                  # fp8 inference (BASELINE configs[4]): e4m3 operands, per-tensor activation / per-channel weight scales
                return ops.conv2d_fp8(x, self.packed_fp8(xq), s, act_code(self.act), out=out, x2=x2, r1=r1, r2=r2, in_scale=in_scale, in_shift=in_shift)
        pk = self.packed(dt, direct=not mfma)
        return ops.conv2d(x, pk, s, act_code(self.act), out=out, x2=x2, r1=r1, r2=r2, in_scale=in_scale, in_shift=in_shift)

    def forward(self, x):
        return self.fwd(self.training and hasattr(self, 'bn'), x)

    # -- training mode: batch-statistics BN, context for backward ---------------------------------------------
    def train_fwd(self, x, out=None, x2=None, r1=None, r2=None):
        """act(bn_batchstats(conv(x [+ x2]))) [+ r1] [+ r2]; keeps (x, x2, raw conv output, mean, rstd) for backward()."""
        k, s = self._geometry()
        dt = self.out_dtype(x) if out is None else out.dtype
        if k == 6:                              # the YOLOv5 stem: the same route as run(); backward() sees the space-to-depth map as the conv's input
            if x2 is not None:
                raise RuntimeError('Conv.train_fwd: the 6x6 stem reads the image (no fused pre-add)')
            x = self._stem6_input(x, dt)
            mfma = ops.conv_can_mfma(x, x.shape[1], self.conv.out_channels, 3, 1, 1, dt)
            y = ops.conv2d(x, self._stem6_packed(dt, not mfma, raw=True), 1, ops.ACT_NONE)
        else:
            mfma = ops.conv_can_mfma(x, self.conv.in_channels, self.conv.out_channels, k, s, self.conv.groups, dt)
            pk = self._cached(('raw', dt, not mfma), [self.conv.weight],
                              lambda: ops.PackedConv(self.conv.weight, None, None, k, dt, direct=not mfma, groups=self.conv.groups))
            if x2 is not None and not mfma:
                raise RuntimeError('Conv.train_fwd: the fused pre-add needs the MFMA path (NHWC input, cin % 4 == 0)')
            y = ops.conv2d(x, pk, s, ops.ACT_NONE, x2=x2)
        bn = self.bn
        mean, rstd = ops.bn_stats(y, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
        z = ops.bn_act(y, mean, rstd, bn.weight, bn.bias, act_code(self.act), out=out, r1=r1, r2=r2)
        self._save_ctx((x, x2, y, mean, rstd, k, s))
        return z

    def backward(self, gz, need_dx=True, dx_out=None, acc=False, r2=None):
        """gz: grad w.r.t. the pre-residual output.  Fills .grad of conv.weight / bn.weight / bn.bias (overwrite), returns dx
        (written into the view `dx_out` when given; `acc`: added to what dx_out holds; `r2`: one more addend, e.g. a shortcut's gradient -
        both fused into the data-gradient convolution's epilogue)."""
        x, x2, y, mean, rstd, k, s = self._ctx.pop()
        if k == 6:
            return self._backward_stem6(gz, x, y, mean, rstd, need_dx)
        if self.conv.groups != 1:
            return self._backward_grouped(gz, x, y, mean, rstd, k, s, need_dx, dx_out, acc, r2)
        bn = self.bn
        ops.grad_buf(bn.weight)
        ops.grad_buf(bn.bias)
        dy = ops.bn_act_bwd(gz, y, mean, rstd, bn.weight, bn.bias, act_code(self.act), bn.weight.grad, bn.bias.grad)
        ops.grad_buf(self.conv.weight)
        ops.conv_wgrad(x, dy, k, s, self.conv.weight.grad, x2=x2)
        if not need_dx:
            return None
        dx = dx_out if dx_out is not None else ops.new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], dy.dtype, dy.device)
        return ops.conv_dgrad(dy, self.conv.weight, k, s, dx, accumulate=bool(acc and dx_out is not None), r2=r2)

    def _backward_stem6(self, gz, sd, y, mean, rstd, need_dx):
        """the 6x6 stem: the 3x3 weight-gradient kernel over the space-to-depth map `sd`, then the inverse permutation of its final sums into
        conv.weight.grad's (cout, c1, 6, 6) layout (ops.stem6_wgrad_unpack flushes deferred sums first).  Layer 0 never needs dx."""
        if need_dx:
            raise RuntimeError('Conv.backward: the 6x6 stem has no data gradient (it reads the image: call backward(g, need_dx=False))')
        bn = self.bn
        dy = ops.bn_act_bwd(gz, y, mean, rstd, bn.weight, bn.bias, act_code(self.act), ops.grad_buf(bn.weight), ops.grad_buf(bn.bias))
        dw3 = torch.empty((self.conv.out_channels, sd.shape[1], 3, 3), dtype=torch.float32, device=sd.device)      # 9 KB scratch per step (captured: the graph's pool)
        ops.conv_wgrad(sd, dy, 3, 1, dw3)
        # stem6_wgrad_unpack flushes ALL pending deferred weight-gradient sums, not only dw3's.  That is always correct (a flush only moves the one
        # final-sum launch forward) and costs nothing where this geometry occurs: the conv reads the image, so it is layer 0, the last layer of
        # the reverse pass, and the flush is the one BaseModel.backward would issue right after.  Elsewhere in a graph it would split that launch in two.
        ops.stem6_wgrad_unpack(dw3, ops.grad_buf(self.conv.weight))
        return None

    def _backward_grouped(self, gz, x, y, mean, rstd, k, s, need_dx, dx_out, acc, r2):
        """DWConv / Conv with g > 1 (conv.py:82-86): the grouped VALU kernels (weight [cout][cin/g][k][k]); not on any target YAML."""
        bn, g = self.bn, self.conv.groups
        dy = ops.bn_act_bwd(gz, y, mean, rstd, bn.weight, bn.bias, act_code(self.act), ops.grad_buf(bn.weight), ops.grad_buf(bn.bias))
        ops.gconv_wgrad(x, dy, k, s, g, ops.grad_buf(self.conv.weight))
        if not need_dx:
            return None
        dx = dx_out if dx_out is not None else ops.new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], dy.dtype, dy.device)
        ops.gconv_dgrad(dy, self.conv.weight, k, s, g, dx, accumulate=bool(acc and dx_out is not None))
        return dx if r2 is None else ops.add(dx, r2, out=dx)

    def forward_fuse(self, x):
        """After BaseModel.fuse(): `bn` is gone and `conv` carries the folded weight + bias (conv.py:40-42)."""
        return self.run(x)


class DWConv(Conv):
    """Depth-wise convolution (reference conv.py:82-86): registry entry, direct kernel."""

    def __init__(self, c1, c2, k=1, s=1, d=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), d=d, act=act)


class ConvTranspose2d(HipModule, nn.ConvTranspose2d):
    """`nn.ConvTranspose2d` rows of a YAML (models/v6/yolov6.yaml:39,45: [c2, 2, 2, 0]): the torch class as parameter container (state_dict keys
    `weight` (c1, c2, 2, 2) and `bias`, what a reference checkpoint holds), compute on the device.  Only kernel 2, stride 2, padding 0, one group,
    with a bias is built (ops.check_deconv2x2): anything else raises here, before any launch.
    forward: ops.deconv2x2 over four panels packed from the live weight (ops.PackedDeconv2x2Live: the trainer's ops.repack_all() refreshes them).
    backward: db (the bias-only mode of bn_act_bwd, which also leaves a dense copy of the incoming gradient), dW and dx (ops.deconv2x2_wgrad /
    ops.deconv2x2_dgrad): three launches plus the layer's share of the batched final sum where both gradients take their one-launch kernel (32 channels);
    where dx composes by measurement (64 and 128 channels) it is four convolution launches over panels packed from the live weight, six launches in all."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        ops.check_deconv2x2(self.kernel_size, self.stride, self.padding, self.groups, self.output_padding, self.dilation)
        if self.bias is None:
            raise RuntimeError('transposed convolution: only the form with a bias is built (nn.ConvTranspose2d(c1, c2, 2, 2, 0)), got bias=False')

    def forward(self, x, out=None):
        """`out`: an NHWC view (B, c2, 2H, 2W) to write into (e.g. this layer's channels of the following Concat's buffer); allocated when None"""
        dt = self.out_dtype(x) if out is None else out.dtype
        pk = self._cached(('deconv', dt), [self.weight, self.bias], lambda: ops.PackedDeconv2x2Live(self.weight, self.bias, dt))
        if self.training:
            self._save_ctx(x)
        return ops.deconv2x2(x, pk, out=out)

    def backward(self, g, need_dx=True, dx_out=None, acc=False, r2=None):
        """g: grad w.r.t. the output.  Fills .grad of weight / bias (overwrite), returns dx (same `dx_out` / `acc` / `r2` forms as Conv.backward)."""
        x = self._ctx.pop()
        dy = ops.bn_act_bwd(g, g, None, None, None, self.bias, ops.ACT_NONE, None, ops.grad_buf(self.bias))     # db = sum of g; dy = g, dense
        ops.deconv2x2_wgrad(x, dy, ops.grad_buf(self.weight))
        if not need_dx:
            return None
        dx = dx_out if dx_out is not None else ops.new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], dy.dtype, dy.device)
        return ops.deconv2x2_dgrad(dy, self.weight, dx, accumulate=bool(acc and dx_out is not None), r2=r2)


class MaxPool2d(HipModule, nn.MaxPool2d):
    """`nn.MaxPool2d` rows of a YAML (models/v3/yolov3-tiny.yaml: [2, 2, 0] and [2, 1, 0]): the torch class as a parameter-free container, compute on
    the device.  Only kernel 2 with stride 2 or 1, padding 0, dilation 1, ceil_mode=False, return_indices=False is built (ops.check_maxpool2d): anything
    else raises here, before any launch.  Output size floor((H - 2) / s) + 1: with stride 2 an odd trailing row or column is not read.
    forward: ops.maxpool2d (ATen's values: a NaN in a window is its maximum).  backward: ops.maxpool2d_bwd recomputes the argmax from the input, the
    only context the layer keeps (no index tensor), and gathers - the first maximum in scan order takes the gradient, pixels no window read get zero."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._k, self._s = ops.check_maxpool2d(self.kernel_size, self.stride, self.padding, self.dilation, self.ceil_mode, self.return_indices)

    def forward(self, x, out=None):
        if self.training:
            self._save_ctx(x)
        return ops.maxpool2d(x, self._k, self._s, out=out)

    def backward(self, g, dx_out=None):
        """g: grad w.r.t. the output -> grad w.r.t. the input, in the activation dtype (written to `dx_out` when given)"""
        x = self._ctx.pop()
        return ops.maxpool2d_bwd(x, g, self._k, self._s, gx=dx_out)


class ZeroPad2d(HipModule, nn.ZeroPad2d):
    """`nn.ZeroPad2d` rows of a YAML (models/v3/yolov3-tiny.yaml: [[0, 1, 0, 1]]): non-negative (left, right, top, bottom).  forward: a zero-filled NHWC
    map of the padded size and one ops.copy into its interior view; backward: the interior view of the incoming gradient (no launch, no copy).  The
    consumer sees the pad as ordinary zeros: a max pool behind it whose first maximum is a pad zero sends that gradient here, and the view drops it."""

    def __init__(self, padding):
        super().__init__(padding)
        if len(self.padding) != 4 or any((not isinstance(p, int)) or p < 0 for p in self.padding):
            raise RuntimeError(f'ZeroPad2d: four non-negative integers (left, right, top, bottom) are built, got {self.padding}')

    def _interior(self, t, h, w):
        left, _, top, _ = self.padding
        return t[:, :, top:top + h, left:left + w]

    def forward(self, x):
        b, c, h, w = x.shape
        left, right, top, bottom = self.padding
        out = ops.new_act(b, c, h + top + bottom, w + left + right, x.dtype, x.device).zero_()
        ops.copy(x, self._interior(out, h, w))
        return out

    def backward(self, g):
        left, right, top, bottom = self.padding
        return self._interior(g, g.shape[2] - top - bottom, g.shape[3] - left - right)


class Repeat(nn.Sequential):
    """A YAML row with repeats n > 1 of a module that does not take n itself (models/v6/yolov6.yaml: `[-1, 6, Conv, [128, 3, 1]]`): the reference's bare
    nn.Sequential (same state_dict keys `0.conv.weight`, ...; every isinstance(m, nn.Sequential) test holds) with the reverse pass the layer loop needs."""

    def backward(self, g, need_dx=True):
        """children in reverse order; `need_dx=False` (the row is layer 0) is handed to the first child"""
        mods = list(self)
        for k in range(len(mods) - 1, -1, -1):
            m = mods[k]
            if not hasattr(m, 'backward'):
                raise NotImplementedError(f'{type(m).__name__}.backward is not built yet (training path of this module: next)')
            g = m.backward(g, need_dx=False) if (k == 0 and not need_dx and isinstance(m, (Conv, ConvTranspose2d))) else m.backward(g)
        return g if need_dx else None


class Concat(nn.Module):
    """Concatenate along a dimension (reference conv.py:287-297); channel concat of NHWC maps on device."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def backward(self, g):
        """Adjoint of the channel concat: channel-slice views of g (no copies)."""
        out, c0 = [], 0
        for c in self._split:
            out.append(g[:, c0:c0 + c])
            c0 += c
        return out

    def forward(self, x):
        if self.d != 1:
            raise RuntimeError('Concat: only channel concatenation (dimension=1) is on the detection path')
        self._split = [t.shape[1] for t in x]
        b, _, h, w = x[0].shape
        out = ops.new_act(b, sum(t.shape[1] for t in x), h, w, x[0].dtype, x[0].device)
        c0 = 0
        for t in x:
            ops.copy(t, out[:, c0:c0 + t.shape[1]])
            c0 += t.shape[1]
        return out
