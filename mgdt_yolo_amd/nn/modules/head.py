"""Detect head (reference: nn/modules/head.py:133-186), compute on MI355X via libmgdt_hip.so.

Per level the box branch (3x3, 3x3, 1x1+bias -> 4*reg_max) and the class branch (3x3, 3x3, 1x1+bias -> nc) write
straight into the two channel ranges of one (B, no, H, W) NHWC map (the reference's torch.cat at head.py:160).
Eval: one decode kernel per level does DFL softmax-expectation + dist2bbox + stride scaling + sigmoid and
writes y (B, 4+nc, A) fp32.
"""
import math

import torch
import torch.nn as nn

from ... import ops
from .block import DFL, Proto
from .conv import Conv, HipModule, fp8_claims, merged_panel, plain, watched

__all__ = ('Detect', 'Segment', 'Pose', 'Classify', 'RTDETRDecoder', 'TOODHead', 'Conv_GN', 'TaskDecomposition', 'DyDCNv2', 'Scale')


class _HeadConv(HipModule):
    """The head's final `nn.Conv2d(c, out, 1)` with bias: parameter container + packed 1x1 MFMA conv."""

    @staticmethod
    def run(owner, conv, x, out):
        # class counts that are not a multiple of 4 (the fork's own data: nc = 1 or 2) give raw maps whose pixel rows are not 8-byte aligned:
        # those go through the direct kernel (element-wise stores), everything else through the MFMA kernel
        q = 4
        mfma = (conv.out_channels % q == 0 and out.stride(3) % q == 0 and out.stride(2) % q == 0 and out.stride(0) % q == 0 and
                out.data_ptr() % (q * out.element_size()) == 0 and
                ops.conv_can_mfma(x, conv.in_channels, conv.out_channels, 1, 1, 1, out.dtype))
        pk = owner._cached((id(conv), out.dtype, mfma), [conv.weight, conv.bias],
                           lambda: ops.PackedConv(conv.weight, conv.bias, None, 1, out.dtype, direct=not mfma))
        return ops.conv2d(x, pk, 1, ops.ACT_NONE, out=out)

    @staticmethod
    def panel(owner, conv, dt):
        """the plain MFMA panel of a final conv, as the Detect tail launch reads it"""
        return owner._cached((id(conv), dt), [conv.weight, conv.bias], lambda: ops.PackedConv(conv.weight, conv.bias, None, 1, dt))

    @staticmethod
    def backward(conv, x, g, accumulate=False):
        """Plain conv + bias: fills (or adds to: a head shared by several levels) conv.weight.grad / conv.bias.grad, returns dx."""
        ops.grad_buf(conv.weight)
        ops.grad_buf(conv.bias)
        ops.conv_wgrad(x, g, 1, 1, conv.weight.grad, dbias=conv.bias.grad, accumulate=accumulate)
        dx = ops.new_act(x.shape[0], x.shape[1], x.shape[2], x.shape[3], x.dtype, x.device)
        return ops.conv_dgrad(g, conv.weight, 1, 1, dx)


class Detect(HipModule):
    """YOLOv8 Detect head for detection models (this fork: reg_max = 4, head.py:145)."""
    dynamic = False
    export = False
    shape = None
    anchors = torch.empty(0)
    strides = torch.empty(0)

    def __init__(self, nc=80, ch=()):
        super().__init__()
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 4
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], self.nc)
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * self.reg_max, 1)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, self.nc, 1)) for x in ch)
        self.dfl = DFL(self.reg_max) if self.reg_max > 1 else nn.Identity()

    def forward(self, x):
        """Train: list of (B, no, H, W) raw maps.  Eval: (y (B, 4+nc, A), that list).  Mutates the input list in place
        like the reference (head.py:160)."""
        shape = x[0].shape
        r4 = 4 * self.reg_max
        y, a_off = None, 0
        strides = None if self.training else self._cached('stride_list', [self.stride], lambda: [float(v) for v in self.stride.tolist()])  # host copy, no sync per call
        tta = None if self.training else self.__dict__.get('_tta')     # one pass of DetectionModel._predict_augment
        aug = None if tta is None else tta['aug']
        if tta is not None:
            y, best, a_off = tta['y'], tta['best'], tta['a_off']
        elif not self.training:
            a_total = sum(t.shape[2] * t.shape[3] for t in x)
            y = torch.empty(shape[0], 4 + self.nc, a_total, dtype=torch.float32, device=x[0].device)
            best = torch.empty(shape[0], a_total, dtype=torch.int64, device=x[0].device)      # NMS keys of the anchors' best classes (detect tail)
        decoded = [False] * self.nl
        offs = [None] * self.nl
        for i in range(self.nl):
            if tta is not None and i not in tta['levels']:
                continue                                      # every anchor of this level is clipped away (_clip_augmented): not run
            offs[i] = a_off
            xi = x[i]
            b, _, h, w = xi.shape
            feat = ops.new_act(b, self.no, h, w, self.cv2[i][0].out_dtype(xi), xi.device)
            pk01 = None if self.training else self._merged_first(i, xi, feat.dtype)
            if pk01 is not None:                              # both branches' first 3x3 conv read xi: one launch, cout = c2 + c3
                xq = self.q8_site(('first01', i), xi) if feat.dtype == torch.bfloat16 else None
                t01 = ops.conv2d(xi, pk01, 1, ops.ACT_SILU) if xq is None else ops.conv2d_fp8(xi, self._merged_first(i, xi, feat.dtype, xq), 1, ops.ACT_SILU)
                c2 = self.cv2[i][0].conv.out_channels
                tc = self.cv3[i][1](t01[:, c2:])
                box3 = self._box3_in_tail(i, t01[:, :c2], tc, feat.dtype)
                if box3 is not None:
                    # the box branch's second 3x3 conv (16 -> 16) runs inside the tail launch: its input is handed over instead of its output
                    pk3, pkb_pad = box3
                    ops.detect_tail(t01[:, :c2], tc, pkb_pad, _HeadConv.panel(self, self.cv3[i][2], feat.dtype), self.nc, strides[i], a_off, feat, y, best, pk3=pk3, aug=aug)
                    decoded[i] = True
                    a_off += h * w
                    x[i] = feat
                    continue
                tb = self.cv2[i][1](t01[:, :c2])
            else:
                tb = self.cv2[i][1](self.cv2[i][0](xi))      # Conv.forward: eval -> fused run, train -> batch-stat BN + ctx
                tc = self.cv3[i][1](self.cv3[i][0](xi))
            if not self.training and ops.detect_tail_supported(tb, tc, self.nc, self.reg_max, feat.dtype):
                # both final 1x1 convs, the raw map and the decode in one launch (mgdt_detect_tail_fwd)
                ops.detect_tail(tb, tc, _HeadConv.panel(self, self.cv2[i][2], feat.dtype), _HeadConv.panel(self, self.cv3[i][2], feat.dtype), self.nc, strides[i], a_off,
                                feat, y, best, aug=aug)
                decoded[i] = True
            else:
                _HeadConv.run(self, self.cv2[i][2], tb, feat[:, :r4])
                _HeadConv.run(self, self.cv3[i][2], tc, feat[:, r4:])
            if self.training:
                self._save_ctx((tb, tc))
            else:
                a_off += h * w
            x[i] = feat
        if self.training:
            return x
        if tta is not None:
            for i in tta['levels']:
                if not decoded[i]:
                    ops.detect_decode(x[i], self.reg_max, self.nc, strides[i], offs[i], y, aug=aug, best=best)
            return y, x
        if self.dynamic or self.shape != shape:
            from ...yolo.utils.tal import make_anchors
            self.anchors, self.strides = (t.transpose(0, 1) for t in make_anchors(x, strides, 0.5))
            self.shape = shape
        a_off = 0
        for i, f in enumerate(x):
            if not decoded[i]:
                ops.detect_decode(f, self.reg_max, self.nc, strides[i], a_off, y)
            a_off += f.shape[2] * f.shape[3]
        if all(decoded):
            ops.attach_best_keys(y, best)        # every level went through the tail kernel: non_max_suppression(y) skips its best-class scan
        return y if self.export else (y, x)

    def _box3_in_tail(self, i, tb_in, tc, dt):
        """(panel of cv2[i][1], zero-padded accumulator-order panel of cv2[i][2]) when the box branch's second conv can run inside the Detect tail
        launch: eval, bf16, 16 -> 16 channels, a plain 3x3 conv nobody watches and fp8 does not own (it is a site of its own), reg_max 4; else None."""
        m3, m1 = self.cv2[i][1], self.cv2[i][2]
        if (self.training or not ops.FUSED_DETECT_BOX3 or dt != torch.bfloat16 or not plain(m3, 3) or m3.conv.in_channels != 16 or m3.conv.out_channels != 16
                or watched(m3) or fp8_claims(m3) or tb_in.shape[1] != 16 or not ops.detect_tail_supported(tb_in, tc, self.nc, self.reg_max, dt)):
            return None
        pk3 = m3.packed(dt, direct=False)

        def pad_pack():
            w = m1.weight.detach().float().reshape(m1.out_channels, 16)
            wp = torch.zeros(m1.out_channels, 32, device=w.device)
            wp[:, :16] = w                                     # channels 16..31 do not exist: zero weights
            return ops.PackedConv(wp[:, ops.acc_order_index(32, w.device)].reshape(m1.out_channels, 32, 1, 1), m1.bias, None, 1, dt)
        return pk3, self._cached((id(m1), dt, 'acc32'), [m1.weight, m1.bias], pad_pack)

    def _merged_first(self, i, xi, dt, xq=None):
        """PackedConv of cat(cv2[i][0], cv3[i][0]) along cout, or None when the pair is not two plain 3x3 convolutions the MFMA kernel takes.  An fp8 site
        of its own (`xq`: its e4m3 panel); hooks on the two are not consulted."""
        a, b = self.cv2[i][0], self.cv3[i][0]
        if (not (plain(a, 3) and plain(b, 3)) or a.conv.out_channels % 8
                or not ops.conv_can_mfma(xi, a.conv.in_channels, a.conv.out_channels + b.conv.out_channels, 3, 1, 1, dt)):
            return None
        return merged_panel(self, ('first01', i), a, b, 3, dt, xq)

    def backward(self, grads):
        """grads: list of d loss / d raw head maps (one per level, NHWC).  Returns the list of input gradients."""
        r4 = 4 * self.reg_max
        ctx = [self._ctx.pop() for _ in range(self.nl)][::-1]
        out = []
        for i, g in enumerate(grads):
            tb, tc = ctx[i]
            gb = self.cv2[i][0].backward(self.cv2[i][1].backward(_HeadConv.backward(self.cv2[i][2], tb, g[:, :r4])))
            gc = self.cv3[i][0].backward(self.cv3[i][1].backward(_HeadConv.backward(self.cv3[i][2], tc, g[:, r4:])))
            out.append(ops.add(gb, gc, out=gb))
        return out

    def bias_init(self):
        """Initialize Detect() biases (reference head.py:179-186); requires stride availability."""
        for a, b, s in zip(self.cv2, self.cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[:self.nc] = math.log(5 / self.nc / (640 / s) ** 2)


SEG_TRAIN_MSG = ('segmentation training is not built: the reference\'s v8SegmentationLoss cannot run in this fork, so there is nothing to pin a '
                 'training path to; Segment / SegmentationModel are inference modules (call .eval())')


class Segment(Detect):
    """YOLOv8 Segment head (reference head.py:189-212): Detect plus, per level, a mask-coefficient branch cv4 (3x3, 3x3, 1x1 + bias -> nm) and the
    Proto module on the first level.  Eval returns (cat(y, mc) (B, 4+nc+nm, A) fp32, (feats, mc (B, nm, A) fp32, p (B, nm, mh, mw) NHWC));
    export=True returns (cat, p).  Detect.forward runs unchanged; one launch (mgdt_seg_concat_fwd) then writes the wide prediction from its y and
    the NHWC cv4 maps, and the best-class NMS keys are carried over to it.  All convolutions of this head stay bf16 under quantize_fp8."""

    def __init__(self, nc=80, nm=32, npr=256, ch=()):
        super().__init__(nc, ch)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        c4 = max(ch[0] // 4, self.nm)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nm, 1)) for x in ch)

    def q8_site(self, key, x, x2=None):
        return None                                           # fp8 for the Segment head is not built: its merged first convolutions stay bf16

    def forward(self, x):
        if self.training:
            raise NotImplementedError(SEG_TRAIN_MSG)
        p = self.proto(x[0])
        mcs = []
        for i in range(self.nl):
            t = self.cv4[i][1](self.cv4[i][0](x[i]))
            b, _, h, w = t.shape
            m = ops.new_act(b, self.nm, h, w, t.dtype, t.device)
            _HeadConv.run(self, self.cv4[i][2], t, m)
            mcs.append(m)
        export, self.export = self.export, False             # Detect.forward's own export form drops the feature maps
        try:
            y, feats = Detect.forward(self, x)
        finally:
            self.export = export
        cat = ops.seg_concat(y, mcs)
        best = ops._best_keys_of(y, y.shape[0], y.shape[2])
        if best is not None:
            ops.attach_best_keys(cat, best)
        mc = cat[:, 4 + self.nc:]
        return (cat, p) if self.export else (cat, (feats, mc, p))

    def backward(self, grads):
        raise NotImplementedError(SEG_TRAIN_MSG)


POSE_TRAIN_MSG = ('pose training is not built: the reference\'s v8PoseLoss calls the assigner with the old signature and cannot run in this fork, so '
                  'there is nothing to pin a training path to; Pose / PoseModel are inference modules (call .eval())')


def padded_conv_params(m, cin_p, cout_p):
    """(weight (cout_p, cin_p, k, k), conv bias or None, BatchNorm tuple or None) of `m` (a Conv before or after fuse(), or a plain nn.Conv2d) with its
    channels zero-padded: padded input channels meet zero weights; padded output channels have zero weights, zero bias and the identity BatchNorm
    (gamma 1, beta 0, mean 0, var 1: folded scale * 0 = 0, folded shift 0), so they carry act(0) = 0 for SiLU and no real channel changes by a bit.
    Works on whatever device the parameters live on."""
    conv = m.conv if isinstance(m, Conv) else m
    w = conv.weight.detach().float()
    cout, cin = w.shape[:2]
    if cout_p < cout or cin_p < cin:
        raise RuntimeError(f'padded_conv_params: cannot pad {cout}x{cin} channels down to {cout_p}x{cin_p}')
    wp = w.new_zeros(cout_p, cin_p, *w.shape[2:])
    wp[:cout, :cin] = w
    pad = lambda t, fill: None if t is None else torch.cat([t.detach().float(), torch.full((cout_p - cout,), fill, dtype=torch.float32, device=t.device)])
    bn = None
    if isinstance(m, Conv) and hasattr(m, 'bn'):
        bn = (pad(m.bn.weight, 1.0), pad(m.bn.bias, 0.0), pad(m.bn.running_mean, 0.0), pad(m.bn.running_var, 1.0), m.bn.eps)
    return wp, pad(conv.bias, 0.0), bn


class Pose(Detect):
    """YOLOv8 Pose head (reference head.py:215-253): Detect plus, per level, a keypoint branch cv4 (3x3, 3x3, 1x1 + bias -> nk = kpt_shape[0] *
    kpt_shape[1]).  Eval returns (cat(y, pred_kpt) (B, 4+nc+nk, A) fp32, (feats, kpt (B, nk, A) fp32 raw)); export=True returns the concatenated
    tensor alone.  Detect.forward runs unchanged; one launch (mgdt_pose_concat_fwd) then decodes the keypoints and writes the wide prediction from
    its y and the NHWC cv4 maps, and the best-class NMS keys are carried over to it.  c4 = max(ch[0] // 4, nk) is 51 for kpt_shape (17, 3) at the
    n, s and m scales, which the MFMA convolution does not take (cin % 8, cout % 4): the branch then runs on it over zero-padded panels (56 hidden,
    52 output channels, `padded_conv_params`), see ops.POSE_PAD_MFMA.  All convolutions of this head stay bf16 under quantize_fp8."""

    def __init__(self, nc=80, kpt_shape=(17, 3), ch=()):
        super().__init__(nc, ch)
        self.kpt_shape = kpt_shape
        self.nk = kpt_shape[0] * kpt_shape[1]
        c4 = max(ch[0] // 4, self.nk)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nk, 1)) for x in ch)

    def q8_site(self, key, x, x2=None):
        return None                                           # fp8 for the Pose head is not built: its merged first convolutions stay bf16

    def _kpt_padded(self, i, xi):
        """zero-padded panels on the MFMA convolution: two plain 3x3 convs nobody watches + a dense 1x1; fp8 is not consulted (q8_site above: the head stays bf16)"""
        c0, c1, c2 = self.cv4[i]
        c4, c4p = c2.in_channels, -(-c2.in_channels // 8) * 8
        return bool(ops.POSE_PAD_MFMA and (c4p != c4 or self.nk % 4) and plain(c0, 3) and plain(c1, 3) and not watched(c0, c1) and c2.kernel_size == (1, 1)
                    and c2.groups == 1 and ops.conv_can_mfma(xi, c0.conv.in_channels, c4p, 3, 1, 1, c0.out_dtype(xi)))

    def _kpt_branch(self, i, xi):
        """cv4[i](xi) as an NHWC map whose first nk channels are the raw keypoints (52 channels on the padded route for nk = 51)."""
        c0, c1, c2 = self.cv4[i]
        dt = c0.out_dtype(xi)
        b, _, h, w = xi.shape
        c4, nk = c2.in_channels, self.nk
        c4p, nkp = -(-c4 // 8) * 8, -(-nk // 4) * 4
        if self._kpt_padded(i, xi):
            # panels packed from padded copies are derived copies (never refreshed in place): rebuilt whenever a live tensor they depend on changes
            pk0 = self._cached(('kpt', i, 0, dt), c0.affine_tensors(), lambda: ops.PackedConv(*padded_conv_params(c0, c0.conv.in_channels, c4p), 3, dt))
            pk1 = self._cached(('kpt', i, 1, dt), c1.affine_tensors(), lambda: ops.PackedConv(*padded_conv_params(c1, c4p, c4p), 3, dt))
            pk2 = self._cached(('kpt', i, 2, dt), [c2.weight, c2.bias], lambda: ops.PackedConv(*padded_conv_params(c2, c4p, nkp), 1, dt))
            t = ops.conv2d(ops.conv2d(xi, pk0, 1, ops.ACT_SILU), pk1, 1, ops.ACT_SILU)
            return ops.conv2d(t, pk2, 1, ops.ACT_NONE)
        t = c1(c0(xi))
        m = ops.new_act(b, nk, h, w, t.dtype, t.device)
        _HeadConv.run(self, c2, t, m)
        return m

    def forward(self, x):
        if self.training:
            raise NotImplementedError(POSE_TRAIN_MSG)
        kps = [self._kpt_branch(i, x[i]) for i in range(self.nl)]
        export, self.export = self.export, False             # Detect.forward's own export form drops the feature maps
        try:
            y, feats = Detect.forward(self, x)
        finally:
            self.export = export
        strides = self._cached('stride_list', [self.stride], lambda: [float(v) for v in self.stride.tolist()])
        cat, kpt = ops.pose_concat(y, kps, strides, self.nk, self.kpt_shape[1])
        best = ops._best_keys_of(y, y.shape[0], y.shape[2])
        if best is not None:
            ops.attach_best_keys(cat, best)
        return cat if self.export else (cat, (feats, kpt))

    def backward(self, grads):
        raise NotImplementedError(POSE_TRAIN_MSG)


class Classify(HipModule):
    """YOLOv8 classification head (reference head.py:256-272): x (b, c1, h, w) -> (b, c2).  `conv` (Conv c1 -> 1280), `pool`, `drop` (p = 0: the
    identity) and `linear` carry the reference's names, so state_dict keys and shapes match.  Eval returns the softmax (b, c2) fp32 in two launches:
    mgdt_classify_pool_fwd (conv + BatchNorm + SiLU + spatial mean, the 1280-channel map never stored) and mgdt_classify_linear_fwd (+ softmax);
    where the fused kernel does not apply (k != 1, groups, another activation, hooks, ops.FUSED_CLS_HEAD off) the unfused chain runs: Conv.forward,
    adaptive_avgpool, the linear as a 1x1 convolution on the (b, 1280, 1, 1) map, the softmax kernel.  Train returns the raw logits (b, c2) fp32
    through the unfused chain (batch-statistics BatchNorm in Conv.train_fwd) and keeps the context of `backward`."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        c_ = 1280                                             # efficientnet_b0 size
        self.conv = Conv(c1, c_, k, s, p, g)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.drop = nn.Dropout(p=0.0, inplace=True)
        self.linear = nn.Linear(c_, c2)

    def q8_site(self, key, x, x2=None):
        return None                                           # fp8 for the Classify head is not built

    def _fusable(self, x, dt):
        """eval, a plain 1x1 conv, nobody watching conv or pool; fp8 is not consulted: the Classify head stays bf16 under quantize_fp8 (q8_site above)"""
        cv = self.conv.conv
        return (not self.training and not watched(self.conv, self.pool) and plain(self.conv, 1)
                and ops.classify_pool_supported(x, cv.in_channels, cv.out_channels, 1, 1, ops.ACT_SILU, dt))

    def _pool_panel(self, dt):
        c = self.conv

        def build():
            if hasattr(c, 'bn'):
                from ...yolo.utils.torch_utils import fuse_conv_and_bn
                f = fuse_conv_and_bn(c.conv, c.bn)            # the arithmetic of BaseModel.fuse(): the panel is bit-equal before and after it
                return ops.PackedClsPool(f.weight, f.bias, dt)
            return ops.PackedClsPool(c.conv.weight, c.conv.bias, dt)
        return self._cached(('clspool', dt), c.affine_tensors(), build)

    def _linear_map(self, pm, dt):
        """the linear as a 1x1 convolution on the (b, 1280, 1, 1) map -> (b, nc, 1, 1); class counts the MFMA kernel does not take go the direct way"""
        lin, nc = self.linear, self.linear.out_features
        out = ops.new_act(pm.shape[0], nc, 1, 1, dt, pm.device)
        mfma = nc % 4 == 0 and ops.conv_can_mfma(pm, lin.in_features, nc, 1, 1, 1, dt)
        pk = self._cached(('lin1x1', dt, mfma), [lin.weight, lin.bias],
                          lambda: ops.PackedConv(lin.weight.reshape(nc, lin.in_features, 1, 1), lin.bias, None, 1, dt, direct=not mfma))
        return ops.conv2d(pm, pk, 1, ops.ACT_NONE, out=out)

    @staticmethod
    def _rows_f32(m):
        """(b, c, 1, 1) map -> contiguous (b, c) fp32"""
        b, c = m.shape[:2]
        if m.dtype == torch.float32:
            return m.reshape(b, c)
        out = torch.empty(b, c, 1, 1, dtype=torch.float32, device=m.device)
        return ops.copy(m, out).reshape(b, c)

    def forward(self, x):
        if isinstance(x, list):
            self._split = [t.shape[1] for t in x]
            b, _, h, w = x[0].shape
            cat = ops.new_act(b, sum(self._split), h, w, x[0].dtype, x[0].device)
            c0 = 0
            for t in x:
                ops.copy(t, cat[:, c0:c0 + t.shape[1]])
                c0 += t.shape[1]
            x = cat
        else:
            self._split = None
        dt = self.conv.out_dtype(x)
        if self._fusable(x, dt):
            lin = self.linear
            wl = self._cached(('lin', dt), [lin.weight], lambda: lin.weight.detach().to(dt).contiguous())
            bl = self._cached(('linb',), [lin.bias], lambda: None if lin.bias is None else lin.bias.detach().float().contiguous())
            return ops.classify_linear(ops.classify_pool(x, self._pool_panel(dt)), wl, bl, softmax=True)[1]
        z = self.conv(x)                                      # eval: folded BN; train: batch statistics + context
        pm = ops.adaptive_avgpool(z, ops.new_act(z.shape[0], z.shape[1], 1, 1, z.dtype, z.device))
        logits = self._rows_f32(self._linear_map(pm, z.dtype))
        if self.training:
            self._save_ctx((pm, tuple(z.shape)))
            return logits
        return ops.cls_softmax(logits)

    def backward(self, g):
        """g: d loss / d logits (b, nc).  Fills .grad of linear.weight / linear.bias and of `conv`; returns the gradient of the head's input (a list
        of channel slices for a list input)."""
        if isinstance(g, (list, tuple)):
            g = g[0]
        pm, zshape = self._ctx.pop()
        lin, nc = self.linear, self.linear.out_features
        b = pm.shape[0]
        gm = ops.new_act(b, nc, 1, 1, pm.dtype, pm.device)
        ops.copy(g.reshape(b, nc, 1, 1), gm)
        xw = pm
        if (nc % 4 or pm.shape[1] % 4) and pm.dtype != torch.float32:          # the generic weight-gradient kernel reads its input as fp32
            xw = ops.copy(pm, ops.new_act(b, pm.shape[1], 1, 1, torch.float32, pm.device))
        ops.grad_buf(lin.weight)
        if lin.bias is not None:
            ops.grad_buf(lin.bias)
        ops.conv_wgrad(xw, gm, 1, 1, lin.weight.grad, dbias=None if lin.bias is None else lin.bias.grad)
        dp = ops.conv_dgrad(gm, lin.weight, 1, 1, ops.new_act(b, pm.shape[1], 1, 1, pm.dtype, pm.device))
        gz = ops.adaptive_avgpool_bwd(dp, ops.new_act(*zshape, pm.dtype, pm.device))
        gx = self.conv.backward(gz)
        if self._split is None:
            return gx
        out, c0 = [], 0
        for c in self._split:
            out.append(gx[:, c0:c0 + c])
            c0 += c
        return out


# ====================================================================================================================
# TOODHead (reference nn/modules/head.py:466-572).  Inference on the HIP kernels; the task-aligned head is not trained here yet.
# Parity is unpinned: the reference needs mmcv (ModulatedDeformConv2d, ConvModule, Scale), which is not shipped with it and not
# installed, so no fixture can be generated - the DCNv2 kernel follows mmcv's published modulated_deform_conv kernel and the whole
# head is checked against `oracle/tood.py` (a restatement, not a reference run).
# ====================================================================================================================
class Scale(nn.Module):
    """mmcv.cnn.Scale: a learnable scalar (constructed by the reference head.py:490, unused by its forward)."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        raise RuntimeError('Scale is a parameter container only: TOODHead.forward never applies it (head.py:537)')


class Conv_GN(HipModule):
    """conv (no bias) + GroupNorm(16) + SiLU (reference head.py:67-81): MFMA conv, then the GroupNorm kernel with the activation."""
    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        if d != 1 or g != 1 or (p is not None and p != k // 2):
            raise RuntimeError('Conv_GN: only dense, dilation-1, same-padding convolutions are built')
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, groups=g, dilation=d, bias=False)
        self.gn = nn.GroupNorm(16, c2)
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()

    def forward(self, x, out=None):
        from .conv import act_code
        dt = self.out_dtype(x)
        k, st = self.conv.kernel_size[0], self.conv.stride[0]
        mfma = ops.conv_can_mfma(x, self.conv.in_channels, self.conv.out_channels, k, st, 1, dt)
        pk = self._cached(('raw', dt, not mfma), [self.conv.weight], lambda: ops.PackedConv(self.conv.weight, None, None, k, dt, direct=not mfma))
        y = ops.conv2d(x, pk, st, ops.ACT_NONE)
        z = ops.groupnorm(y, self.gn.weight.detach().float(), self.gn.bias.detach().float(), self.gn.num_groups, self.gn.eps, act_code(self.act), out=out)
        if self.training:
            self._save_ctx((x, y))
        return z

    def backward(self, g, accumulate=False):
        """d loss / d x; parameter gradients written, or added when `accumulate` (the head is shared by the levels)."""
        from .conv import act_code
        x, y = self._ctx.pop()
        for p in (self.conv.weight, self.gn.weight, self.gn.bias):
            ops.grad_buf(p)
        dy = ops.gn_act_bwd(g, y, self.gn.weight.detach().float(), self.gn.bias.detach().float(), self.gn.num_groups, self.gn.eps, act_code(self.act),
                            self.gn.weight.grad, self.gn.bias.grad, accumulate)
        k = self.conv.kernel_size[0]
        ops.conv_wgrad(x, dy, k, 1, self.conv.weight.grad, accumulate=accumulate)
        return ops.conv_dgrad(dy, self.conv.weight, k, 1, ops.like(x))


class _ConvModuleBias(nn.Module):
    """mmcv ConvModule(norm_cfg=None): `conv` with bias + ReLU `activate` - parameter container with the reference's key names."""

    def __init__(self, c1, c2):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, 1, bias=True)
        self.activate = nn.ReLU(inplace=True)


class TaskDecomposition(HipModule):
    """Layer attention folded into the 1x1 reduction conv (reference head.py:83-131, norm_cfg=None as TOODHead builds it):
    the per-image weights w[b, k] scale the reduction conv's weight block k == they scale input channel k*feat + j, which is the
    conv kernel's per-(image, channel) input scale."""

    def __init__(self, feat_channels, stacked_convs, la_down_rate=8, conv_cfg=None, norm_cfg=None):
        super().__init__()
        if norm_cfg is not None:
            raise RuntimeError('TaskDecomposition: norm_cfg is None everywhere in the reference head')
        self.feat_channels, self.stacked_convs = feat_channels, stacked_convs
        self.in_channels = feat_channels * stacked_convs
        self.la_conv1 = nn.Conv2d(self.in_channels, self.in_channels // la_down_rate, 1)
        self.relu = nn.ReLU(inplace=True)
        self.la_conv2 = nn.Conv2d(self.in_channels // la_down_rate, stacked_convs, 1, padding=0)
        self.sigmoid = nn.Sigmoid()
        self.reduction_conv = _ConvModuleBias(self.in_channels, feat_channels)

    def forward(self, feat, sums=None):
        """`sums` = sum_hw feat per (image, channel) (ops.nc_reduce), shared by the two decompositions like the reference's avg_feat."""
        f32 = lambda t: t.detach().float().reshape(t.shape[0], -1).contiguous()
        la = self._cached('la', [self.la_conv1.weight, self.la_conv1.bias, self.la_conv2.weight, self.la_conv2.bias],
                          lambda: (f32(self.la_conv1.weight), self.la_conv1.bias.detach().float().contiguous(), f32(self.la_conv2.weight),
                                   self.la_conv2.bias.detach().float().contiguous()))
        scale = ops.tood_layer_attn(feat, la[0], la[1], la[2], la[3], self.stacked_convs, sums=sums)
        rc = self.reduction_conv.conv
        dt = self.out_dtype(feat)
        # as written in the reference the bmm path uses only `.conv.weight`: reduction_conv's bias parameter is never added (head.py:117-127)
        pk = self._cached(('red', dt), [rc.weight], lambda: ops.PackedConv(rc.weight, None, None, 1, dt))
        out = ops.conv2d(feat, pk, 1, ops.ACT_RELU, in_scale=scale)
        if self.training:
            self._save_ctx((feat, scale, sums if sums is not None else ops.nc_reduce(feat), out, la))
        return out

    def backward(self, g, accumulate=False):
        """-> (t, scale, dsums): d loss / d feat = t * scale[n, c] + dsums[n, c] (the GAP branch, already divided by H*W); the caller sums the
        two decompositions in one pass."""
        feat, scale, sums, out, la = self._ctx.pop()
        rc = self.reduction_conv.conv
        for p in (rc.weight, self.la_conv1.weight, self.la_conv1.bias, self.la_conv2.weight, self.la_conv2.bias):
            ops.grad_buf(p)
        gr = ops.relu_mask(g, out)
        ops.conv_wgrad(ops.channel_affine(feat, scale, None), gr, 1, 1, rc.weight.grad, accumulate=accumulate)      # d W = sum (feat * scale) x g
        t = ops.conv_dgrad(gr, rc.weight, 1, 1, ops.like(feat))
        dscale = ops.nc_reduce(t, feat)
        dsums = ops.tood_layer_attn_bwd(sums, dscale, feat.shape[2] * feat.shape[3], la[0], la[1], la[2], la[3], self.stacked_convs,
                                        self.la_conv1.weight.grad, self.la_conv1.bias.grad, self.la_conv2.weight.grad, self.la_conv2.bias.grad, accumulate)
        return t, scale, dsums


class _DCNParams(nn.Module):
    """mmcv ModulatedDeformConv2d(in, out, 3, padding=1, bias=False) as a parameter container (weight (out, in, 3, 3))."""

    def __init__(self, c1, c2, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(c2, c1, 3, 3))
        self.bias = nn.Parameter(torch.zeros(c2)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)


class DyDCNv2(HipModule):
    """Modulated deformable conv 3x3 + GroupNorm(16) (reference block.py:401-432)."""

    def __init__(self, in_channels, out_channels, stride=1, norm_cfg=dict(type='GN', num_groups=16, requires_grad=True)):
        super().__init__()
        if stride != 1:
            raise RuntimeError('DyDCNv2: stride 1 only (the head never uses another)')
        self.with_norm = norm_cfg is not None
        self.conv = _DCNParams(in_channels, out_channels, bias=not self.with_norm)
        if self.with_norm:
            self.norm = nn.GroupNorm(norm_cfg.get('num_groups', 16), out_channels)

    def forward(self, x, offset_mask, act=ops.ACT_NONE):
        """offset_mask: (B, >=27, H, W) = 18 offsets + 9 mask LOGITS (the sigmoid of head.py:525 runs inside the kernel)."""
        cw = self.conv.weight
        if self.training:
            # training: the sampled-and-modulated columns are materialised once; the DCN is then the 1x1 conv of col with weight.view(cout, cin*9)
            if self.conv.bias is not None or not self.with_norm:
                raise NotImplementedError('DyDCNv2 training: only the normalised, bias-free form the head builds')
            dt = x.dtype
            col = ops.dcn_im2col(x, offset_mask)
            pk1 = self._cached(('col1x1', dt), [cw], lambda: ops.PackedConv(cw.detach().reshape(cw.shape[0], cw.shape[1] * 9, 1, 1), None, None, 1, dt))
            d = ops.conv2d(col, pk1, 1, ops.ACT_NONE)
            z = ops.groupnorm(d, self.norm.weight.detach().float(), self.norm.bias.detach().float(), self.norm.num_groups, self.norm.eps, act)
            self._save_ctx((x, offset_mask, col, d, act))
            return z
        wg = self._cached('gemm', [cw], lambda: cw.detach().float().permute(2, 3, 1, 0).reshape(9 * cw.shape[1], cw.shape[0]).contiguous())
        b = None if self.conv.bias is None else self.conv.bias.detach().float()
        if (b is None and x.dtype == torch.bfloat16 and offset_mask.dtype == x.dtype and cw.shape[1] % 8 == 0 and cw.shape[0] % 16 == 0 and cw.shape[0] <= 64
                and ops.is_nhwc(x) and ops.is_nhwc(offset_mask)):
            pk = self._cached('mfma', [cw], lambda: ops.PackedConv(cw, None, None, 3, torch.bfloat16))     # the ordinary fragment panel of a 3x3 conv
            y = ops.dcnv2_mfma(x, offset_mask, pk)
        else:
            y = ops.dcnv2(x, offset_mask, wg, b, cw.shape[0])
        if not self.with_norm:
            return y
        return ops.groupnorm(y, self.norm.weight.detach().float(), self.norm.bias.detach().float(), self.norm.num_groups, self.norm.eps, act, out=y)


    def backward(self, g, accumulate=False):
        """-> (d loss / d x, d loss / d offset_mask map)."""
        x, om, col, d, act = self._ctx.pop()
        cw = self.conv.weight
        for p in (cw, self.norm.weight, self.norm.bias):
            ops.grad_buf(p)
        gd = ops.gn_act_bwd(g, d, self.norm.weight.detach().float(), self.norm.bias.detach().float(), self.norm.num_groups, self.norm.eps, act,
                            self.norm.weight.grad, self.norm.bias.grad, accumulate)
        w1 = cw.detach().reshape(cw.shape[0], cw.shape[1] * 9, 1, 1)
        ops.conv_wgrad(col, gd, 1, 1, cw.grad.view(cw.shape[0], cw.shape[1] * 9, 1, 1), accumulate=accumulate)
        gcol = ops.conv_dgrad(gd, w1, 1, 1, ops.like(col))
        return ops.dcn_col2im_bwd(gcol, x, om)


class TOODHead(Detect):
    """Task-aligned dynamic detection head (reference head.py:466-572): shared Conv_GN stack, task decomposition, DCNv2-aligned box
    branch, probability-gated class branch; reg_max = 16.  Single shared head over all levels."""

    def __init__(self, nc, hidc, ch=()):
        HipModule.__init__(self)
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 16
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        if any(c != hidc for c in ch):
            raise RuntimeError(f'TOODHead: every input level must have hidc={hidc} channels, got {list(ch)} (the reference YAML passes hidc unscaled, '
                               'tasks.py:664-665)')
        self.share_conv = nn.Sequential(Conv_GN(hidc, hidc // 2, 3), Conv_GN(hidc // 2, hidc // 2, 3))
        self.cls_decomp = TaskDecomposition(hidc // 2, 2, 16)
        self.reg_decomp = TaskDecomposition(hidc // 2, 2, 16)
        self.DyDCNV2 = DyDCNv2(hidc // 2, hidc // 2)
        self.spatial_conv_offset = nn.Conv2d(hidc, 3 * 3 * 3, 3, padding=1)
        self.offset_dim = 2 * 3 * 3
        self.cls_prob_conv1 = nn.Conv2d(hidc, hidc // 4, 1)
        self.cls_prob_conv2 = nn.Conv2d(hidc // 4, 1, 3, padding=1)
        self.cv2 = nn.Conv2d(hidc // 2, 4 * self.reg_max, 1)
        self.cv3 = nn.Conv2d(hidc // 2, self.nc, 1)
        self.scale = nn.ModuleList(Scale(1.0) for _ in ch)
        self.dfl = DFL(self.reg_max) if self.reg_max > 1 else nn.Identity()

    def _bias_conv(self, conv, x, act, dt, pad_to=None):
        """nn.Conv2d with bias on the conv kernels; `pad_to` appends zero output channels so that cout % 4 == 0 (MFMA path)."""
        k = conv.kernel_size[0]

        def build():
            w, b = conv.weight.detach().float(), conv.bias.detach().float()
            if pad_to and pad_to > w.shape[0]:
                w = torch.cat([w, w.new_zeros(pad_to - w.shape[0], *w.shape[1:])])
                b = torch.cat([b, b.new_zeros(pad_to - b.shape[0])])
            mf = ops.conv_can_mfma(x, w.shape[1], w.shape[0], k, 1, 1, dt)
            return ops.PackedConv(w, b, None, k, dt, direct=not mf)
        pk = self._cached((id(conv), dt, pad_to), [conv.weight, conv.bias], build)
        return ops.conv2d(x, pk, 1, act)

    def forward(self, x):
        shape = x[0].shape
        r4 = 4 * self.reg_max
        tta = None if self.training else self.__dict__.get('_tta')     # one pass of DetectionModel._predict_augment
        for i in range(self.nl):
            if tta is not None and i not in tta['levels']:
                continue                                                # every anchor of this level is clipped away: not run
            xi = x[i]
            b, _, h, w = xi.shape
            dt = self.share_conv[0].out_dtype(xi)
            half = self.share_conv[0].conv.out_channels
            feat = ops.new_act(b, 2 * half, h, w, dt, xi.device)        # torch.cat(stack_res_list) = two channel slots
            self.share_conv[0](xi, out=feat[:, :half])
            self.share_conv[1](feat[:, :half], out=feat[:, half:])
            sums = ops.nc_reduce(feat)                                  # both decompositions share avg_feat = GAP(feat) (head.py:516)
            cls_feat = self.cls_decomp(feat, sums)
            reg_feat = self.reg_decomp(feat, sums)
            om = self._bias_conv(self.spatial_conv_offset, feat, ops.ACT_NONE, dt, pad_to=28)     # 18 offsets | 9 mask logits | pad
            reg_feat = self.DyDCNV2(reg_feat, om, act=ops.ACT_RELU)      # F.relu(reg_feat) of head.py:537 folded into the GroupNorm pass
            p1 = self._bias_conv(self.cls_prob_conv1, feat, ops.ACT_RELU, dt)
            prob = self._bias_conv(self.cls_prob_conv2, p1, ops.ACT_NONE, dt)
            out = ops.new_act(b, self.no, h, w, dt, xi.device)
            gated = ops.pixel_gate(cls_feat, prob)
            _HeadConv.run(self, self.cv2, reg_feat, out[:, :r4])
            _HeadConv.run(self, self.cv3, gated, out[:, r4:])
            if self.training:
                self._save_ctx(dict(feat=feat, half=half, om=om, reg_feat=reg_feat, cls_feat=cls_feat, p1=p1, prob=prob, gated=gated))
            x[i] = out
        if self.training:
            return x
        strides = self._cached('stride_list', [self.stride], lambda: [float(v) for v in self.stride.tolist()])
        if tta is not None:
            a_off = tta['a_off']
            for i in tta['levels']:
                ops.detect_decode(x[i], self.reg_max, self.nc, strides[i], a_off, tta['y'], aug=tta['aug'], best=tta['best'])
                a_off += x[i].shape[2] * x[i].shape[3]
            return tta['y'], x
        if self.dynamic or self.shape != shape:
            from ...yolo.utils.tal import make_anchors
            self.anchors, self.strides = (t.transpose(0, 1) for t in make_anchors(x, strides, 0.5))
            self.shape = shape
        a_total = sum(f.shape[2] * f.shape[3] for f in x)
        y = torch.empty(shape[0], 4 + self.nc, a_total, dtype=torch.float32, device=x[0].device)
        a_off = 0
        for i, f in enumerate(x):
            ops.detect_decode(f, self.reg_max, self.nc, strides[i], a_off, y)
            a_off += f.shape[2] * f.shape[3]
        return y if self.export else (y, x)

    def _bias_conv_bwd(self, conv, x, g, pad_to=None, accumulate=False):
        """Backward of _bias_conv (without its activation): parameter gradients (+=), returns dx."""
        ops.grad_buf(conv.weight)
        ops.grad_buf(conv.bias)
        k = conv.kernel_size[0]
        w = conv.weight
        if pad_to and pad_to > w.shape[0]:          # g carries the zero padding channels of the forward
            wp = self._cached(('wpad', id(conv), pad_to), [w], lambda: torch.cat([w.detach().float(), w.new_zeros(pad_to - w.shape[0], *w.shape[1:])]).contiguous())
            dwp = torch.empty_like(wp)
            dbp = torch.empty(pad_to, dtype=torch.float32, device=w.device)
            ops.conv_wgrad(x, g, k, 1, dwp, dbias=dbp)
            (conv.weight.grad.add_ if accumulate else conv.weight.grad.copy_)(dwp[:w.shape[0]])
            (conv.bias.grad.add_ if accumulate else conv.bias.grad.copy_)(dbp[:w.shape[0]])
            return ops.conv_dgrad(g, wp, k, 1, ops.like(x))
        ops.conv_wgrad(x, g, k, 1, conv.weight.grad, dbias=conv.bias.grad, accumulate=accumulate)
        return ops.conv_dgrad(g, w, k, 1, ops.like(x))

    def backward(self, grads):
        """grads: d loss / d raw maps, one per level.  The head is shared: the levels are walked last to first (every sub-module's saved-state
        stack is LIFO) and parameter gradients are written by the first level processed, accumulated by the others.  Parameters the reference's
        forward never touches (`scale.*`, `reduction_conv.conv.bias`) get zero gradients."""
        r4 = 4 * self.reg_max
        out = [None] * self.nl
        for p in [m.scale for m in self.scale] + [self.cls_decomp.reduction_conv.conv.bias, self.reg_decomp.reduction_conv.conv.bias]:
            ops.grad_buf(p).zero_()
        for step, i in enumerate(reversed(range(self.nl))):
            acc = step > 0
            c = self._ctx.pop()
            g = grads[i]
            feat, half = c['feat'], c['half']
            hw = feat.shape[2] * feat.shape[3]
            # box branch: cv2 <- reg_feat = relu(GN(DCN(reg_feat0, om)))   (ReLU folded into the GroupNorm backward)
            g_reg = _HeadConv.backward(self.cv2, c['reg_feat'], g[:, :r4], accumulate=acc)
            g_reg0, g_om = self.DyDCNV2.backward(g_reg, accumulate=acc)
            # class branch: cv3 <- cls_feat * sigmoid(prob)
            g_gated = _HeadConv.backward(self.cv3, c['gated'], g[:, r4:], accumulate=acc)
            # cls_prob_conv2 has ONE output channel: its gradient map is kept as channel 0 of a zero 4-channel map so that the weight-gradient
            # kernel sees 4-aligned channels (pad_to=4 below drops the padding rows again)
            gp4 = ops.new_act(g.shape[0], 4, g.shape[2], g.shape[3], g.dtype, g.device).zero_()
            g_cls, _ = ops.pixel_gate_bwd(g_gated, c['cls_feat'], c['prob'], glogit=gp4[:, :1])
            g_p1 = ops.relu_mask(self._bias_conv_bwd(self.cls_prob_conv2, c['p1'], gp4, pad_to=4, accumulate=acc), c['p1'])
            gf = self._bias_conv_bwd(self.cls_prob_conv1, feat, g_p1, accumulate=acc)                       # d feat, accumulated below
            gf = ops.add(gf, self._bias_conv_bwd(self.spatial_conv_offset, feat, g_om, pad_to=28, accumulate=acc), out=gf)
            # the two task decompositions (processed in reverse order of the forward: reg, then cls)
            t_r, s_r, ds_r = self.reg_decomp.backward(g_reg0, accumulate=acc)
            t_c, s_c, ds_c = self.cls_decomp.backward(g_cls, accumulate=acc)
            gd = ops.nc_axpby(t_c, s_c, t_r, s_r, ops.ew_add_nc(ds_c, ds_r))                                 # t_c*s_c + t_r*s_r + (dsums_c + dsums_r)[n, c]
            gf = ops.add(gf, gd, out=gf)
            # feat = [f0 | f1]: f1 = share_conv[1](f0), f0 = share_conv[0](x)
            g_f0 = self.share_conv[1].backward(gf[:, half:], accumulate=acc)
            g_f0 = ops.add(g_f0, gf[:, :half], out=g_f0)
            out[i] = self.share_conv[0].backward(g_f0, accumulate=acc)
        return out

    def bias_init(self):
        """reference head.py:562-568 (single shared head: the class prior uses stride 16)."""
        self.cv2.bias.data[:] = 1.0
        self.cv3.bias.data[:self.nc] = math.log(5 / self.nc / (640 / 16) ** 2)


# ====================================================================================================================
# RTDETRDecoder (reference nn/modules/head.py:275-464), inference only.
RTDETR_TRAIN_MSG = ('RT-DETR training is not built: the generation of the denoising query groups (vit/utils/ops.py get_cdn_group) and the reverse pass of the '
                    'decoder have no HIP counterpart here; RTDETRDecoder runs in eval() only.  The criterion exists on its own: RTDETRDetectionModel.detr_criterion(), '
                    'predict_layers() and loss_from_preds()')


class RTDETRDecoder(HipModule):
    """RT-DETR decoder head.  Submodules and parameters carry the reference's names (`input_proj.{i}.{0,1}`, `decoder.layers.{i}.self_attn.in_proj_weight`,
    `... .cross_attn.sampling_offsets`, `denoising_class_embed`, `query_pos_head`, `enc_output`, `enc_score_head`, `enc_bbox_head`, `dec_score_head.{i}`,
    `dec_bbox_head.{i}`); nn.Linear / nn.LayerNorm / nn.MultiheadAttention objects hold parameters only.

    Eval forward of a list of nl feature maps -> (dec_bboxes (1, B, nq, 4) xywh in [0, 1], dec_scores (1, B, nq, nc) after the sigmoid, enc_bboxes
    (B, nq, 4), enc_scores (B, nq, nc), None), all fp32, no host read.  Launches: nl input projections into one (B, L, 256) token memory; enc_output
    linear + masked LayerNorm; enc_score_head over all tokens, the per-token class maximum, the selection (`select_queries`: descending score, equal
    scores by ascending token index); the gather of the nq selected tokens and enc_bbox_head on those rows only; ONE value projection for all `ndl`
    decoder layers (an ndl*256-column panel over the memory); then per layer the query-position MLP, the q/k and v projections (the position added in the
    GEMM's input stage), self-attention, out_proj, add + LayerNorm, ONE panel for sampling offsets + attention weights, deformable attention, output_proj,
    add + LayerNorm, the FFN, add + LayerNorm, the box MLP and the box refinement; the last layer's score head and sigmoid.
    bf16 compute: the token memory, the enc_output linear's output and the projected values are bf16 in HBM and computed on the bf16 MFMA (everything of
    size L); the LayerNorm behind enc_output reads bf16 and writes fp32, and from there on (scores, selection, the whole query side) it is fp32.
    Built for hd = 256, nh = 8, ndp = 4, up to 4 levels; any nq, nc, ndl."""

    def __init__(self, nc=80, ch=(512, 1024, 2048), hd=256, nq=300, ndp=4, nh=8, ndl=6, d_ffn=1024, dropout=0., act=nn.ReLU(), eval_idx=-1,
                 nd=100, label_noise_ratio=0.5, box_noise_scale=1.0, learnt_init_query=False):
        super().__init__()
        from .transformer import MLP, DeformableTransformerDecoder, DeformableTransformerDecoderLayer
        if hd != 256 or nh != 8 or ndp != 4 or not 1 <= len(ch) <= 4:
            raise NotImplementedError(f'RTDETRDecoder: the HIP kernels are built for hd = 256, nh = 8, ndp = 4 and 1..4 levels, got hd = {hd}, nh = {nh}, '
                                      f'ndp = {ndp}, {len(ch)} levels')
        if learnt_init_query:
            raise NotImplementedError('RTDETRDecoder: learnt_init_query=True is not built (the queries are the selected encoder tokens)')
        if d_ffn % 4 or nq < 1 or ndl < 1 or nc < 1:
            raise ValueError(f'RTDETRDecoder: d_ffn = {d_ffn} (a multiple of 4), nq = {nq}, ndl = {ndl}, nc = {nc}')
        self.hidden_dim, self.nhead, self.nl, self.nc, self.num_queries, self.num_decoder_layers = hd, nh, len(ch), nc, nq, ndl
        self.input_proj = nn.ModuleList(nn.Sequential(nn.Conv2d(x, hd, 1, bias=False), nn.BatchNorm2d(hd)) for x in ch)
        self.decoder = DeformableTransformerDecoder(hd, DeformableTransformerDecoderLayer(hd, nh, d_ffn, dropout, act, self.nl, ndp), ndl, eval_idx)
        self.denoising_class_embed = nn.Embedding(nc, hd)
        self.num_denoising, self.label_noise_ratio, self.box_noise_scale = nd, label_noise_ratio, box_noise_scale
        self.learnt_init_query = learnt_init_query
        self.query_pos_head = MLP(4, 2 * hd, hd, num_layers=2)
        self.enc_output = nn.Sequential(nn.Linear(hd, hd), nn.LayerNorm(hd))
        self.enc_score_head = nn.Linear(hd, nc)
        self.enc_bbox_head = MLP(hd, hd, 4, num_layers=3)
        self.dec_score_head = nn.ModuleList([nn.Linear(hd, nc) for _ in range(ndl)])
        self.dec_bbox_head = nn.ModuleList([MLP(hd, hd, 4, num_layers=3) for _ in range(ndl)])
        self._reset_parameters()

    def _reset_parameters(self):
        """head.py:443-464: the constants are deterministic, the uniform draws are not pinned to the reference's random stream"""
        from torch.nn.init import constant_, uniform_, xavier_uniform_
        bias_cls = float(-math.log((1 - 0.01) / 0.01)) / 80 * self.nc
        constant_(self.enc_score_head.bias, bias_cls)
        constant_(self.enc_bbox_head.layers[-1].weight, 0.)
        constant_(self.enc_bbox_head.layers[-1].bias, 0.)
        for cls_, reg_ in zip(self.dec_score_head, self.dec_bbox_head):
            constant_(cls_.bias, bias_cls)
            constant_(reg_.layers[-1].weight, 0.)
            constant_(reg_.layers[-1].bias, 0.)
        lin = self.enc_output[0]
        bound = 1 / math.sqrt(lin.weight.shape[0])
        uniform_(lin.bias, -bound, bound)
        xavier_uniform_(lin.weight)
        xavier_uniform_(self.query_pos_head.layers[0].weight)
        xavier_uniform_(self.query_pos_head.layers[1].weight)
        for layer in self.input_proj:
            xavier_uniform_(layer[0].weight)

    def q8_site(self, key, x, x2=None):
        return None                                           # fp8 for the RT-DETR head is not built

    # -- dense linears on the implicit-GEMM convolution: a token matrix (B, N, C) is an NHWC map of height 1 -----------------------
    VIEW_BYTES = (1 << 31) - 1                                # the convolution addresses one view with 32-bit byte offsets: larger token matrices go in batch chunks

    @staticmethod
    def _as_map(t):
        """(B, N, C) -> (B, C, 1, N), channels innermost in memory; the unused stride of the height-1 dimension is one token, not the whole image"""
        b, n, c = t.shape
        return t.as_strided((b, c, 1, n), (t.stride(0), 1, t.stride(1), t.stride(1)), t.storage_offset())

    def _linear(self, key, x, cout, weight, bias, act=ops.ACT_NONE, x2=None, tensors=None):
        """act((x [+ x2]) @ weight^T + bias): x (B, N, cin) -> (B, N, cout), computed and stored in x's dtype (fp32, or bf16 for the token memory's
        consumers).  `weight` / `bias`: callables that build the (merged) panel's source when the panel is packed, `tensors`: the parameters it
        depends on."""
        b, n, cin = x.shape
        xm = self._as_map(x)
        dt = x.dtype
        mfma = cout % 4 == 0 and ops.conv_can_mfma(xm, cin, cout, 1, 1, 1, dt)
        if not mfma and dt != torch.float32:
            raise RuntimeError(f'RTDETRDecoder: the bf16 linear {key} ({cin} -> {cout}) is outside the MFMA route')
        if not mfma and x2 is not None:
            raise RuntimeError(f'RTDETRDecoder: the linear {key} ({cin} -> {cout}) is outside the MFMA route and cannot add its second input')
        pk = self._cached((key, mfma, dt), tensors, lambda: ops.PackedConv(weight().reshape(cout, cin, 1, 1), bias(), None, 1, dt, direct=not mfma))
        out = torch.empty(b, n, cout, dtype=dt, device=x.device)
        om, x2m = self._as_map(out), None if x2 is None else self._as_map(x2)
        step = max(1, self.VIEW_BYTES // (n * max(cin, cout, x.stride(1)) * x.element_size()))
        for b0 in range(0, b, step):
            ops.conv2d(xm[b0:b0 + step], pk, 1, act, out=om[b0:b0 + step], x2=None if x2m is None else x2m[b0:b0 + step])
        return out

    def _lin(self, key, x, lin, act=ops.ACT_NONE, x2=None):
        return self._linear(key, x, lin.out_features, lambda: lin.weight, lambda: lin.bias, act, x2, [lin.weight, lin.bias])

    def _mlp(self, key, x, mlp):
        for j, lin in enumerate(mlp.layers):
            x = self._lin((key, j), x, lin, ops.ACT_RELU if j < mlp.num_layers - 1 else ops.ACT_NONE)
        return x

    # -- encoder side ---------------------------------------------------------------------------------------------------------------
    def _encode(self, x):
        """feature maps -> (memory (B, L, 256), shapes, features (B, L, 256) after enc_output, class logits (B, L, nc), score_max (B, L))"""
        if self.training:
            raise NotImplementedError(RTDETR_TRAIN_MSG)
        if not isinstance(x, (list, tuple)) or len(x) != self.nl:
            raise RuntimeError(f'RTDETRDecoder: expected a list of {self.nl} feature maps')
        dt = self.out_dtype(x[0])
        if any(f.dtype != dt for f in x):
            raise RuntimeError(f'RTDETRDecoder: the feature maps must come in the compute dtype {dt}, got {[str(f.dtype) for f in x]}')
        b = x[0].shape[0]
        shapes = [(int(f.shape[2]), int(f.shape[3])) for f in x]
        L = sum(h * w for h, w in shapes)
        memory = torch.empty(b, L, self.hidden_dim, dtype=dt, device=x[0].device)
        off = 0
        for i, (f, (h, w)) in enumerate(zip(x, shapes)):
            conv, bn = self.input_proj[i][0], self.input_proj[i][1]
            self._no_train_bn(bn)
            if not ops.conv_can_mfma(f, conv.in_channels, self.hidden_dim, 1, 1, 1, dt):
                raise RuntimeError(f'RTDETRDecoder: input {i} ({tuple(f.shape)}, strides {f.stride()}) is outside the implicit-GEMM route (NHWC, channels % 4 == 0 in fp32, % 8 == 0 in bf16)')
            pk = self._cached(('proj', i, dt), [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var],
                              lambda conv=conv, bn=bn: ops.PackedConv(conv.weight, None, (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps), 1, dt))
            ops.conv2d(f, pk, 1, ops.ACT_NONE, out=memory[:, off:off + h * w].view(b, h, w, self.hidden_dim).permute(0, 3, 1, 2))
            off += h * w
        lin, ln = self.enc_output[0], self.enc_output[1]
        # a token whose anchor is invalid enters enc_output zeroed (head.py:408): its linear is the bias, which the LayerNorm launch substitutes
        feats = ops.add_layernorm(self._lin('enc_output', memory, lin), None, ln.weight, ln.bias, ln.eps, fill=lin.bias, shapes=shapes)
        logits = self._lin('enc_score', feats, self.enc_score_head)
        return memory, shapes, feats, logits, ops.rtdetr_rowmax(logits)

    def select_queries(self, x):
        """The query selection of head.py:416 as a public step: (index (B, nq) int64, score_max (B, L) fp32), both on the device.  torch.topk leaves
        the order of equal scores unspecified; here it is descending score, equal scores by ascending token index."""
        enc = self._encode(x)
        return ops.rtdetr_topk(enc[4], self.num_queries), enc[4]

    def forward(self, x, batch=None, query_index=None):
        if self.training or batch is not None:
            raise NotImplementedError(RTDETR_TRAIN_MSG)
        if self.__dict__.get('_select_only'):                 # RTDETRDetectionModel.select_queries
            return self.select_queries(x)
        if query_index is None:
            query_index = self.__dict__.get('_query_index')   # RTDETRDetectionModel.predict(query_index=...)
        return self._decode(x, query_index, bool(self.__dict__.get('_all_layers')))

    def forward_layers(self, x, query_index=None):
        """Eval only: the reference's training-layout tuple without denoising (head.py with self.training set and num_denoising = 0):
        (dec_bboxes (ndl, B, nq, 4) - the refined boxes after every decoder layer, dec_scores (ndl, B, nq, nc) RAW logits of every layer's score head,
        enc_bboxes (B, nq, 4), enc_scores (B, nq, nc) raw, None).  The launches are forward()'s, plus the score head on every layer and no sigmoid."""
        if self.training:
            raise NotImplementedError(RTDETR_TRAIN_MSG)
        return self._decode(x, query_index, True)

    def _decode(self, x, query_index, all_layers):
        memory, shapes, feats, logits, score_max = self._encode(x)
        b, nq, hd = memory.shape[0], self.num_queries, self.hidden_dim
        if query_index is None:
            index = ops.rtdetr_topk(score_max, nq)
        else:
            index = query_index
            if not torch.is_tensor(index) or index.dtype != torch.int64 or tuple(index.shape) != (b, nq) or index.device != memory.device:
                raise RuntimeError(f'RTDETRDecoder: query_index must be a ({b}, {nq}) int64 tensor on {memory.device}')
            index = index.contiguous()
        embed, enc_scores = ops.rtdetr_gather(feats, logits, index)
        ref = enc_bboxes = ops.rtdetr_ref_init(self._mlp('enc_bbox', embed, self.enc_bbox_head), index, shapes)
        layers = self.decoder.layers
        # every layer's value_proj reads the same memory: one GEMM with an ndl*256-column panel
        vt = [t for l in layers for t in (l.cross_attn.value_proj.weight, l.cross_attn.value_proj.bias)]
        values = self._linear('values', memory, len(layers) * hd, lambda: torch.cat([l.cross_attn.value_proj.weight for l in layers], 0),
                              lambda: torch.cat([l.cross_attn.value_proj.bias for l in layers], 0), tensors=vt)
        no = self.nhead * self.nl * 4 * 2
        scores = None
        all_boxes, all_scores = [], []
        from .conv import act_code
        for i, l in enumerate(layers):
            sa, ca = l.self_attn, l.cross_attn
            pos = self._mlp(('pos', i), ref, self.query_pos_head)
            wt = [sa.in_proj_weight, sa.in_proj_bias]
            qk = self._linear(('qk', i), embed, 2 * hd, lambda: sa.in_proj_weight[:2 * hd], lambda: sa.in_proj_bias[:2 * hd], x2=pos, tensors=wt)
            v = self._linear(('v', i), embed, hd, lambda: sa.in_proj_weight[2 * hd:], lambda: sa.in_proj_bias[2 * hd:], tensors=wt)
            t = self._lin(('sa_out', i), ops.mha(qk[..., :hd], qk[..., hd:], v), sa.out_proj)
            embed = ops.add_layernorm(t, embed, l.norm1.weight, l.norm1.bias, l.norm1.eps)
            # sampling offsets and attention weights: one panel
            ow = self._linear(('ow', i), embed, no + no // 2, lambda: torch.cat([ca.sampling_offsets.weight, ca.attention_weights.weight], 0),
                              lambda: torch.cat([ca.sampling_offsets.bias, ca.attention_weights.bias], 0), x2=pos,
                              tensors=[ca.sampling_offsets.weight, ca.attention_weights.weight, ca.sampling_offsets.bias, ca.attention_weights.bias])
            samp = ops.msdeform_attn(values[..., i * hd:(i + 1) * hd], shapes, ref, ow[..., :no], ow[..., no:])
            t = self._lin(('ca_out', i), samp, ca.output_proj)
            embed = ops.add_layernorm(t, embed, l.norm2.weight, l.norm2.bias, l.norm2.eps)
            t = self._lin(('ffn2', i), self._lin(('ffn1', i), embed, l.linear1, act_code(l.act)), l.linear2)
            embed = ops.add_layernorm(t, embed, l.norm3.weight, l.norm3.bias, l.norm3.eps)
            ref = ops.rtdetr_refine(self._mlp(('bbox', i), embed, self.dec_bbox_head[i]), ref)
            if all_layers:
                all_boxes.append(ref)
                all_scores.append(self._lin(('score', i), embed, self.dec_score_head[i]))
                continue
            if i == self.decoder.eval_idx:
                scores = ops.rtdetr_sigmoid(self._lin(('score', i), embed, self.dec_score_head[i]))
                break
        if all_layers:
            return torch.stack(all_boxes), torch.stack(all_scores), enc_bboxes, enc_scores, None
        if scores is None:
            raise RuntimeError(f'RTDETRDecoder: eval_idx {self.decoder.eval_idx} is outside the {len(layers)} decoder layers')
        return ref.unsqueeze(0), scores.unsqueeze(0), enc_bboxes, enc_scores, None
