"""Training-mode restatements of the YOLOv8 / MSPA-C2f-GD blocks and the Detect head from plain torch functional ops, for float64 autograd.

Every function takes the block's state dict (the module's own key names; tensors that require grad where a gradient is wanted), its inputs and
  rnd   where the device code stores a tensor in the compute dtype: the input, the packed weight, the raw convolution output, the BN + activation output
        after its residuals are added, concat slots and resampled maps.  Identity by default (the exact float64 function); `round_bf16` for bf16.
  omit  detaches ONE named path so that its gradient is missing (reference side only: the sensitivity check of tests/test_train_modules.py).
  mom, eps  BatchNorm momentum / eps of the module.
and returns (output, running) with running = {BatchNorm prefix: (running_mean, running_var)} after the step: batch statistics of the stored raw map,
biased mean, unbiased variance, running <- (1 - mom) * running + mom * batch (what nn.BatchNorm2d does in training mode).

`round_bf16` rounds to bfloat16 in the forward AND rounds the incoming gradient in the backward: activation gradients (gz, dy, dx) are stored in
the compute dtype too.  Parameters are rounded forward-only (`_Ref.w`): their gradients are fp32 on the device and stay unrounded here.
The max-pool adjoint is ATen's CPU one: the gradient goes to the FIRST maximum of each window in (ky, kx) scan order, the rule
tests/test_reverse_kernels.py pins ops.maxpool5_bwd to (bf16 rounding makes ties common).
"""
import torch
import torch.nn.functional as F

OMIT_PATHS = ('shortcut', 'pending', 'preadd', 'attention', 'gate', 'residual', 'cls')


def identity(t):
    return t


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def round_bf16(t):
    return _RoundBf16.apply(t)


def _key(p, name):
    return f'{p}.{name}' if p else name


class _Ref:
    """the arguments every restatement shares + the running statistics it collects"""

    def __init__(self, sd, rnd, omit, mom, eps):
        if omit is not None and omit not in OMIT_PATHS:
            raise KeyError(omit)
        self.sd, self.rnd, self.omit, self.mom, self.eps, self.running = sd, rnd, omit, mom, eps, {}

    def w(self, key):
        """a parameter as the packed panel holds it: rounded in the forward, gradient untouched (exactly the rounded value: the difference of a
        float32 and its bfloat16 rounding is exact in float64)"""
        t = self.sd[key]
        return t if self.rnd is identity else t + (self.rnd(t.detach()) - t.detach())

    def cba(self, p, x, s=1, act='silu', x2=None, r1=None, r2=None):
        """Conv.train_fwd: act(bn_batchstats(conv(x [+ x2]))) [+ r1] [+ r2]"""
        rnd = self.rnd
        w = self.w(_key(p, 'conv.weight'))
        y = rnd(F.conv2d(x if x2 is None else rnd(x + x2), w, None, s, w.shape[-1] // 2))
        bn = _key(p, 'bn')
        with torch.no_grad():
            mu, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=True)
            self.running[bn] = ((1 - self.mom) * self.sd[bn + '.running_mean'] + self.mom * mu, (1 - self.mom) * self.sd[bn + '.running_var'] + self.mom * var)
        z = F.batch_norm(y, None, None, self.sd[bn + '.weight'], self.sd[bn + '.bias'], True, 0.0, self.eps)
        z = {'silu': F.silu, 'relu': torch.relu, 'none': identity}[act](z)
        for r in (r1, r2):
            if r is not None:
                z = z + r
        return rnd(z)

    def bottleneck(self, p, x, shortcut, x2=None):
        """Bottleneck.run: [x (+ x2)] + cv2(cv1(x (+ x2)))"""
        t = self.cba(_key(p, 'cv1'), x, x2=x2)
        if not shortcut:
            return self.cba(_key(p, 'cv2'), t)
        keep = (lambda r: r.detach()) if self.omit == 'shortcut' else identity
        return self.cba(_key(p, 'cv2'), t, r1=keep(x), r2=None if x2 is None else keep(x2))

    def convnext(self, p, x):
        """ConvNeXtV2_Block._train_fwd: dw7x7 + LayerNorm, pwconv1 (raw, then bias + GELU), GRN as a per-(image, channel) affine, pwconv2 + residual"""
        rnd, sd, c = self.rnd, self.sd, x.shape[1]
        u = rnd(F.conv2d(x, sd[_key(p, 'dwconv.weight')], sd[_key(p, 'dwconv.bias')], 1, 3, 1, c))
        t1 = rnd(F.layer_norm(u.permute(0, 2, 3, 1), (c,), sd[_key(p, 'norm.weight')], sd[_key(p, 'norm.bias')], 1e-6))
        y1 = rnd(F.linear(t1, self.w(_key(p, 'pwconv1.weight'))))
        t2 = rnd(F.gelu(y1 + sd[_key(p, 'pwconv1.bias')]))
        gx = torch.norm(t2, p=2, dim=(1, 2), keepdim=True)
        nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
        t3 = rnd(sd[_key(p, 'grn.gamma')] * (t2 * nx) + sd[_key(p, 'grn.beta')] + t2)
        t = F.linear(t3, self.w(_key(p, 'pwconv2.weight')), sd[_key(p, 'pwconv2.bias')]).permute(0, 3, 1, 2)
        return rnd((x.detach() if self.omit == 'residual' else x) + t)


def _spr(x, sd, p):
    """SPRModule on one channel group: fp32 parameters and fp32 arithmetic on the device (no rounding point)"""
    b = x.shape[0]
    o = torch.cat((F.adaptive_avg_pool2d(x, 1).reshape(b, -1, 1, 1), F.adaptive_avg_pool2d(x, 2).reshape(b, -1, 1, 1)), 1)
    o = torch.relu(F.conv2d(o, sd[p + '.fc1.weight'], sd[p + '.fc1.bias']))
    return torch.sigmoid(F.conv2d(o, sd[p + '.fc2.weight'], sd[p + '.fc2.bias']))


# ------------------------------------------------------------------------------------------------ the blocks
def conv(sd, x, s=1, act='silu', x2=None, r1=None, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    """Conv.train_fwd(x, x2=, r1=): the pre-add rides in the convolution's input, the residual is added after the activation"""
    c = _Ref(sd, rnd, omit, mom, eps)
    return c.cba('', rnd(x), s, act, x2=None if x2 is None else rnd(x2), r1=None if r1 is None else rnd(r1)), c.running


def bottleneck(sd, x, shortcut, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    c = _Ref(sd, rnd, omit, mom, eps)
    return c.bottleneck('', rnd(x), shortcut), c.running


def c2f(sd, x, n, shortcut, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    c = _Ref(sd, rnd, omit, mom, eps)
    y = list(c.cba('cv1', rnd(x)).chunk(2, 1))
    for j in range(n):
        y.append(c.bottleneck(f'm.{j}', y[-1], shortcut))
    return c.cba('cv2', torch.cat(y, 1)), c.running


def mspa_c2f(sd, x, n, shortcut, rnd=identity, omit=None, mom=0.03, eps=1e-3, scale=4):
    """MSPA_C2f.forward (stride 1): the front chain with its pre-adds, the bottleneck chain (the first one takes the pending addend), the closing conv,
    then the SPR attention: softmax over the groups, applied to the stored closing map"""
    c = _Ref(sd, rnd, omit, mom, eps)
    b, wd = x.shape[0], x.shape[1] // scale
    spx = rnd(x).chunk(scale, 1)
    sp = c.cba('convs.0', spx[0])
    outs = [sp]
    for i in range(1, scale - 1):
        sp = c.cba(f'convs.{i}', sp, x2=spx[i].detach() if omit == 'preadd' else spx[i])
        outs.append(sp)
    pending = spx[scale - 1].detach() if omit == 'pending' else spx[scale - 1]
    for j in range(n):
        sp = c.bottleneck(f'bottleneck.{j}', sp, shortcut, x2=pending if j == 0 else None)
        outs.append(sp)
    out = c.cba(f'convs.{scale - 1}', torch.cat(outs, 1))
    ow = out.shape[1] // scale
    attn = torch.cat([_spr(t, sd, 'attention') for t in out.chunk(scale, 1)], 1)
    attn = torch.softmax(attn.view(b, scale, ow, 1, 1), 1)
    if omit == 'attention':
        attn = attn.detach()
    return rnd((out.view(b, scale, ow, *out.shape[2:]) * attn).reshape(out.shape)), c.running


def sppf(sd, x, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    c = _Ref(sd, rnd, omit, mom, eps)
    x0 = c.cba('cv1', rnd(x))
    y1 = rnd(F.max_pool2d(x0, 5, 1, 2))
    y2 = rnd(F.max_pool2d(y1, 5, 1, 2))
    y3 = rnd(F.max_pool2d(y2, 5, 1, 2))
    return c.cba('cv2', torch.cat((x0, y1, y2, y3), 1)), c.running


def _bilinear(x, hw):
    return F.interpolate(x, size=hw, mode='bilinear', align_corners=False)


def simfusion_4in(sd, xs, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    x_l, x_m, x_s, x_n = (rnd(t) for t in xs)
    hw = tuple(x_s.shape[2:])
    return torch.cat([rnd(F.adaptive_avg_pool2d(x_l, hw)), rnd(F.adaptive_avg_pool2d(x_m, hw)), x_s, rnd(_bilinear(x_n, hw))], 1), {}


def simfusion_3in(sd, xs, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    c = _Ref(sd, rnd, omit, mom, eps)
    xs = [rnd(t) for t in xs]
    hw = tuple(xs[1].shape[2:])
    t = [rnd(F.adaptive_avg_pool2d(xs[0], hw)), xs[1], rnd(_bilinear(xs[2], hw))]
    for i in range(3):
        if f'cv{i + 1}.conv.weight' in sd:
            t[i] = c.cba(f'cv{i + 1}', t[i], act='relu')
    return c.cba('cv_fuse', torch.cat(t, 1), act='relu'), c.running


def convnext_block(sd, x, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    c = _Ref(sd, rnd, omit, mom, eps)
    return c.convnext('', rnd(x)), c.running


def ifm(sd, x, nblocks=3, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    c = _Ref(sd, rnd, omit, mom, eps)
    t = c.cba('conv.0', rnd(x))
    for i in range(nblocks):
        t = c.convnext(f'conv.{i + 1}', t)
    return c.cba(f'conv.{nblocks + 1}', t), c.running


def inject(sd, xs, global_inp, flag, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    """InjectionMultiSum_Auto_pool: local * resample(gate) + resample(embedding); the up-sampling branch gates with h_sigmoid, the pooling one does not"""
    c = _Ref(sd, rnd, omit, mom, eps)
    x_l, x_g = rnd(xs[0]), rnd(xs[1])
    hw = tuple(x_l.shape[2:])
    c0 = sum(global_inp[:flag])
    g = x_g[:, c0:c0 + global_inp[flag]]
    local = c.cba('local_embedding', x_l, act='none')
    ga = c.cba('global_act', g, act='none')
    gf = c.cba('global_embedding', g, act='none')
    if x_l.shape[2] < x_g.shape[2]:
        sig, gf = rnd(F.adaptive_avg_pool2d(ga, hw)), rnd(F.adaptive_avg_pool2d(gf, hw))
    else:
        sig, gf = rnd(_bilinear(rnd(F.relu6(ga + 3) / 6), hw)), rnd(_bilinear(gf, hw))
    if omit == 'gate':
        sig = sig.detach()
    return rnd(local * sig + gf), c.running


def detect(sd, xs, rnd=identity, omit=None, mom=0.03, eps=1e-3):
    """Detect in training mode: the raw (B, 4 * reg_max + nc, H, W) map of every level"""
    c = _Ref(sd, rnd, omit, mom, eps)
    out = []
    for i, x in enumerate(xs):
        x = rnd(x)
        t = c.cba(f'cv2.{i}.1', c.cba(f'cv2.{i}.0', x))
        box = rnd(F.conv2d(t, c.w(f'cv2.{i}.2.weight'), sd[f'cv2.{i}.2.bias']))
        t = c.cba(f'cv3.{i}.1', c.cba(f'cv3.{i}.0', x.detach() if omit == 'cls' else x))
        cls = rnd(F.conv2d(t, c.w(f'cv3.{i}.2.weight'), sd[f'cv3.{i}.2.bias']))
        out.append(torch.cat((box, cls), 1))
    return out, c.running
