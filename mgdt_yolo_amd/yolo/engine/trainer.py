"""Training-step counterpart of the reference's DetectionTrainer hot loop (yolo/engine/trainer.py:314-362,462-470).

Only what touches the device per step lives here; the data pipeline, callbacks, checkpoints and logging of the reference's
BaseTrainer are out of scope.  One step = warm-up interpolation of lr / momentum (trainer.py:317-326) ->
preprocess (uint8 batch handed to the stem as is: /255 is fused into the first conv's loader) -> train-mode forward (HIP) ->
fused assigner+loss (HIP) -> reverse pass (HIP; reachable from `loss.backward()` too) with the flat gradient buffer
all-reduced in layer-ordered buckets while the earlier layers are still running backward (RCCL over xGMI) -> every
`accumulate` batches: clip(10) + SGD(Nesterov, the reference's three parameter groups) + EMA on the flat parameter buffer.
`optimizer=` selects Adam / AdamW / RMSProp instead of SGD, or 'auto' (the reference's default, build_optimizer trainer.py:635-639).
"""
import collections
import math

import numpy as np
import torch
import torch.nn as nn

from ... import ops, parallel
from ..utils.loss import loss_and_head_grads, v8DetectionLoss


def param_groups(model):
    """The reference's build_optimizer rule (trainer.py:641-649), name -> group: 'bias' anywhere in the full name -> 2 (no decay, bias
    warm-up lr); a parameter of an nn.*Norm* module -> 1 (no decay); everything else -> 0 (decay).  Note what this implies: the custom
    utils.LayerNorm / GRN of the ConvNeXt blocks are plain nn.Modules, so LayerNorm.weight and GRN.gamma / GRN.beta are decayed."""
    bn = tuple(v for k, v in nn.__dict__.items() if 'Norm' in k and isinstance(v, type))
    out = {}
    for module_name, module in model.named_modules():
        for param_name, _ in module.named_parameters(recurse=False):
            fullname = f'{module_name}.{param_name}' if module_name else param_name
            out[fullname] = 2 if 'bias' in fullname else 1 if isinstance(module, bn) else 0
    return out


OPTIMIZERS = ('SGD', 'Adam', 'AdamW', 'RMSProp')
NOT_BUILT = ('Adamax', 'NAdam', 'RAdam')          # names the reference's build_optimizer accepts (trainer.py:651) that have no kernel here
ADAM_BETA2, OPT_EPS, RMS_ALPHA = 0.999, 1e-8, 0.99   # build_optimizer passes betas=(momentum, 0.999); eps / alpha are torch's defaults


def resolve_optimizer(name, nc, iterations, lr0, momentum, warmup_bias_lr):
    """build_optimizer's name handling (trainer.py:635-639,651-661) -> (name, lr0, optimizer momentum, warmup_bias_lr).  'auto': AdamW with
    lr0 = round(0.002 * 5 / (4 + nc), 6) up to 10 000 iterations, SGD with lr0 0.01 beyond; momentum 0.9 and warmup_bias_lr 0 in both."""
    if name == 'auto':
        if iterations is None:
            raise ValueError("optimizer='auto' needs `iterations` (ceil(len(dataset) / max(batch, nbs)) * epochs, trainer.py:252)")
        name, lr0, momentum = ('SGD', 0.01, 0.9) if iterations > 10000 else ('AdamW', round(0.002 * 5 / (4 + nc), 6), 0.9)
        warmup_bias_lr = 0.0
    if name in NOT_BUILT:
        raise NotImplementedError(f"Optimizer '{name}' is not built: there is no HIP kernel for it (built: {', '.join(OPTIMIZERS)}, auto).")
    if name not in OPTIMIZERS:
        raise NotImplementedError(f"Optimizer '{name}' not found in list of available optimizers [Adam, AdamW, NAdam, RAdam, RMSProp, SGD, auto].")
    return name, lr0, momentum, warmup_bias_lr


# One record per optimizer family: everything DetectionTrainer has to know about it.
#   second_moment   it needs state.second_moment (Adam's exp_avg_sq, RMSProp's square_avg)
#   warmed          its groups have a 'momentum' key, which the warm-up moves (trainer.py:325); Adam's beta1 never moves
#   has_step        its state entries carry 'step'; without one a loaded buffer is marked by _loaded_momentum instead
#   shared_step     the step count enters the update (bias corrections), so a loaded state must hold one count for all parameters
#   state_keys(mom), torch_cls, torch_kwargs(mom)    the state entries and the torch optimizer of optimizer_state_dict
#   hyper(tr, d)    the device vector of a captured step as Python floats, d the EMA decay
#   eager(tr, st, p, clip) / captured(tr, st, p, clip, hyper)    the step kernel on the flat buffers st = tr.state, p the parameters' part of
#                   st.data: with the scalars of `tr` (ops.ema_update follows), or with those and the EMA decay read from `hyper` at replay
Family = collections.namedtuple('Family', 'second_moment warmed has_step shared_step state_keys torch_cls torch_kwargs hyper eager captured')


def _adam(torch_cls, decoupled):            # every optimizer step is an EMA update, so Adam's 1-based step is st.steps + 1 (+ a loaded count)
    return Family(
        second_moment=True, warmed=False, has_step=True, shared_step=True, state_keys=lambda mom: ('exp_avg', 'exp_avg_sq'),
        torch_cls=torch_cls, torch_kwargs=lambda mom: dict(betas=(mom, ADAM_BETA2), weight_decay=0.0),
        hyper=lambda tr, d: ops.adam_hyper(tr.lr, tr.lr_bias, tr.mom, ADAM_BETA2, tr.state.steps + tr.opt_step_offset + 1, d),
        eager=lambda tr, st, p, clip: ops.adam_step(p, st.grad, st.momentum_buf, st.second_moment, st.wd, tr.lr, tr.mom, ADAM_BETA2, OPT_EPS,
                                                    st.steps + tr.opt_step_offset + 1, decoupled, clip, lr_bias=tr.lr_bias),
        captured=lambda tr, st, p, clip, hyper: ops.adam_ema_step_dev(p, st.grad, st.momentum_buf, st.second_moment, st.wd, st.ema, st.data, hyper,
                                                                      ADAM_BETA2, OPT_EPS, decoupled, clip))


FAMILIES = {
    # `first` (the buffer becomes g') on the first step unless a loaded buffer is continued; a captured step is never the first (_graph_ok)
    'SGD': Family(
        second_moment=False, warmed=True, has_step=False, shared_step=False, state_keys=lambda mom: ('momentum_buffer',),
        torch_cls=torch.optim.SGD, torch_kwargs=lambda mom: dict(momentum=mom, nesterov=True),
        hyper=lambda tr, d: ops.rmsprop_hyper(tr.lr, tr.lr_bias, tr.mom, d),        # SGD reads the first four
        eager=lambda tr, st, p, clip: ops.sgd_step(p, st.grad, st.momentum_buf, st.wd, tr.lr, tr.mom, True,
                                                   st.steps == 0 and not tr._loaded_momentum, clip, lr_bias=tr.lr_bias),
        captured=lambda tr, st, p, clip, hyper: ops.sgd_ema_step_dev(p, st.grad, st.momentum_buf, st.wd, st.ema, st.data, hyper, True, False, clip)),
    # torch tests momentum > 0 every step; the momentum / no-momentum kernel of a captured step is fixed at capture: see _graph_step
    'RMSProp': Family(
        second_moment=True, warmed=True, has_step=True, shared_step=False,
        state_keys=lambda mom: ('square_avg', 'momentum_buffer') if mom > 0 else ('square_avg',),
        torch_cls=torch.optim.RMSprop, torch_kwargs=lambda mom: dict(momentum=mom), hyper=lambda tr, d: ops.rmsprop_hyper(tr.lr, tr.lr_bias, tr.mom, d),
        eager=lambda tr, st, p, clip: ops.rmsprop_step(p, st.grad, st.second_moment, st.momentum_buf, st.wd, tr.lr, RMS_ALPHA, OPT_EPS, tr.mom,
                                                       clip, lr_bias=tr.lr_bias),
        captured=lambda tr, st, p, clip, hyper: ops.rmsprop_ema_step_dev(p, st.grad, st.second_moment, st.momentum_buf, st.wd, st.ema, st.data, hyper,
                                                                         RMS_ALPHA, OPT_EPS, tr.mom > 0, clip)),
    'Adam': _adam(torch.optim.Adam, False),
    'AdamW': _adam(torch.optim.AdamW, True),
}


class FlatState:
    """All trainable parameters (and float buffers) of a model as views into one flat fp32 buffer; grads likewise."""

    def __init__(self, model, weight_decay, second_moment=False):
        params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        bufs = [(n, b) for n, b in model.named_buffers() if b.dtype.is_floating_point and b.numel() > 0 and 'anchors' not in n and 'strides' not in n]
        dev = params[0][1].device
        self.n_param = sum(p.numel() for _, p in params)
        self.n_total = self.n_param + sum(b.numel() for _, b in bufs)
        self.data = torch.empty(self.n_total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.n_param, dtype=torch.float32, device=dev)
        # per-element weight decay; -1 marks the bias group (no decay, its own warm-up learning rate: mgdt_sgd_step)
        self.wd = torch.zeros(self.n_param, dtype=torch.float32, device=dev)
        groups = param_groups(model)
        self.offsets = {}                  # parameter name -> (offset, numel)
        self.layer_end = {}                # top-level layer index i -> end offset of its parameters in the flat buffers
        off = 0
        for n, p in params:
            k = p.numel()
            self.data[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.data[off:off + k].view(p.shape)
            p.grad = self.grad[off:off + k].view(p.shape)
            g = groups[n]
            self.wd[off:off + k] = weight_decay if g == 0 else (-1.0 if g == 2 else 0.0)
            self.offsets[n] = (off, k)
            parts = n.split('.')
            if len(parts) > 2 and parts[0] == 'model' and parts[1].isdigit():
                self.layer_end[int(parts[1])] = off + k
            off += k
        for n, b in bufs:
            k = b.numel()
            self.data[off:off + k].copy_(b.detach().reshape(-1))
            b.data = self.data[off:off + k].view(b.shape)
            off += k
        ops.LIVE_STORAGES.add(self.data.untyped_storage().data_ptr())       # packed panels built from these bytes may be refreshed in place (ops.repack_all)
        self.momentum_buf = torch.zeros(self.n_param, dtype=torch.float32, device=dev)       # SGD / RMSProp momentum buffer, Adam's exp_avg
        # Adam's exp_avg_sq / RMSProp's square_avg: only the optimizers that have one pay for it
        self.second_moment = torch.zeros(self.n_param, dtype=torch.float32, device=dev) if second_moment else None
        self.ema = self.data.clone()
        self.steps = 0                     # optimizer steps taken (= ModelEMA.updates)


class BucketedAllReduce:
    """Data-parallel gradient exchange overlapped with the reverse pass.  The flat gradient buffer is laid out in layer order and the
    reverse pass finishes layers last-to-first, so the buffer completes from its tail: as soon as the layers of a bucket are done, that
    contiguous slice is all-reduced asynchronously (RCCL runs it on its own stream behind the kernels already queued) while the earlier
    layers are still running backward.  Messages are a few MB (the whole n model is 5.26 MB), i.e. latency-bound on xGMI, so buckets are few."""

    def __init__(self, state, n_layers, n_buckets=3):
        ends = [state.layer_end.get(i) for i in range(n_layers)]
        last = 0
        for i in range(n_layers):          # layers without parameters inherit the previous end
            ends[i] = last = ends[i] if ends[i] is not None else last
        total = state.n_param
        # cut so that the buckets hold ~equal numbers of elements, at layer boundaries; bucket b covers layers [lo_b, hi_b)
        cuts, target = [], [total * (k + 1) / n_buckets for k in range(n_buckets - 1)]
        for t in target:
            i = min(range(n_layers), key=lambda j: abs(ends[j] - t))
            if ends[i] not in (0, total) and (i + 1) not in cuts:
                cuts.append(i + 1)
        self.bounds = [0] + sorted(cuts) + [n_layers]                     # layer indices
        self.slices = []
        for lo, hi in zip(self.bounds[:-1], self.bounds[1:]):
            a = ends[lo - 1] if lo > 0 else 0
            self.slices.append((lo, a, ends[hi - 1] if hi < n_layers else total))
        self.state, self.work = state, []

    def layer_done(self, i):
        """Called by BaseModel.backward after layer i's adjoint kernels are queued."""
        import torch.distributed as dist
        for lo, a, b in self.slices:
            if lo == i and b > a:
                ops.flush_wgrad()                      # the slice must hold finished weight gradients before it is sent
                self.work.append(dist.all_reduce(self.state.grad[a:b], op=dist.ReduceOp.SUM, async_op=True))

    def finish(self):
        import torch.distributed as dist
        for w in self.work:
            w.wait()
        self.work = []
        self.state.grad.div_(dist.get_world_size())


class DetectionTrainer:
    """Per-step driver: `trainer.step(batch)` -> (loss*B, loss_items[3]).  Hyper-parameters follow yolo/cfg/default.yaml of the fork
    (lr0 0.001, lrf 0.01, momentum 0.937, weight_decay 5e-4, warmup 3 epochs / momentum 0.8 / bias lr 0.1, nbs 64, nesterov SGD; grad
    clip 10.0; EMA decay 0.9999, tau 2000).  `batch_size` is the GLOBAL batch (trainer.py:238,250), `nb` the batches per epoch.

    `optimizer`: 'SGD' (default), 'Adam', 'AdamW', 'RMSProp' or 'auto' (resolve_optimizer; needs `iterations`).  After construction
    `optimizer` holds the resolved name, `lr0` its learning rate and `opt_momentum` the momentum the optimizer was built with (beta1 of Adam /
    AdamW, where it stays constant with beta2 = 0.999: their groups have no 'momentum' key for the warm-up to move, trainer.py:325).  SGD and
    RMSProp are warmed towards `momentum`, the constructor's argument, which is therefore what remains after the warm-up - also under
    'auto' -> SGD, whose own 0.9 is visible only when no warm-up runs (batch_size=None).  `cos_lr`: one_cycle(1, lrf, epochs) instead of the
    linear schedule (trainer.py:260-261)."""

    def __init__(self, model, lr0=0.001, lrf=0.01, momentum=0.937, weight_decay=5e-4, world_size=1, ema_decay=0.9999, ema_tau=2000.0,
                 batch_size=None, nb=None, epochs=100, nbs=64, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, overlap=True, amp=False,
                 graph=False, graph_split=None, optimizer='SGD', iterations=None, cos_lr=False):
        self.optimizer, lr0, self.opt_momentum, warmup_bias_lr = resolve_optimizer(optimizer, self._nc(model), iterations, lr0, momentum, warmup_bias_lr)
        self.family = FAMILIES[self.optimizer]
        self.iterations, self.cos_lr = iterations, bool(cos_lr)
        self.model = model.train()
        # amp: the reference trains under autocast (trainer.py:223,329: fp16 + GradScaler); on this hardware the reduced-precision training path
        # is bfloat16 activations / gradients with fp32 master weights, fp32 accumulation and fp32 weight gradients - no loss scaling needed
        model.set_compute_dtype(torch.bfloat16 if amp else torch.float32)
        self.amp = bool(amp)
        self.crit = v8DetectionLoss(model)
        self.world_size = world_size
        self.lr0, self.lrf, self.momentum, self.epochs = lr0, lrf, momentum, epochs
        self.warmup_momentum, self.warmup_bias_lr, self.nbs = warmup_momentum, warmup_bias_lr, nbs
        self.batch_size, self.nb = batch_size, nb
        if batch_size is None:                      # no schedule requested: constant lr0 / momentum, every batch is an optimizer step
            self.accumulate, self.nw, wd = 1, -1, weight_decay
        else:
            self.accumulate = max(round(nbs / batch_size), 1)                                    # trainer.py:250
            wd = weight_decay * batch_size * self.accumulate / nbs                               # trainer.py:251
            self.nw = max(round(warmup_epochs * nb), 100)                                        # trainer.py:284
        self.weight_decay = wd                      # of the decayed group, scaled as trainer.py:251 does
        self.state = FlatState(model, wd, second_moment=self.family.second_moment)
        model._flat_state = self.state
        self.ema_decay, self.ema_tau = ema_decay, ema_tau
        self.ni, self.last_opt_step, self.lr, self.lr_bias, self.mom = 0, -1, lr0, lr0, self.opt_momentum
        # Adam's `step` is st.steps + 1 (every optimizer step is an EMA update) unless a loaded optimizer state carried another count;
        # a loaded SGD momentum buffer is continued instead of being re-initialised by the first step
        self.opt_step_offset, self._loaded_momentum = 0, False
        # graph=True: from the second optimizer step on, the whole step (forward, loss, reverse pass, clip + SGD + EMA: ~500 launches) is one
        # hipGraph replay; lr / momentum / EMA decay / the assigner's call counter live in device memory so that the warm-up schedule and the
        # EMA ramp keep advancing between replays.  accumulate == 1 only (otherwise the eager path runs).  With several ranks (or
        # graph_split=True) the step is captured as TWO graphs - forward/loss/reverse pass, then clip/SGD/EMA/re-pack - with the one
        # flat-gradient all-reduce issued eagerly between the two replays (RCCL is not captured).
        self.graph = bool(graph)
        self.graph_split = parallel.world() > 1 if graph_split is None else bool(graph_split)
        self._graphs, self._pool, self._static = {}, None, None
        self.exchange = None
        if parallel.world() > 1:
            parallel.broadcast_(self.state.data)            # what DDP's constructor does (trainer.py:225): rank 0's parameters AND buffers
            self.state.ema.copy_(self.state.data)
            if overlap:
                self.exchange = BucketedAllReduce(self.state, len(model.model))

    @staticmethod
    def _nc(model):
        """build_optimizer reads getattr(model, 'nc', 10) (trainer.py:636); the reference's trainer has attached data['nc'] by then
        (v8/detect/train.py:72), which is the class count the head was built with."""
        nc = getattr(model, 'nc', None)
        if nc is None:
            nc = getattr(model.model[-1], 'nc', None) if hasattr(model, 'model') else None
        return 10 if nc is None else int(nc)

    def lf(self, epoch):
        """linear lr schedule (trainer.py:263), or with cos_lr one_cycle(1, lrf, epochs) (trainer.py:261, torch_utils.py:309-311)"""
        if self.cos_lr:
            return ((1 - math.cos(epoch * math.pi / self.epochs)) / 2) * (self.lrf - 1) + 1
        return (1 - epoch / self.epochs) * (1.0 - self.lrf) + self.lrf

    def warmup(self, epoch=0):
        """lr / momentum / accumulate of iteration self.ni (trainer.py:317-326); after warm-up the epoch's scheduled values."""
        base = self.lr0 * self.lf(epoch) if self.batch_size is not None else self.lr0
        self.lr = self.lr_bias = base
        # groups with a 'momentum' key (SGD, RMSProp) are left at the warm-up's target, the constructor's momentum; Adam's beta1 never moves
        warmed = self.family.warmed and self.nw >= 0
        self.mom = self.momentum if warmed else self.opt_momentum
        if self.ni <= self.nw:
            xi = [0, self.nw]
            self.accumulate = max(1, np.interp(self.ni, xi, [1, self.nbs / self.batch_size]).round())
            self.lr = float(np.interp(self.ni, xi, [0.0, base]))
            self.lr_bias = float(np.interp(self.ni, xi, [self.warmup_bias_lr, base]))
            if warmed:
                self.mom = float(np.interp(self.ni, xi, [self.warmup_momentum, self.momentum]))

    def preprocess_batch(self, batch):
        """detect/train.py:62-65 moves the uint8 batch to the device and computes float()/255; here the uint8 tensor goes to the stem
        kernel, which divides by 255 exactly while loading (no separate pass)."""
        img = batch['img'].to(self.state.data.device, non_blocking=True)
        return img if img.dtype == torch.uint8 else (img.to(torch.bfloat16) if self.amp else img.float())

    def optimizer_step(self, hyper=None):
        """unscale (no loss scaling: fp32 / bf16) -> clip_grad_norm_(10) -> the family's step -> zero_grad (implicit: overwrite) -> EMA
        (trainer.py:462-470) -> re-pack.  With `hyper`, inside a captured step: the scalars are those the device vector holds at replay, the EMA
        runs in the step's launch and the host side (st.steps) is _graph_step's.  Returns the refreshed panels."""
        st = self.state
        clip = ops.grad_clip_coef(st.grad, 10.0)
        p = st.data[:st.n_param]
        if hyper is None:
            self.family.eager(self, st, p, clip)
            st.steps += 1
            ops.ema_update(st.ema, st.data, self.ema_decay * (1 - math.exp(-st.steps / self.ema_tau)))      # torch_utils.py:342
        else:
            self.family.captured(self, st, p, clip, hyper)
        return ops.repack_all()                     # the packed panels of this step, refreshed for the next one in a few launches

    # ---- optimizer state in torch's layout -------------------------------------------------------------------------------------------
    def _reference_groups(self):
        """Parameter names in the reference's optimizer order: param_groups [0] biases, [1] decayed weights, [2] norm weights
        (build_optimizer trainer.py:652-664), each in named_modules order."""
        groups = param_groups(self.model)
        names = [[n for n, g in groups.items() if g == k] for k in (2, 0, 1)]
        return names                               # frozen parameters (dfl.conv.weight) are members too; they never get a state entry

    def optimizer_state_dict(self):
        """The optimizer state as torch's Optimizer.state_dict() of the reference's optimizer would hold it (what the reference saves in a
        checkpoint's 'optimizer' entry): per-parameter `step` / `exp_avg` / `exp_avg_sq` (Adam, AdamW), `momentum_buffer` (SGD) or `step` /
        `square_avg` [/ `momentum_buffer`] (RMSProp), indexed through the three groups.  Before the first step the state is empty, as torch's."""
        st, names = self.state, self._reference_groups()
        shapes = {n: p.shape for n, p in self.model.named_parameters()}
        # the hyper-parameter keys of the installed torch, from an optimizer over empty stand-ins
        fam = self.family
        opt = fam.torch_cls([{'params': [nn.Parameter(torch.empty(0)) for _ in ns], 'weight_decay': w, 'lr': lr, 'initial_lr': self.lr0}
                             for ns, w, lr in zip(names, (0.0, self.weight_decay, 0.0), (self.lr_bias, self.lr, self.lr))], lr=self.lr0, **fam.torch_kwargs(self.mom))
        groups = opt.state_dict()['param_groups']
        state, steps = {}, st.steps + self.opt_step_offset
        if steps > 0 or self._loaded_momentum:
            bufs = {'exp_avg': st.momentum_buf, 'momentum_buffer': st.momentum_buf, 'exp_avg_sq': st.second_moment, 'square_avg': st.second_moment}
            for i, n in enumerate(n for ns in names for n in ns):
                if n not in st.offsets:
                    continue
                off, k = st.offsets[n]
                e = {'step': torch.tensor(float(steps))} if fam.has_step else {}
                e.update({key: bufs[key][off:off + k].view(shapes[n]).clone() for key in fam.state_keys(self.mom)})
                state[i] = e
        return {'state': state, 'param_groups': groups}

    def load_optimizer_state_dict(self, sd):
        """Takes what optimizer_state_dict() returns - what the reference's resume_training hands to optimizer.load_state_dict
        (trainer.py:589-590).  The moment buffers and the step count are restored; learning rates and momentum stay the trainer's own
        schedule (the reference recomputes them from initial_lr every iteration / epoch as well).  A state of another optimizer type, other
        group sizes or other tensor shapes raises ValueError."""
        st, names = self.state, self._reference_groups()
        flat = [n for ns in names for n in ns]
        groups = sd['param_groups']
        if [len(g['params']) for g in groups] != [len(ns) for ns in names]:
            raise ValueError(f"optimizer state has groups of {[len(g['params']) for g in groups]} parameters, the model {[len(ns) for ns in names]}")
        idx = [i for g in groups for i in g['params']]
        state, keys = sd['state'], self.family.state_keys(self.mom)
        known = {'exp_avg', 'exp_avg_sq', 'square_avg', 'momentum_buffer', 'max_exp_avg_sq', 'grad_avg'}
        shapes = {n: p.shape for n, p in self.model.named_parameters()}
        bufs = {'exp_avg': st.momentum_buf, 'momentum_buffer': st.momentum_buf, 'exp_avg_sq': st.second_moment, 'square_avg': st.second_moment}
        steps = set()
        for i, n in zip(idx, flat):                # validate everything before anything is written
            e = state.get(i, state.get(str(i)))
            if n not in st.offsets:
                continue
            if e is None:
                if state:
                    raise ValueError(f'optimizer state has no entry for parameter {i} ({n})')
                continue
            have = {k for k in e if k in known and e[k] is not None}
            if have != set(keys):
                raise ValueError(f'optimizer state of parameter {i} ({n}) holds {sorted(have)}; {self.optimizer} needs {sorted(keys)}')
            for k in keys:
                if tuple(e[k].shape) != tuple(shapes[n]):
                    raise ValueError(f'{k} of parameter {i} ({n}) has shape {tuple(e[k].shape)}, the parameter {tuple(shapes[n])}')
            if 'step' in e:
                steps.add(int(e['step']))
        if self.family.shared_step and state and len(steps) != 1:
            raise ValueError(f'Adam state needs one step count for all parameters, got {sorted(steps)}')
        st.momentum_buf.zero_()
        if st.second_moment is not None:
            st.second_moment.zero_()
        for i, n in zip(idx, flat):
            e = state.get(i, state.get(str(i)))
            if e is not None and n in st.offsets:
                off, k = st.offsets[n]
                for key in keys:
                    bufs[key][off:off + k].copy_(e[key].reshape(-1))
        self._loaded_momentum = bool(state) and not self.family.has_step
        self.opt_step_offset = (max(steps) if steps else 0) - st.steps if self.family.has_step else 0

    # ---- captured step -------------------------------------------------------------------------------------------------------------
    def _graph_ok(self):
        return (self.graph and self.state.steps >= 1 and self.accumulate == 1
                and (self.batch_size is None or self.nbs / self.batch_size <= 1.0))

    def _graph_body(self, part=None):
        """part None: the whole step; 'grad': forward + loss + reverse pass; 'update': clip + SGD + EMA + re-pack."""
        S = self._static
        if part != 'update':
            feats = self.model._predict_once(S['img'])
            ls = ops.detect_loss_fwd(list(feats), self.crit.stride_list, self.crit.reg_max, self.crit.nc, S['gt'], 0,
                                     (self.crit.hyp.box, self.crit.hyp.cls, self.crit.hyp.dfl), call_count_dev=S['calls'])
            grads = ops.detect_loss_bwd(ls, float(self.world_size))
            self.model.backward(grads)
            S['out5'] = ls.out5
            if part == 'grad':
                return
        S['panels'] = self.optimizer_step(S['hyper'])      # next step's packed weights, all convolutions in a few launches

    def _graph_step(self, batch):
        st = self.state
        img = self.preprocess_batch(batch)
        b = img.shape[0]
        gt = self.crit.preprocess(batch, b, (img.shape[2], img.shape[3]))
        nmax = max(16, -(-int(gt.shape[1]) // 16) * 16)             # label slots of the captured step (zero rows are padding, loss.py:177-181)
        S = self._static
        if S is None or S['img'].shape != img.shape or S['img'].dtype != img.dtype:
            S = self._static = dict(img=torch.empty_like(img), hyper=torch.empty(ops.OPT_HYPER_LEN, dtype=torch.float32, device=img.device),
                                    calls=torch.zeros(1, dtype=torch.int32, device=img.device), gts={})
            self._graphs, self._pool = {}, None
        # Every captured graph reads - and, in its trailing re-pack, rewrites - the packed weight panels that were current when it was
        # captured.  They must stay the ONE live panel set: each graph holds strong references to them (the caches only hold the newest
        # object), every replay stamps them with the new optimizer epoch (so the next capture / eager step reuses them instead of packing
        # new ones and freeing these), and if anything else moved the weights without refreshing them the graphs are dropped.
        if any(not ops.pack_is_current(o) for _, _, panels in self._graphs.values() for o in panels):
            self._graphs, self._pool = {}, None
        keys = self.family.state_keys(self.mom)     # the buffers the captured kernel touches: RMSProp's change when momentum > 0 flips
        if S.setdefault('state_keys', keys) != keys:
            self._graphs, self._pool, S['state_keys'] = {}, None, keys
        if nmax not in S['gts']:
            S['gts'][nmax] = torch.zeros(b, nmax, 5, dtype=torch.float32, device=img.device)
        S['gt'] = S['gts'][nmax]
        S['img'].copy_(img, non_blocking=True)
        S['gt'].zero_()
        if gt.shape[1]:
            S['gt'][:, :gt.shape[1]].copy_(gt)
        d = self.ema_decay * (1 - math.exp(-(st.steps + 1) / self.ema_tau))      # torch_utils.py:342 with updates = steps + 1
        hyper = self.family.hyper(self, d)
        S['hyper'].copy_(torch.tensor(hyper, dtype=torch.float32), non_blocking=True)
        S['calls'].fill_(int(self.crit.epoch))
        captured = nmax not in self._graphs
        if captured:
            gs = []
            torch.cuda.synchronize()
            # an eval forward since the last step has cached derived copies of the weights under this epoch: the capture must not read them
            ops.fresh_epoch_for_capture()
            epoch0 = ops.PARAM_EPOCH[0]
            for part in (('grad', 'update') if self.graph_split else (None,)):
                g = torch.cuda.CUDAGraph()
                # several ranks: the RCCL watchdog thread polls events while we capture, so only this thread's calls are checked
                with torch.cuda.graph(g, pool=self._pool, capture_error_mode='thread_local' if parallel.world() > 1 else 'global'):
                    self._graph_body(part)
                if self._pool is None:
                    self._pool = g.pool()
                gs.append(g)
            assert ops.PARAM_EPOCH[0] == epoch0 + 1        # the capture walked through exactly one optimizer step on the host side
            ops.PARAM_EPOCH[0] = epoch0                     # ... which has not run yet: the replay below is that step
            for o in S['panels']:
                o.epoch = epoch0
            # A panel that became live since the earlier captures (an eval() forward of this model packs its own, BatchNorm folded) is in this
            # graph's re-pack only: a replay of an older graph would leave it behind.  Those graphs go, and are captured again over this set
            # when their label-slot bucket comes back.
            ids = {id(o) for o in S['panels']}
            self._graphs = {k: v for k, v in self._graphs.items() if {id(o) for o in v[2]} == ids}
            self._graphs[nmax] = (gs, S['out5'], list(S['panels']))
        gs, out5, panels = self._graphs[nmax]
        gs[0].replay()
        if self.graph_split:
            parallel.all_reduce_mean_(st.grad)       # one flat message between the two replays (loss was scaled by world_size: trainer.py:337-338)
            gs[1].replay()
        ops.PARAM_EPOCH[0] += 1                     # the replay moved the weights: packed-weight caches of any eager forward are stale ...
        for o in panels:                            # ... except the panels the replayed re-pack just refreshed in place - those and no others
            o.epoch = ops.PARAM_EPOCH[0]
        st.steps += 1
        self.crit.epoch += 1
        self.last_opt_step = self.ni
        self.ni += 1
        return out5[0].clone(), out5[1:4].clone()

    def step(self, batch, epoch=0):
        ops.refuse_inference_mode('DetectionTrainer.step')
        st = self.state
        self.warmup(epoch)
        if self._graph_ok():
            return self._graph_step(batch)
        first_micro = self.ni == self.last_opt_step + 1            # first backward after an optimizer step (zero_grad)
        feats = self.model._predict_once(self.preprocess_batch(batch))
        # loss * world_size so that the mean all-reduce yields the global sum (trainer.py:337-338)
        total, items, head_grads = loss_and_head_grads(self.crit, feats, batch, gscale=float(self.world_size))
        keep = None if first_micro else st.grad.clone()              # gradient accumulation: the adjoint kernels overwrite
        will_step = self.ni - self.last_opt_step >= self.accumulate
        ex = self.exchange if (will_step and keep is None) else None
        self.model.backward(head_grads, layer_done=ex.layer_done if ex is not None else None)
        if keep is not None:
            st.grad.add_(keep)
        if will_step:
            if ex is not None:
                ex.finish()
            else:
                parallel.all_reduce_mean_(st.grad)                     # one flat message (accumulated micro-batches / no overlap)
            self.optimizer_step()
            self.last_opt_step = self.ni
        self.ni += 1
        return total, items
