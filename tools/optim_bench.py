"""Times of the captured-step optimizer kernels on the flat buffers of the n and the s model (mspa_c2f_gd_yolov8, nc 80: every trainable
parameter plus the float buffers the EMA covers): mgdt_adam_ema_step_dev (AdamW), mgdt_rmsprop_ema_step_dev (momentum) and, as the yardstick in the
same process, mgdt_sgd_ema_step_dev.

    python tools/optim_bench.py [--rounds 7] [--steps 30] [--reps 20] [--warmup 5] [--train-step]

The three kernels alternate measurement by measurement on buffers of their own (so no kernel inherits another's cache contents); one measurement
is `reps` back-to-back launches between two HIP events, divided by `reps` (a single launch of ~10 us is below what an event pair resolves); a round's
figure is the median of `steps` measurements; the spread of a kernel is (max - min) / median over the rounds' medians.  Bytes per launch: SGD 8
words per parameter (p, buf, ema read and written; g, wd read), Adam / RMSProp 10 (one more state array read and written), 3 per buffer element
(p read, ema read and written).  --train-step adds the whole captured training step (B = 32, 640 x 640, bf16) with optimizer='SGD' and 'AdamW'.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.models import get_config  # noqa: E402
from mgdt_yolo_amd.nn.tasks import DetectionModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images, seeded_labels  # noqa: E402

DEV = 'cuda:0'
med = statistics.median


def flat_sizes(scale):
    m = DetectionModel(get_config('mspa_c2f_gd_yolov8', scale, 80), verbose=False)
    n_param = sum(p.numel() for p in m.parameters() if p.requires_grad)
    n_buf = sum(b.numel() for n, b in m.named_buffers() if b.dtype.is_floating_point and b.numel() > 0 and 'anchors' not in n and 'strides' not in n)
    return n_param, n_param + n_buf


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(n_param, n_total):
    def bufs(k):
        g = torch.Generator().manual_seed(k)
        mk = lambda n, s=1.0: (torch.randn(n, generator=g) * s).to(DEV)
        return dict(data=mk(n_total), g=mk(n_param, 0.01), m=torch.zeros(n_param, device=DEV), v=torch.zeros(n_param, device=DEV), ema=mk(n_total),
                    wd=torch.tensor([5e-4, 0.0, -1.0]).repeat(n_param // 3 + 1)[:n_param].to(DEV), clip=torch.tensor([1.0, 1.0], device=DEV))
    S, A, R = bufs(1), bufs(2), bufs(3)
    hs = torch.tensor(ops.rmsprop_hyper(1e-3, 1e-3, 0.937, 0.9999), device=DEV)
    ha = torch.tensor(ops.adam_hyper(1e-3, 1e-3, 0.9, 0.999, 100, 0.9999), device=DEV)
    return {
        'sgd': (lambda: ops.sgd_ema_step_dev(S['data'][:n_param], S['g'], S['m'], S['wd'], S['ema'], S['data'], hs, True, False, S['clip']), 8),
        'adamw': (lambda: ops.adam_ema_step_dev(A['data'][:n_param], A['g'], A['m'], A['v'], A['wd'], A['ema'], A['data'], ha, 0.999, 1e-8, True, A['clip']), 10),
        'rmsprop': (lambda: ops.rmsprop_ema_step_dev(R['data'][:n_param], R['g'], R['v'], R['m'], R['wd'], R['ema'], R['data'], hs, 0.99, 1e-8, True, R['clip']), 10),
    }


def train_step_ms(optimizer, steps, warmup):
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    B, S, nc = 32, 640, 80
    m = seed_state_dict_(DetectionModel(get_config('mspa_c2f_gd_yolov8', 'n', nc), verbose=False), 0).to(DEV)
    tr = DetectionTrainer(m, amp=True, graph=True, optimizer=optimizer)
    batch = dict(img=(seeded_images(B, S, S, seed=2) * 255).to(torch.uint8).to(DEV), **seeded_labels(B, nc, seed=6, max_boxes=8, min_boxes=2))
    for _ in range(warmup + 2):                     # the first step is eager, the second captures
        tr.step(batch)
    torch.cuda.synchronize()
    return med([timed(lambda: tr.step(batch), 1) for _ in range(steps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--train-step', action='store_true')
    a = ap.parse_args()
    out = {'rounds': a.rounds, 'steps': a.steps, 'reps': a.reps}
    for scale in ('n', 's'):
        n_param, n_total = flat_sizes(scale)
        ks = kernels(n_param, n_total)
        for fn, _ in ks.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in ks}
        for _ in range(a.rounds):
            ts = {k: [] for k in ks}
            for _ in range(a.steps):
                for k, (fn, _) in ks.items():
                    ts[k].append(timed(fn, a.reps))
            for k in ks:
                rounds[k].append(med(ts[k]))
        row = {'n_param': n_param, 'n_total': n_total}
        for k, (_, words) in ks.items():
            t = med(rounds[k])
            nbytes = 4 * (words * n_param + 3 * (n_total - n_param))
            row[k] = {'us': round(t * 1e3, 3), 'MB': round(nbytes / 1e6, 2), 'TB_per_s': round(nbytes / (t * 1e-3) / 1e12, 3),
                      'spread': round((max(rounds[k]) - min(rounds[k])) / t, 4)}
        out[scale] = row
    if a.train_step:
        out['train_step_B32_640_bf16_ms'] = {o: round(train_step_ms(o, a.steps, a.warmup), 3) for o in ('SGD', 'AdamW')}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
