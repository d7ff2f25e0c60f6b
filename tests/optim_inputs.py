"""Seeded inputs shared by tests/golden/gen_optim.py (which runs the reference on them) and tests/test_optimizers.py (which regenerates
them): the cases of the `auto` rule, the hyper-parameters and gradients of the recorded optimizer trajectories, the sampling of a list
of tensors.  A plain module, not a conftest."""
import zlib

import torch

AUTO_CASES = [(nc, it) for nc in (1, 2, 80) for it in (100, 10000, 10001)]
ONE_CYCLE_EPOCHS = (0, 1, 50, 99)
SAMPLE = 64                       # leading elements recorded per tensor
# yolo/cfg/default.yaml of the fork, with batch = nbs (accumulate 1) and nw = 100 (trainer.py:281: max(round(3 * nb), 100) for nb <= 33)
TRAJ_ARGS = dict(nc=4, lr0=0.001, lrf=0.01, momentum=0.937, weight_decay=5e-4, warmup_momentum=0.8, warmup_bias_lr=0.1, nbs=64, batch=64,
                 nb=10, nw=100, epochs=100)
# tag -> (build_optimizer name, iterations, iterations run, snapshots after these iterations)
TRAJ = {'auto': ('auto', 5000, 5, (1, 5)), 'rmsprop': ('RMSProp', 5000, 3, (3,)), 'adam': ('Adam', 5000, 3, (3,))}
GRAD_SCALE = (0.02, 0.005, 0.03, 0.004, 0.02)     # flat gradient norm ~ 1146 * scale: clipped (norm > 10) and not clipped, in turn


def traj_grad(tag, it, n_param):
    """The flat fp32 gradient of iteration `it` (0-based), in named_parameters order of the trainable parameters."""
    gen = torch.Generator().manual_seed(zlib.crc32(repr(('optim-traj', tag, it)).encode()))
    return torch.randn(n_param, generator=gen) * GRAD_SCALE[it]


def sample_flat(tensors):
    """The first SAMPLE elements of every tensor, concatenated (fp32)."""
    return torch.cat([t.detach().reshape(-1)[:SAMPLE].float().cpu() for t in tensors])
