"""A/B of mgdt_conv1x1_inject_conv_fwd / mgdt_conv1x1_inject_fwd between two builds of the library: raw kernel outputs on the shapes of
tests/test_inject_rework.py, compared bit for bit.

  MGDT_LIB=/path/to/libmgdt_hip.so python tools/inject_ab.py dump DIR      # one process per library
  python tools/inject_ab.py compare DIR_A DIR_B                            # numpy.array_equal per case, exit status 1 on a difference
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def dump(out_dir):
    import torch
    from kernel_ref import BF16, _nhwc
    from mgdt_yolo_amd import _lib, ops
    from test_block_kernels import _inj_inputs
    from test_inject_rework import CASES, WRAP
    os.makedirs(out_dir, exist_ok=True)
    print('library', _lib.LIB_PATH)
    for cid, cin, cout2, B, H, W, Hg, Wg, _, gconv in CASES:
        x, pk, gaf, gsrc, pkg, pk2, _ = _inj_inputs(cid, cin, 256, B, H, W, Hg, Wg, False, gconv, cout2)
        xv, gd = _nhwc(x, BF16)[0], _nhwc(gaf, BF16)[0]
        out = ops.new_act(B, cout2, H, W, BF16, xv.device)
        p2 = pk2.pack(ops.acc_order_index(256, 'cpu'))
        if gconv:
            ops.conv1x1_inject_conv(xv, pk.pack(), None, None, p2, ops.ACT_SILU, out, gsrc=_nhwc(gsrc, BF16)[0], pkg=pkg.pack())
        else:
            ops.conv1x1_inject_conv(xv, pk.pack(), gd[:, :256], gd[:, 256:], p2, ops.ACT_SILU, out)
        np.save(os.path.join(out_dir, f'{cid}-{"gconv" if gconv else "maps"}.npy'), out.view(torch.int16).cpu().numpy())
    cid, cin, _, B, H, W, Hg, Wg, _ = WRAP
    x, pk, gaf, _, _, _, _ = _inj_inputs(cid + '-plain', cin, 128, B, H, W, Hg, Wg, False)
    xv, gd = _nhwc(x, BF16)[0], _nhwc(gaf, BF16)[0]
    out = ops.new_act(B, 128, H, W, BF16, xv.device)
    ops.conv1x1_inject(xv, pk.pack(), gd[:, :128], gd[:, 128:], out=out)
    np.save(os.path.join(out_dir, f'{cid}-plain.npy'), out.view(torch.int16).cpu().numpy())
    torch.cuda.synchronize()


def compare(a, b):
    names = sorted(os.listdir(a))
    assert names and names == sorted(os.listdir(b)), 'the two directories hold different cases'
    bad = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        same = np.array_equal(x, y)
        bad += not same
        print(f'{n}: {x.shape} {"equal" if same else f"DIFFERENT in {(x != y).sum()} of {x.size} elements"}')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'dump':
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
