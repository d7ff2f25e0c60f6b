"""A/B of the kernels that interpolate through csrc/resample.h - mgdt_bilinear_fwd and mgdt_inject_fwd - between two builds of the library: raw
outputs on odd sizes and ratios, bf16 with 8 and 4 channels per lane and fp32, compared bit for bit.

  MGDT_LIB=/path/to/libmgdt_hip.so python tools/resample_ab.py dump DIR      # one process per library
  python tools/resample_ab.py compare DIR_A DIR_B                            # numpy.array_equal per case, exit status 1 on a difference
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

# (n, c, h, w, hs, ws): a map of hs x ws resampled to h x w
CASES = [(2, 64, 37, 53, 13, 19), (2, 64, 9, 11, 4, 5), (1, 64, 9, 11, 12, 7), (2, 64, 13, 9, 6, 4), (3, 64, 24, 40, 12, 20), (2, 12, 21, 17, 8, 5),
         (1, 256, 40, 40, 20, 20), (1, 128, 23, 31, 10, 14)]


def dump(out_dir):
    import torch
    from kernel_ref import _gen
    from mgdt_yolo_amd import _lib, ops
    os.makedirs(out_dir, exist_ok=True)
    print('library', _lib.LIB_PATH)
    for case in CASES:
        n, c, h, w, hs, ws = case
        for dt in (torch.bfloat16, torch.float32):
            g = _gen('resample ab', case)
            mk = lambda *s: torch.randn(*s, generator=g).to(dt).to('cuda:0').contiguous(memory_format=torch.channels_last)
            src, gate, loc = mk(n, c, hs, ws), mk(n, c, hs, ws), mk(n, c, h, w)
            up = ops.bilinear(src, ops.new_act(n, c, h, w, dt, src.device))
            outs = {'bilinear': up}
            if h >= hs and w >= ws:
                outs['inject'] = ops.inject(loc, gate, src)
            torch.cuda.synchronize()
            for k, t in outs.items():
                a = t.view(torch.int16 if dt == torch.bfloat16 else torch.int32).cpu().numpy()
                np.save(os.path.join(out_dir, '%s-%s-%s.npy' % (k, 'x'.join(map(str, case)), str(dt).split('.')[1])), a)


def compare(da, db):
    names = sorted(os.listdir(da))
    bad = [f for f in names if not np.array_equal(np.load(os.path.join(da, f)), np.load(os.path.join(db, f)))]
    print('%d arrays, %d differ' % (len(names), len(bad)), *bad)
    return 1 if bad or names != sorted(os.listdir(db)) or not names else 0


if __name__ == '__main__':
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == 'dump' else compare(sys.argv[2], sys.argv[3]))
