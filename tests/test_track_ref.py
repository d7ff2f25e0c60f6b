"""CPU: tests/track_ref.py (the numpy model of the device tracker) against the fixtures recorded from the reference's own BYTETracker
(tests/golden/gen_track.py), and its solver against the stored extended-matrix solutions and scipy.
The rules of the comparison: tests/track_checks.py."""
import os

import numpy as np
import pytest

import track_ref as TR
from track_checks import GOLD, SEQS, cfg_of, check_rows, check_state, ext_total


def test_fixtures_exist():
    assert len(SEQS) >= 2 and os.path.exists(os.path.join(GOLD, 'track_solver.npz'))
    assert any(cfg_of(np.load(p))['track_buffer'] == 5 for p in SEQS)


@pytest.mark.parametrize('path', SEQS, ids=[os.path.basename(p)[:-4] for p in SEQS])
def test_track_ref_reproduces_the_reference(path):
    z = np.load(path)
    cfg = cfg_of(z)
    rows, counts = z['rows'], z['counts']
    nb, nf = counts.shape
    trk = TR.Tracker(streams=nb, cap=128, **cfg)
    for f in range(nf):
        for b in range(nb):
            out, flag = trk.update(b, rows[b, f, :counts[b, f]])
            assert flag == 0
            check_rows(out, z['out'][b, f, :z['nout'][b, f]], f'stream {b} frame {f + 1}')
            if (f + 1) % 10 == 0:
                check_state(trk.s[b].export(), z, b, (f + 1) // 10 - 1, f'stream {b} frame {f + 1}')


def test_solver_equals_the_stored_solutions():
    z = np.load(os.path.join(GOLD, 'track_solver.npz'))
    thresh = float(z['thresh'])
    assert set(z['names']) >= {'u0x5', 'u5x0', 'u1x1', 'u7x13', 'u13x7', 'u64x64', 'u65x63', 'u128x128', 'u128x1', 'above', 'sparse'}
    for name in z['names']:
        cost, want = z[name + '_cost'], z[name + '_x']
        x = TR.assign(cost, thresh)
        assert np.array_equal(x, want), name
        assert abs(ext_total(cost, thresh, x) - float(z[name + '_total'])) <= 1e-5, name


def test_solver_equals_scipy_on_fresh_matrices():
    lsa = pytest.importorskip('scipy.optimize').linear_sum_assignment
    rng = np.random.default_rng(11)
    for n, m, thresh in ((3, 3, 0.5), (9, 4, 0.8), (4, 9, 0.7), (30, 31, 0.8), (50, 20, 0.3), (17, 17, 0.99)):
        for _ in range(4):
            cost = rng.uniform(0, 1, (n, m)).astype(np.float32)
            e = np.full((n + m, n + m), thresh / 2)
            e[n:, m:] = 0
            e[:n, :m] = cost
            r, c = lsa(e)
            x = TR.assign(cost, thresh)
            assert abs(ext_total(cost, np.float64(np.float32(thresh)), x) - e[r, c].sum()) <= 1e-5
            assert len(set(x[x >= 0])) == int((x >= 0).sum()) and not (cost[np.nonzero(x >= 0)[0], x[x >= 0]] > thresh).any()


def test_capacity_is_a_flag_not_a_fault():
    """A table of 8 tracks fed 12 objects: the flag is set, the state is as it was, no rows; 8 objects fit."""
    rng = np.random.default_rng(0)
    rows = np.zeros((12, 6), np.float32)
    rows[:, 0], rows[:, 1] = np.arange(12) * 50, rng.uniform(0, 300, 12)
    rows[:, 2], rows[:, 3], rows[:, 4] = rows[:, 0] + 40, rows[:, 1] + 60, 0.9
    trk = TR.Tracker(streams=1, cap=8)
    out, flag = trk.update(0, rows[:8])
    assert flag == 0 and len(out) == 8
    before = trk.s[0].export()
    out, flag = trk.update(0, rows)
    assert flag == TR.FLAG_TRACKS and len(out) == 0
    after = trk.s[0].export()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    many = np.tile(rows[:1], (TR.DET_CAP + 1, 1))
    out, flag = trk.update(0, many)
    assert flag == TR.FLAG_DETS and len(out) == 0 and trk.s[0].frame_id == 1
