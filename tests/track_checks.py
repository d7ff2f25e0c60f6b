"""Shared by tests/test_track_ref.py and tests/test_track.py: the fixtures of tests/golden/gen_track.py and the rules of the comparison.

Rules of the comparison: ids, idx, cls, states and counters exact; scores bit-equal; boxes and filter means within 1e-3 px (the project's box
contract); the expanded covariance exactly zero off the four 2x2 blocks.  On the blocks the covariance is compared at rtol 1e-5: the reference forms
the standard deviations of a new track from a float32 measurement (relative error 2^-24 each, 2^-23 squared), everything after that is float64 in
both, and the recursion is linear in the covariance, so 1e-5 leaves two decimal orders over what the formats allow.
"""
import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEQS = sorted(glob.glob(os.path.join(GOLD, 'track_[0-9][0-9].npz')))
BOX_TOL = 1e-3
OFF_BLOCK = np.ones((8, 8), bool)
for _i in range(4):
    OFF_BLOCK[_i, _i] = OFF_BLOCK[_i, _i + 4] = OFF_BLOCK[_i + 4, _i] = OFF_BLOCK[_i + 4, _i + 4] = False


def cfg_of(z):
    return {k[4:]: float(z[k]) for k in z.files if k.startswith('cfg_')}


def check_rows(got, want, what):
    got, want = np.asarray(got, np.float32).reshape(-1, 8), np.asarray(want, np.float32).reshape(-1, 8)
    assert got.shape == want.shape, f'{what}: {len(got)} rows, expected {len(want)}'
    assert np.array_equal(got[:, [4, 6, 7]], want[:, [4, 6, 7]]), f'{what}: id / cls / idx differ'
    assert np.array_equal(got[:, 5].view(np.uint32), want[:, 5].view(np.uint32)), f'{what}: scores are not bit-equal'
    if len(got):
        err = np.abs(got[:, :4].astype(np.float64) - want[:, :4]).max()
        assert err <= BOX_TOL, f'{what}: box error {err} px'


def check_state(exp, z, b, i, what):
    """exp: an export dict (track_ref.Stream.export / BYTETracker.state); z: a sequence fixture, snapshot i of stream b."""
    n = int(z['snap_n'][b, i])
    assert len(exp['id']) == n, f'{what}: {len(exp["id"])} live tracks, expected {n}'
    for k in ('id', 'state', 'is_activated', 'frame_id', 'start_frame', 'tracklet_len', 'cls'):
        assert np.array_equal(np.asarray(exp[k]).astype(np.float64), z['snap_' + k][b, i, :n].astype(np.float64)), f'{what}: {k} differs'
    assert np.array_equal(np.asarray(exp['score'], np.float32).view(np.uint32), z['snap_score'][b, i, :n].view(np.uint32)), f'{what}: score bits'
    assert int(exp['tracker_frame_id']) == int(z['snap_tracker_frame_id'][b, i]) and int(exp['count']) == int(z['snap_count'][b, i]), what
    if n:
        assert np.abs(exp['mean'] - z['snap_mean'][b, i, :n]).max() <= BOX_TOL, f'{what}: filter mean'
        cov = np.asarray(exp['covariance'])
        assert not cov[:, OFF_BLOCK].any(), f'{what}: covariance off the 2x2 blocks is not exactly zero'
        assert not z['snap_covariance'][b, i, :n][:, OFF_BLOCK].any()
        np.testing.assert_allclose(cov, z['snap_covariance'][b, i, :n], rtol=1e-5, atol=0, err_msg=what)


def ext_total(cost, thresh, x):
    n, m = cost.shape
    r = np.nonzero(x >= 0)[0]
    return float(cost.astype(np.float64)[r, x[r]].sum() + (n + m - 2 * len(r)) * thresh / 2)
