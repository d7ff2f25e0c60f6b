"""Every route of nms_kernel / nms_best_kernel (mgdt_yolo_amd/csrc/nms.hip) and both instantiations of val_match_kernel (val_match.hip) against the CPU
oracle, bit for bit.

Which route of nms_kernel runs depends on the data: how many candidates pass, how their scores fall into the 2048 histogram bins, how soon the
greedy scan reaches max_det.  Every NMS case therefore STATES its route - per segment `selector.sort.np2` with selector hist | rank and sort
shuffle (<= 1024 keys, boxes parked in LDS) | lds (<= 16384) | global - plus cached | uncached keys and the candidate source; the statement is the
case's id, and test_route_census holds nms_ref.nms_plan (a host restatement of the kernel's planner) to it on the CPU.  The GPU tests (-m gpu, a real
MI355X) compare ops.nms / ops.nms_masks with oracle.nms.non_max_suppression(..., return_index=True): kept anchors, kept classes and the output rows
must be BIT-EQUAL; ops.val_match is compared with oracle.val.process_batch the same way.  There is no tolerance in this file.
"""
import functools

import numpy as np
import pytest
import torch

import nms_ref as NR
from oracle import nms as ON
from oracle import val as OV

gpu = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
KW = dict(conf_thres=0.25, iou_thres=0.5)


def cl(seed, A, nc, grid, scores, cls=None):
    return NR.clusters(seed, A, nc, grid, 100.0, 40.0, 1.5, scores, cls)


class Case:
    """One launch.  make() -> (B, 4+nc[+nm], A) float32; route: the segments every image takes (or one list per image); source: where the candidate
    keys come from - best_kernel (nms_best_kernel's scan), multi_label (key_at reads the score rows), best_keys (a `best` tensor attached to y)."""

    def __init__(self, name, make, kw, route, cached=True, source='best_kernel', kept=None, nm=0):
        self.last = 0                                                # 1: _isolate_last put one more keeper at the very end of the key order
        self.name, self._make, self.kw, self.route, self.cached, self.source, self.kept, self.nm = name, make, dict(kw), route, cached, source, kept, nm
        per_image = route and isinstance(route[0], list)
        r = ' / '.join('+'.join(x) or 'none' for x in route) if per_image else ('+'.join(route) or 'none')
        self.id = f'{name}[{r}|{"cached" if cached else "uncached"}|{source}]'

    @functools.lru_cache(maxsize=None)
    def pred(self):
        p = np.ascontiguousarray(self._make(), F32)
        p.setflags(write=False)                                      # shared by the census, the oracle and the GPU run
        return p

    def dev(self):
        return torch.from_numpy(self.pred().copy()).to(DEV)

    @property
    def nc(self):
        return self.pred().shape[1] - 4 - self.nm

    def routes(self):
        B = self.pred().shape[0]
        return self.route if (self.route and isinstance(self.route[0], list)) else [self.route] * B

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        return ON.non_max_suppression(self.pred(), return_index=True, nc=self.nc, **self.kw)

    @functools.lru_cache(maxsize=None)
    def plans(self):
        return [NR.nms_plan(p, nc=self.nc, **self.kw) for p in self.pred()]


def _isolate_last(y, kw):
    """Move the box of the candidate that comes LAST in the kernel's key order (lowest score, then highest candidate id, within max_nms) to a place of
    its own: the oracle keeps it, so a segment that loses its last key or a scan that stops one candidate early shows in the result."""
    nc = y.shape[0] - 4
    _, conf, cls, anc = ON.nms_candidates(y, kw['conf_thres'], kw.get('multi_label', False))
    order = np.argsort(NR.make_key_np(conf, anc * nc + cls), kind='stable')[:kw.get('max_nms', 30000)]
    y[0:2, anc[order[-1]]] = 5000.0
    return y


def _stack(fn, seeds, kw=None):
    return lambda: np.stack([fn(s) if kw is None else _isolate_last(fn(s), kw) for s in seeds])


def _hist_then_rank(seed):
    r = np.random.default_rng(seed)
    s = np.concatenate([NR.distinct_scores(r, 1000, 0.6, 0.99), np.full(7000, 0.40625, F32)])
    return cl(seed, 8000, 2, 8, r.permutation(s))


def _mixed():
    tiny = np.zeros(22000, F32)
    tiny[[3, 500, 9999, 21999, 12000]] = [0.9, 0.8, 0.7, 0.6, 0.3]
    return np.stack([cl(31, 22000, 1, 8, tiny), _isolate_last(cl(32, 22000, 1, 8, 0.5), KW), cl(33, 22000, 1, 8, np.zeros(22000, F32))])


def _ml(seed):
    r = np.random.default_rng(1000 + seed)
    return cl(seed, 2800, 8, 8, r.uniform(0.05, 0.95, (8, 2800)).astype(F32))


KW_ML = dict(conf_thres=0.001, iou_thres=0.5, multi_label=True, agnostic=True)
G3 = ['hist.shuffle.1024', 'hist.lds.4096', 'hist.global.32768']
R3 = ['rank.shuffle.1024', 'rank.lds.4096', 'rank.global.32768']
ROUTE_CASES = [
    # four workgroups on the global-buffer sort at once (B = 4, one seed per image)
    Case('rank-global', _stack(lambda s: cl(s, 22000, 1, 8, 0.5), (1, 2, 3, 4), KW), KW, R3, cached=False, kept=64),
    Case('hist-global', _stack(lambda s: cl(s, 22000, 1, 8, (0.3, 0.99)), (5, 6, 7, 8), KW), KW, G3, cached=False, kept=64),
    Case('hist-global-nc3', _stack(lambda s: cl(s, 23000, 3, 6, (0.3, 0.99)), (9, 10, 11, 12), KW), KW, G3, cached=False, kept=108),
    Case('ml-global', _stack(_ml, (13, 14, 15, 16)), KW_ML, G3, cached=False,
         source='multi_label', kept=64),
    # per-image workspace offsets and counts: a tiny image, a global-route image, an image without a candidate
    Case('mixed-batch', _mixed, KW, [['hist.shuffle.8'], R3, []], cached=False),
    Case('lds2048', _stack(lambda s: cl(s, 1536, 2, 8, (0.3, 0.99)), (17, 18), KW), KW, ['hist.lds.2048'], kept=128),
    Case('two-seg-1537', _stack(lambda s: cl(s, 1537, 2, 8, (0.3, 0.99)), (19, 20), KW), KW, ['hist.shuffle.1024', 'hist.shuffle.1024'], kept=128),
    Case('lds4096', _stack(lambda s: cl(s, 4024, 2, 8, (0.3, 0.99)), (21, 22), KW), KW, ['hist.shuffle.1024', 'hist.lds.4096'], kept=128),
    Case('lds8192', _stack(lambda s: cl(s, 6000, 2, 8, (0.3, 0.99)), (23, 24), KW), KW, ['hist.shuffle.1024', 'hist.lds.8192'], kept=128),
    Case('lds16384', _stack(lambda s: cl(s, 16000, 2, 8, (0.3, 0.99)), (25, 26), KW), KW, ['hist.shuffle.1024', 'hist.lds.4096', 'hist.lds.16384'],
         cached=False, kept=128),
    Case('hist-then-rank', _stack(_hist_then_rank, (27, 28), KW), KW, ['hist.shuffle.1024', 'rank.lds.4096', 'rank.lds.4096'], kept=128),
    Case('max-nms-cut-late', _stack(lambda s: cl(s, 8000, 2, 8, (0.3, 0.99)), (29, 30), dict(KW, max_nms=5000)), dict(KW, max_nms=5000), ['hist.shuffle.1024', 'rank.lds.4096'],
         kept=128),
]
for _c in ROUTE_CASES:
    _c.last = int(_c.name not in ('ml-global', 'mixed-batch'))
# exact key counts where the plan fixes them (rank select and single segments)
EXACT_KEYS = {'rank-global': [1024, 4096, 16880], 'lds2048': [1536], 'hist-then-rank': [1000, 4096, 2904]}


# ---- suppression chains: 40 x 40 boxes on a line, step 10 (IoU 0.6 with the neighbour, 1/3 with the next-but-one); greedy keeps every second
def _chain(length, shift, reverse):
    def make():
        A, nc = 300, 2
        r = np.random.default_rng(length * 1000 + shift + reverse)
        y = np.zeros((4 + nc, A), F32)
        y[0] = 6000 + 100 * np.arange(A); y[1] = 100; y[2] = 30; y[3] = 30        # isolated fillers
        perm = r.permutation(A)
        ch, top, rest = perm[:length], perm[length:length + shift], perm[length + shift:]
        y[:4, ch] = NR.chain(length, 100.0)
        along = np.arange(length)[::-1] if reverse else np.arange(length)
        y[5, ch] = (0.99 - 0.0009 * along).astype(F32)
        y[5, top] = (0.992 + 0.0001 * np.arange(shift)).astype(F32)                 # `shift` isolated boxes ahead of the chain in score order
        y[4, rest] = (0.3 + 0.001 * np.arange(len(rest))).astype(F32)
        return y[None]
    return make


CHAIN_CASES = [Case(f'chain{n}-at{s}{"-rev" if rev else ""}', _chain(n, s, rev), KW, ['hist.shuffle.512']) for n, s, rev in
               [(64, 0, 0), (64, 37, 0), (65, 0, 0), (65, 37, 0), (200, 0, 0), (200, 37, 0), (64, 0, 1)]]

# ---- max_det: odd (the padding in front of the kept keys), 1, around a chunk of 64, the LDS limit; the oracle keeps ~870 boxes here
MAX_DETS = (1, 7, 63, 64, 65, 301, 804)
_maxdet_input = functools.lru_cache(maxsize=None)(lambda: cl(41, 1990, 1, 32, (0.3, 0.99))[None])
MAXDET_CASES = [Case(f'max_det{md}', _maxdet_input, dict(KW, max_det=md), ['hist.shuffle.1024'] + (['hist.shuffle.1024'] if md > 650 else []))
                for md in MAX_DETS]


# ---- nms_best_kernel: class counts around its unrolled-by-8 loop, ties between classes of one anchor, a class filter that removes the best class
def _nc_input(nc, A):
    def make():
        r = np.random.default_rng(nc * 1000 + A)
        y = np.zeros((4 + nc, A), F32)
        y[0] = r.uniform(20, 600, A); y[1] = r.uniform(20, 600, A); y[2] = r.uniform(8, 60, A); y[3] = r.uniform(8, 60, A)
        y[4:] = r.uniform(0.3, 0.9, (nc, A)).astype(F32)
        if nc > 1:                                                                  # every second anchor: two classes with bit-identical maximal scores
            for a in range(0, A, 2):
                c0, c1 = (a // 2) % nc, (a // 2 * 7 + 3) % nc
                if c0 != c1:
                    y[4 + c0, a] = y[4 + c1, a] = F32(0.9) + F32(0.0001) * F32(a % 64)
        return y[None]
    return make


NC_CASES = []
NC_FILTER_ROUTE = {(2, 255): ['hist.shuffle.64'], (2, 257): ['hist.shuffle.128']}
NC_FILTER_ROUTE.update({(n, 1): [] for n in (2, 8, 9, 10, 16, 17, 81)})              # the only anchor's best class (0, tied with a later one) is filtered out
NC_FILTER_ROUTE.update({(n, 255): ['hist.shuffle.256'] for n in (8, 9, 10, 16, 17, 81)})
for _nc in (1, 2, 8, 9, 10, 16, 17, 81):
    for _A in (1, 255, 257):
        _np2 = {1: 1, 255: 256, 257: 512}[_A]
        NC_CASES.append(Case(f'nc{_nc}-A{_A}', _nc_input(_nc, _A), KW, [f'hist.shuffle.{_np2}']))
        _cls = [c for c in range(_nc) if c % 3 != 0] if _nc > 1 else [0]
        # the filter removes about a third of the candidates (nc = 2: half of them, and the only anchor of A = 1)
        _r = [f'hist.shuffle.{_np2}'] if _nc == 1 else NC_FILTER_ROUTE.get((_nc, _A), [f'hist.shuffle.{max(_np2 // 2, 1)}'])
        NC_CASES.append(Case(f'nc{_nc}-A{_A}-filter', _nc_input(_nc, _A), dict(KW, classes=_cls), _r))


# ---- threshold edges
def _edge_scores():
    """conf_thres = 0: scores 0 (excluded), the smallest subnormal, exact multiples of 1/2048 (histogram bin edges) with their +-1 ulp neighbours."""
    r = np.random.default_rng(51)
    m = r.choice(np.arange(1, 2048), 600, replace=False).astype(F32) / F32(2048)
    pool = np.concatenate([m, np.nextafter(m, F32(0)), np.nextafter(m, F32(2)), np.zeros(60, F32), np.full(40, np.nextafter(F32(0), F32(1)), F32),
                           np.full(20, 1.0, F32)])
    return cl(51, len(pool), 2, 8, r.permutation(pool))[None]


def _conf_edge():
    r = np.random.default_rng(52)
    c = F32(0.25)
    pool = np.concatenate([np.full(100, c), np.full(100, np.nextafter(c, F32(1))), np.full(100, np.nextafter(c, F32(0))), np.full(100, 1.0, F32),
                           NR.distinct_scores(r, 400, 0.2, 1.0)])
    return cl(52, len(pool), 3, 4, r.permutation(pool))[None]


def _zero_area():
    y = np.zeros((6, 12), F32)
    y[:4, 0:3] = np.array([[50, 50, 0, 0]], F32).T                                  # three identical zero-area boxes: 0 / 0 is NaN, nothing is suppressed
    y[:4, 3:5] = np.array([[50, 50, 20, 20]], F32).T                                # a box around them (inter 0) and its copy (IoU 1)
    y[:4, 5:7] = np.array([[200, 50, 0, 10]], F32).T                                # zero width
    y[:4, 7:9] = np.array([[300, 50, 10, 0]], F32).T                                # zero height
    y[:4, 9:12] = np.array([[400, 50, 10, 10]], F32).T
    y[4] = np.linspace(0.9, 0.4, 12).astype(F32)
    return y[None]


EDGE_CASES = [
    Case('conf0-bin-edges', _edge_scores, dict(conf_thres=0.0, iou_thres=0.5), ['hist.shuffle.1024', 'hist.shuffle.1024']),
    Case('conf-edge-ones', _conf_edge, KW, ['hist.shuffle.1024']),
    Case('iou0', lambda: cl(53, 900, 2, 8, (0.3, 0.99))[None], dict(conf_thres=0.25, iou_thres=0.0), ['hist.shuffle.1024']),
    Case('iou1', lambda: cl(54, 900, 2, 8, (0.3, 0.99))[None], dict(conf_thres=0.25, iou_thres=1.0), ['hist.shuffle.1024']),
    Case('zero-area', _zero_area, KW, ['hist.shuffle.16']),
]

# ---- hand-made best keys (the Detect tail's output restated on the host), with a class filter and with more anchors than the register cache holds
BESTKEY_CASES = [
    Case('bestkeys-filter', lambda: _nc_input(9, 1500)(), dict(KW, classes=[1, 2, 4, 5, 7, 8]), ['hist.shuffle.1024'], source='best_keys'),
    Case('bestkeys-9000', _stack(lambda s: cl(s, 9000, 4, 8, (0.3, 0.99)), (55, 56)), KW, ['hist.shuffle.1024', 'hist.lds.4096', 'hist.lds.4096'],
         cached=False, source='best_keys'),
]


# ---- ops.nms_masks: the same selection with nm more rows behind the class scores
def _masks(seed, A, nc, nm, grid):
    def make():
        r = np.random.default_rng(seed)
        return np.stack([np.concatenate([cl(seed + i, A, nc, grid, (0.3, 0.99)), r.standard_normal((nm, A)).astype(F32)]) for i in range(2)])
    return make


MASK_CASES = [
    Case('masks-nc1-nm51', _masks(61, 1537, 1, 51, 8), KW, ['hist.shuffle.1024', 'hist.shuffle.1024'], nm=51, kept=64),
    Case('masks-nc3-nm1', _masks(63, 700, 3, 1, 6), KW, ['hist.shuffle.1024'], nm=1, kept=108),
    Case('masks-nc80-nm32', _masks(65, 1000, 80, 32, 4), KW, ['hist.shuffle.1024'], nm=32),
]

NMS_CASES = ROUTE_CASES + CHAIN_CASES + MAXDET_CASES + NC_CASES + EDGE_CASES + BESTKEY_CASES
ALL_CASES = NMS_CASES + MASK_CASES
_ids = lambda cs: [c.id for c in cs]


# ================================================================================================ host tests
def _route_of(plan):
    return [f'{sel}.{sort}.{np2}' for sel, _, np2, sort, _ in plan['segments']]


def test_case_ids_are_unique():
    ids = _ids(ALL_CASES)
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


def test_plan_constants_match_the_kernel():
    """nms_ref.nms_plan repeats four numbers of nms.hip; a retune of the kernel fails here and not by silently moving cases onto another route."""
    assert NR.kernel_constants() == dict(NMS_THREADS=NR.NMS_THREADS, NMS_LDS_KEYS=NR.NMS_LDS_KEYS, NMS_BINS=NR.NMS_BINS, KPT=NR.KPT)
    src = open(NR.NMS_HIP).read()
    assert 'unsigned done = 0, seg = 1024;' in src and 'seg *= 4;' in src and 'lds > 150 * 1024' in src
    # the "do not leave a small tail" rule changes the plan and never the result: no output comparison can see it go, so its text is pinned here
    assert src.count('(K - done <= seg + seg / 2)') == 2 and 'const bool cached = total <= (long)KPT * NMS_THREADS;' in src


def test_max_det_lds_arithmetic():
    """804 is the largest max_det whose kept list fits beside the sort keys: 131072 + 28 * max_det (+ 4 if odd) <= 150 KiB."""
    assert NR.lds_bytes(804) == 131072 + 28 * 804 <= NR.LDS_LIMIT
    assert NR.lds_bytes(805) == 131072 + 28 * 805 + 4 > NR.LDS_LIMIT and NR.lds_bytes(806) > NR.LDS_LIMIT
    assert all(NR.lds_bytes(md) <= NR.LDS_LIMIT for md in MAX_DETS) and max(MAX_DETS) == 804


@pytest.mark.parametrize('c', ALL_CASES, ids=_ids(ALL_CASES))
def test_route_census(c):
    """nms_ref.nms_plan (the kernel's planner restated on the host) sends every image of the case down exactly the route the case states."""
    plans, routes = c.plans(), c.routes()
    assert len(plans) == len(routes)
    for i, (p, want) in enumerate(zip(plans, routes)):
        assert _route_of(p) == want, (i, p)
        assert p['cached'] == c.cached, (i, p)
        for sel, cnt, np2, sort, kept0 in p['segments']:
            assert np2 // 2 < cnt <= np2 and kept0 < c.kw.get('max_det', 300)
        if c.kept is not None and len(want) > 1:                     # the scan has found every cluster by the end of the first segment and goes on
            assert [s[4] for s in p['segments'][1:]] == [c.kept] * (len(want) - 1), (i, p)
        if c.kept is not None:                                       # ... and the isolated last candidate (_isolate_last) is kept on top of them
            assert p['kept'] == c.kept + c.last, (i, p)
        if c.name in EXACT_KEYS:
            assert [s[1] for s in p['segments']] == EXACT_KEYS[c.name], (i, p)
    if c.source == 'multi_label':
        assert c.kw.get('multi_label') and all(p['ncand'] == p['total'] == c.pred().shape[2] * c.nc for p in plans)


def test_route_census_covers_every_route():
    seen = [(c, i, p) for c in ALL_CASES for i, p in enumerate(c.plans())]
    segs = [(c, k, s) for c, _, p in seen for k, s in enumerate(p['segments'])]
    assert any(s[3] == 'shuffle' and k == 0 for _, k, s in segs) and any(s[3] == 'shuffle' and k > 0 for _, k, s in segs)
    assert {s[2] for _, _, s in segs if s[3] == 'lds'} == {2048, 4096, 8192, 16384}
    assert {s[0] for _, _, s in segs if s[3] == 'global'} == {'hist', 'rank'}
    assert sum(1 for c, i, p in seen if p['segments'] and p['segments'][-1][3] == 'global') >= 17          # four batches of four + the mixed batch
    # rank select after a histogram segment, with more segments to come (select_rank runs with done > 0 and a histogram edge as lo_key)
    assert any([s[0] for s in p['segments']][:3] == ['hist', 'rank', 'rank'] for _, _, p in seen)
    # max_nms cuts inside a later segment
    assert any(p['K'] < p['ncand'] and len(p['segments']) > 1 and p['segments'][-1][0] == 'rank' for _, _, p in seen)
    assert {p['cached'] for _, _, p in seen} == {True, False}
    assert any(not p['cached'] and len(p['segments']) > 1 for c, _, p in seen if c.source == 'best_kernel')
    assert {c.source for c in ALL_CASES} == {'best_kernel', 'multi_label', 'best_keys'}
    assert any(not p['cached'] for c, _, p in seen if c.source == 'best_keys') and any(c.kw.get('classes') for c in BESTKEY_CASES)
    # a wave's block of the LDS sort is exactly 128 elements at np2 = 2048, the smallest with wave-local passes
    assert 2048 // (NR.NMS_THREADS // 64) == 128
    assert any(len(p['segments']) == 2 for c in MASK_CASES for p in c.plans())


def test_chain_geometry_and_expected_keepers():
    """IoU 0.6 / (1/3) along the chain, so the oracle keeps every second box; with 64 boxes in sorted positions 0..63 that is a 64-long dependency
    chain inside one chunk, the most the kernel's fixed-point loop (64 rounds) resolves."""
    b = NR.chain(3, 100.0).T
    xyxy = np.stack([b[:, 0] - 20, b[:, 1] - 20, b[:, 0] + 20, b[:, 1] + 20], 1)
    inter = lambda p, q: max(0, min(p[2], q[2]) - max(p[0], q[0])) * max(0, min(p[3], q[3]) - max(p[1], q[1]))
    assert inter(xyxy[0], xyxy[1]) / (3200 - inter(xyxy[0], xyxy[1])) == 0.6 and inter(xyxy[0], xyxy[2]) / (3200 - inter(xyxy[0], xyxy[2])) == 1 / 3
    for c in CHAIN_CASES:
        n = int(c.name[5:].split('-')[0])
        _, okept = c.oracle()
        cls1 = int((okept[0][1] == 1).sum())
        shift = 37 if 'at37' in c.name else 0
        assert cls1 == (n + 1) // 2 + shift, (c.name, cls1)
        # sorted positions of the chain: shift .. shift + n - 1
        sc = c.pred()[0, 4:].max(0)
        pos = np.argsort(-sc, kind='stable')
        assert (c.pred()[0, 1, pos[shift:shift + n]] == 2000).all() and (c.pred()[0, 1, pos[:shift]] == 100).all()


def test_nc_inputs_have_ties_and_filtered_best_classes():
    for c in NC_CASES:
        p = c.pred()[0, 4:]
        if c.nc > 1 and p.shape[1] > 1:
            top = p.max(0)
            assert ((p == top).sum(0) == 2).sum() >= p.shape[1] // 4, c.name                 # two classes share the maximum, bit for bit
        if c.kw.get('classes') and c.nc > 1 and p.shape[1] > 1:
            best = p.argmax(0)
            assert (~np.isin(best, c.kw['classes'])).sum() >= 10, c.name                         # anchors whose best class the filter removes
            _, okept = c.oracle()
            assert not np.isin(okept[0][0], np.nonzero(~np.isin(best, c.kw['classes']))[0]).any()


def test_edge_inputs_hold_what_they_claim():
    s = _edge_scores()[0, 4:].max(0)
    assert (s == 0).sum() == 60 and (s == np.nextafter(F32(0), F32(1))).sum() == 40 and (s == 1).sum() == 20
    on_edge = s[(s * 2048 == np.floor(s * 2048)) & (s > 0) & (s < 1)]
    assert len(on_edge) == 600 and np.isin(np.nextafter(on_edge, F32(0)), s).all() and np.isin(np.nextafter(on_edge, F32(2)), s).all()
    plan = EDGE_CASES[0].plans()[0]
    assert plan['ncand'] == len(s) - 60 > 1024                                                   # the subnormal passes conf_thres = 0, zero does not
    s = _conf_edge()[0, 4:].max(0)
    assert (s == F32(0.25)).sum() == 100 and EDGE_CASES[1].plans()[0]['ncand'] == (s > F32(0.25)).sum()


# ================================================================================================ GPU tests
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _assert_equal(rows, kept, oracle, what):
    orows, okept = oracle
    assert len(rows) == len(orows)
    for i in range(len(orows)):
        k = kept[i].cpu().numpy().astype(np.int64)
        r = rows[i].cpu().numpy()
        assert len(k) == len(okept[i][0]), (what, i, len(k), len(okept[i][0]))
        assert np.array_equal(k, okept[i][0]), (what, i, 'kept anchors')
        assert np.array_equal(r[:, 5].astype(np.int64), okept[i][1]), (what, i, 'kept classes')
        assert np.array_equal(_bits(r[:, :6]), _bits(orows[i])), (what, i, 'rows')


def _run(c, y=None):
    from mgdt_yolo_amd.yolo.utils.ops import nms_with_index
    y = c.dev() if y is None else y
    rows, kept = nms_with_index(y, **c.kw)
    _assert_equal(rows, kept, c.oracle(), c.id)
    return rows, kept


@gpu
@pytest.mark.parametrize('c', ROUTE_CASES, ids=_ids(ROUTE_CASES))
def test_nms_segment_routes(c):
    rows, kept = _run(c)
    if c.name == 'mixed-batch':
        assert [len(k) for k in kept] == [5, 65, 0]
    elif c.kept is not None:
        assert all(len(k) == c.kept + c.last for k in kept)


@gpu
@pytest.mark.parametrize('c', CHAIN_CASES, ids=_ids(CHAIN_CASES))
def test_nms_suppression_chains(c):
    _run(c)


@gpu
@pytest.mark.parametrize('c', MAXDET_CASES, ids=_ids(MAXDET_CASES))
def test_nms_max_det(c):
    rows, kept = _run(c)
    assert len(kept[0]) == c.kw['max_det']


@gpu
def test_nms_max_det_beyond_the_lds_limit_raises_before_any_launch():
    from mgdt_yolo_amd import ops
    c = MAXDET_CASES[-1]
    y = c.dev()
    with pytest.raises(RuntimeError, match='max_det=805 too large'):
        ops.nms(y, 0.25, 0.5, None, False, False, 805, 30000, 7680)
    torch.cuda.synchronize()
    _run(c, y)                                                      # the process is still usable: the 804 case


@gpu
@pytest.mark.parametrize('c', NC_CASES, ids=_ids(NC_CASES))
def test_nms_best_class_scan(c):
    _run(c)


@gpu
@pytest.mark.parametrize('c', EDGE_CASES, ids=_ids(EDGE_CASES))
def test_nms_threshold_edges(c):
    _run(c)


@gpu
@pytest.mark.parametrize('cls,agnostic,jog', [(0, True, 0.0), (3, False, 0.0), (3, False, 0.3)], ids=['agnostic', 'class3-offset', 'class3-offset-rounded'])
def test_nms_iou_exactly_on_the_threshold(cls, agnostic, jog):
    """[0,0,2,1] against [0,0,1,1]: IoU is exactly 0.5 in fp32 (also after the exact class offset 3 * 7680), not suppressed at iou_thres = 0.5 (strict >),
    suppressed at the next float below.  `jog` moves both boxes by 0.3 so that the class offset rounds their coordinates: oracle equality only."""
    from mgdt_yolo_amd.yolo.utils.ops import nms_with_index
    y = np.zeros((1, 8, 2), F32)
    y[0, :4, 0] = [1 + jog, 0.5 + jog, 2, 1]
    y[0, :4, 1] = [0.5 + jog, 0.5 + jog, 1, 1]
    y[0, 4 + cls] = [0.9, 0.8]
    below = float(np.nextafter(F32(0.5), F32(0)))
    for thr in (0.5, below):
        kw = dict(conf_thres=0.25, iou_thres=thr, agnostic=agnostic)
        rows, kept = nms_with_index(torch.from_numpy(y).to(DEV), **kw)
        _assert_equal(rows, kept, ON.non_max_suppression(y, return_index=True, **kw), (cls, agnostic, jog, thr))
        if jog == 0.0:
            assert len(kept[0]) == (2 if thr == 0.5 else 1)


@gpu
@pytest.mark.parametrize('c', BESTKEY_CASES, ids=_ids(BESTKEY_CASES))
def test_nms_hand_made_best_keys(c):
    """A `best` tensor built on the host with nms_ref.make_key and attached to y: the kernel reads its candidates from it (no nms_best_kernel launch).
    Rows equal the oracle and the run without the keys; a key that lies about one anchor shows that the keys are what the kernel read."""
    from mgdt_yolo_amd import ops
    from mgdt_yolo_amd.yolo.utils.ops import nms_with_index
    B, _, A = c.pred().shape
    y = c.dev()
    best = NR.best_keys(c.pred(), c.nc)
    ops.attach_best_keys(y, best.to(DEV))
    assert ops._best_keys_of(y, B, A) is not None
    rows, kept = _run(c, y)
    ops.NMS_USE_BEST_KEYS = False
    try:
        assert ops._best_keys_of(y, B, A) is None
        rows2, kept2 = _run(c, y)
    finally:
        ops.NMS_USE_BEST_KEYS = True
    for i in range(B):
        assert torch.equal(rows[i], rows2[i]) and torch.equal(kept[i], kept2[i])
    top = int(kept[0][0])                                           # image 0's best box: give its key a zero score
    lie = best.clone()
    lie[0, top] = NR.make_key(np.zeros(1, F32), np.asarray([top * c.nc]))[0]
    ops.attach_best_keys(y, lie.to(DEV))
    _, kept3 = nms_with_index(y, **c.kw)
    assert top not in kept3[0].tolist()
    ops.attach_best_keys(y, best.to(DEV))
    y.mul_(1.0)                                                     # an in-place write: the keys no longer describe y
    assert ops._best_keys_of(y, B, A) is None
    _run(c, y)


@gpu
@pytest.mark.parametrize('c', MASK_CASES, ids=_ids(MASK_CASES))
def test_nms_masks_rows(c):
    from mgdt_yolo_amd import ops
    p = c.pred()
    out, kept, counts = ops.nms_masks(c.dev(), c.nm, 0.25, 0.5, None, False, False, 300, 30000, 7680)
    counts = counts.tolist()
    rows = [out[i, :n] for i, n in enumerate(counts)]
    _assert_equal(rows, [kept[i, :n] for i, n in enumerate(counts)], c.oracle(), c.id)
    for i, n in enumerate(counts):
        assert n > 0 and (c.kept is None or n == c.kept)
        want = p[i, 4 + c.nc:, kept[i, :n].cpu().numpy()]
        assert np.array_equal(_bits(rows[i][:, 6:].cpu().numpy()), _bits(want)), (c.id, i)


# ================================================================================================ validator matching
VM_MAX_DET, VM_MAX_LAB = 600, 40
VM_LEVELS = {1: torch.tensor([0.5]), 10: torch.linspace(0.5, 0.95, 10), 16: torch.linspace(0.2, 0.95, 16)}


@functools.lru_cache(maxsize=None)
def _vm_images():
    """(name, det, lab, claimed ndet, claimed nlab): three rounds of 256 detections, counts beyond the buffers (clamped), empty images side by side."""
    imgs = [(n, d, l, len(d), len(l)) for n, d, l in NR.val_crafted()]
    d, l = NR.val_random(71, 600, 40)
    imgs.append(('random600', d, l, 600, 40))
    d, l = NR.val_random(72, 600, 40)
    imgs.append(('clamped', d, l, 700, 50))
    d, l = NR.val_random(73, 100, 10)
    imgs.append(('no_labels', d, l[:0], 100, 0))
    imgs.append(('no_detections', d[:0], l, 0, 10))
    d, l = NR.val_random(74, 257, 33, wrong_cls=0.4)
    imgs.append(('random257', d, l, 257, 33))
    return imgs


@pytest.mark.parametrize('T', sorted(VM_LEVELS))
def test_val_match_inputs_have_no_tie(T):
    """The reference decides an exact IoU tie between two labels of one detection by numpy's unstable sort; no input may hold one.  A condition on the
    inputs, not a tolerance."""
    for name, d, l, _, _ in _vm_images():
        assert not NR.val_has_tie(d, l, VM_LEVELS[T].numpy()), name


def test_val_match_inputs_hold_what_they_claim():
    imgs = {n: (d, l) for n, d, l, _, _ in _vm_images()}
    d, l = imgs['iou_on_level']
    iou = OV.box_iou(torch.from_numpy(l[:, 1:]), torch.from_numpy(d[:, :4])).numpy()
    assert iou[0, 0] == F32(0.5) == VM_LEVELS[10][0].item() == VM_LEVELS[1][0].item() and iou[1, 1] == F32(0.75)
    assert 0.4999 < iou[2, 2] < 0.5 and 0.7499 < iou[3, 3] < 0.75
    iouv = VM_LEVELS[10]
    c = OV.process_batch(torch.from_numpy(d), torch.from_numpy(l), iouv)
    assert c[0, 0] and c[1, 0] and not c[2].any() and not c[3, 5:].any()
    d, l = imgs['late_only']
    c = OV.process_batch(torch.from_numpy(d), torch.from_numpy(l), iouv)
    assert c[300].any() and c[599].any() and c.any(1).sum() == 2
    d, l = imgs['cross_round']
    c = OV.process_batch(torch.from_numpy(d), torch.from_numpy(l), iouv)
    assert c[10, 0] and not c[400, 0] and not c[580, 0] and c[400, -1] and not c[10, -1]       # the lower index wins where both pass the level
    assert c[255, 0] and not c[256, 0] and c[256, -1]
    d, l = imgs['class_never_seen']
    assert not OV.process_batch(torch.from_numpy(d), torch.from_numpy(l), iouv).any()
    d, l = imgs['random600']
    c = OV.process_batch(torch.from_numpy(d), torch.from_numpy(l), iouv)
    assert c[:256].any() and c[256:512].any() and c[512:].any()


@functools.lru_cache(maxsize=None)
def _vm_batch():
    """The images of `_vm_images` in the batch layout (host tensors): det, ndet, lab, nlab."""
    imgs = _vm_images()
    b = len(imgs)
    det = torch.zeros(b, VM_MAX_DET, 6); lab = torch.zeros(b, VM_MAX_LAB, 5)
    ndet = torch.zeros(b, dtype=torch.int32); nlab = torch.zeros(b, dtype=torch.int32)
    for i, (_, d, l, nd, nl) in enumerate(imgs):
        det[i, :len(d)] = torch.from_numpy(d); lab[i, :len(l)] = torch.from_numpy(l)
        ndet[i], nlab[i] = nd, nl
    return det, ndet, lab, nlab


def _vm_check(correct, iouv):
    imgs = _vm_images()
    assert correct.shape == (len(imgs), VM_MAX_DET, len(iouv))
    for i, (name, d, l, nd, nl) in enumerate(imgs):
        ref = OV.process_batch(torch.from_numpy(d), torch.from_numpy(l), iouv)
        assert np.array_equal(correct[i, :len(d)], ref), (name, len(iouv))
        assert not correct[i, len(d):].any(), (name, len(iouv))


@gpu
@pytest.mark.parametrize('T', sorted(VM_LEVELS))
def test_val_match_bit_equal(T):
    from mgdt_yolo_amd import ops
    iouv = VM_LEVELS[T]
    det, ndet, lab, nlab = (t.to(DEV) for t in _vm_batch())
    _vm_check(ops.val_match(det, ndet, lab, nlab, iouv.to(DEV)).cpu().numpy(), iouv)


@gpu
@pytest.mark.parametrize('T', sorted(VM_LEVELS))
def test_val_match_iou_on_the_box_iou_matrix_equals_val_match(T):
    """Both instantiations of val_match_kernel obey one rule: the matrix source, fed with the (B, max_lab, max_det) float32 box IoUs computed on the CPU
    in the kernel's operation order (oracle.val.box_iou; zero past nlab / ndet), returns what the box source returns on the boxes, and what the oracle
    returns.  The inputs hold no tie (test_val_match_inputs_have_no_tie), so the reference alone decides every entry."""
    from mgdt_yolo_amd import ops
    iouv = VM_LEVELS[T]
    det, ndet, lab, nlab = _vm_batch()
    iou = torch.zeros(len(det), VM_MAX_LAB, VM_MAX_DET)
    for i, (_, d, l, _, _) in enumerate(_vm_images()):
        if len(d) and len(l):
            iou[i, :len(l), :len(d)] = OV.box_iou(torch.from_numpy(l[:, 1:]), torch.from_numpy(d[:, :4]))
    assert iou.dtype == torch.float32
    det, ndet, lab, nlab = (t.to(DEV) for t in (det, ndet, lab, nlab))
    from_matrix = ops.val_match_iou(iou.to(DEV), det, ndet, lab, nlab, iouv.to(DEV))
    assert torch.equal(from_matrix, ops.val_match(det, ndet, lab, nlab, iouv.to(DEV))), T
    _vm_check(from_matrix.cpu().numpy(), iouv)
