"""Pose validation: object keypoint similarity (mgdt_kpt_iou_fwd), metrics.kpt_iou and PoseValidator against what the reference's own code returned
on seeded inputs (tests/golden/poseval_00.npz, produced by tests/golden/gen_poseval.py; inputs re-created by tests/poseval_ref.py).

Output convention pinned here: entries of the OKS matrix past nlab[i] / counts[i] are WRITTEN as zero; nothing outside the (B, max_lab, max_det)
block is touched (guard values before and after).

OKS bound: max |device - fp64| <= max(4 * d64, 1e-6), d64 the reference's own fp32-vs-fp64 difference recorded per case (about 1e-7).  The floor:
a term exp(-e) moves by at most e * exp(-e) <= 0.37 times the relative error of e, about six roundings of 2^-24 (the differences, their squares
and sum, sigma, the coefficient, the product); add two ulps of the exponential, the roundings of a sum of at most 17 terms and the closing
multiplication: below 1e-6 for values in [0, 1]."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseval_ref as R  # noqa: E402

from mgdt_yolo_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
KEYS = [f'metrics/{k}({s})' for s in 'BP' for k in ('precision', 'recall', 'mAP50', 'mAP50-95')]
_FIX = []


def fixture():
    if not _FIX:
        _FIX.append(R.load_fixture())
    return _FIX[0]


def bound(g, name):
    return max(4.0 * float(g[name + '_d64']), 1e-6)


# ------------------------------------------------------------------------------------------------ host
def test_new_entry_point_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    declared = set(re.findall(r'\b(mgdt_[a-z0-9_]+)\s*\(', hdr))
    assert 'mgdt_kpt_iou_fwd' in declared and 'mgdt_kpt_iou_fwd' in _lib.PROTOTYPES and hasattr(_lib.lib(), 'mgdt_kpt_iou_fwd')
    from mgdt_yolo_amd import ops
    assert (ops.KPT_IOU_MAX_DET, ops.KPT_IOU_MAX_LAB, ops.KPT_IOU_MAX_NKPT) == (1024, 256, 120)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    BAD_SHAPE, BAD_ARG = -1, -4
    p = 16          # a non-null address that is never dereferenced: every refusal below happens on the host
    ok = dict(pred=p, stride=57, ndim=3, counts=p, n=1, max_det=300, gt=p, area=p, nlab=p, max_lab=20, nkpt=17, sigma=p, eps=1e-7, oks=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mgdt_kpt_iou_fwd(a['pred'], a['stride'], a['ndim'], a['counts'], a['n'], a['max_det'], a['gt'], a['area'], a['nlab'], a['max_lab'],
                                    a['nkpt'], a['sigma'], a['eps'], a['oks'], None)
    for k in ('pred', 'counts', 'gt', 'area', 'nlab', 'sigma', 'oks'):
        assert call(**{k: None}) == BAD_ARG, k
        assert b'null' in lib.mgdt_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(max_det=0), dict(max_det=1025), dict(max_lab=0), dict(max_lab=257), dict(nkpt=0), dict(nkpt=121, stride=400),
               dict(ndim=1), dict(ndim=4, stride=100), dict(stride=50), dict(ndim=2, nkpt=5, stride=9), dict(stride=(1 << 20) + 1),
               dict(n=65535, max_det=1024, max_lab=256)):
        assert call(**kw) == BAD_SHAPE, kw
        assert b'kpt_iou' in lib.mgdt_last_error()


def test_validator_refuses_host_tooling_and_kpt_iou_refuses_cpu_tensors():
    from mgdt_yolo_amd.yolo.utils.metrics import kpt_iou
    from mgdt_yolo_amd.yolo.v8.pose import PoseValidator
    for k in ('plots', 'save_json', 'single_cls', 'save_hybrid'):
        with pytest.raises(RuntimeError, match='host-side tooling'):
            PoseValidator(device='cpu', args={k: True})
    v = PoseValidator(device='cpu', args=dict(plots=False))
    for fn in (v.pred_to_json, v.plot_predictions, v.plot_val_samples, v.eval_json):
        with pytest.raises(RuntimeError, match='host-side tooling'):
            fn()
    with pytest.raises(RuntimeError, match='no CPU'):
        kpt_iou(torch.zeros(2, 17, 3), torch.zeros(3, 17, 3), torch.ones(2), R.OKS_SIGMA)
    v.init_metrics()
    assert np.array_equal(v.sigma, R.OKS_SIGMA) and v.kpt_shape == (17, 3)
    v.init_metrics(kpt_shape=(5, 2))
    assert np.array_equal(v.sigma, np.ones(5) / 5)
    with pytest.raises(RuntimeError, match='kpt_shape'):
        v.init_metrics(kpt_shape=(5, 4))


def test_oks_sigma_equals_the_references():
    from mgdt_yolo_amd.yolo.utils.metrics import OKS_SIGMA
    g = fixture()
    assert OKS_SIGMA.dtype == np.float64 and np.array_equal(OKS_SIGMA, g['oks_sigma']) and np.array_equal(R.OKS_SIGMA, g['oks_sigma'])


def _native_images(name):
    """-> kpt_shape, [(det (nd, 6), pk (nd, nkpt, ndim), lab (nl, 5), gk (nl, nkpt, 3))] in native space, keys of the fixture."""
    if name in R.CASES:
        return R.CASES[name][0], R.case_inputs(name), [f'{name}_{k}' for k in range(len(R.CASES[name][2]))]
    import pose_ref as PR
    tag = name[len('chain_'):]
    shape, rp = R.CHAIN_BOXES[tag]
    rows, batch = R.chain_inputs(PR.load_fixture())
    imgs = []
    for si, rw in enumerate(rows):
        sel = batch['batch_idx'] == si
        lab, tk = R.native_labels(R.FRAME, batch['cls'][sel], batch['bboxes'][sel], batch['keypoints'][sel], shape, rp)
        det = np.concatenate([R.scale_boxes_f32(R.FRAME, rw, shape, rp), rw[:, 4:6]], 1)
        imgs.append((det, R.scale_coords_f32(R.FRAME, rw[:, 6:].reshape(-1, 17, 3), shape, rp), lab, tk))
    return (17, 3), imgs, [f'{name}_{si}' for si in range(len(rows))]


ALL_CASES = list(R.CASES) + [f'chain_{t}' for t in R.CHAIN_BOXES]


@pytest.mark.parametrize('name', ALL_CASES)
def test_restatement_reproduces_the_fixture(name):
    """The float64 restatement the GPU tests lean on: OKS within the case's recorded d64 of the reference's float32 matrix, both `correct` matrices
    exactly outside the exception list."""
    g = fixture()
    kpt_shape, imgs, keys = _native_images(name)
    d64 = float(g[name + '_d64'])
    assert 0 < d64 < 2.5e-7               # the reference's own float32 error: the derived floor of 1e-6 is the bound of every case
    n_exc = n_det = 0
    for key, (det, pk, lab, gk) in zip(keys, imgs):
        nd, nl = det.shape[0], lab.shape[0]
        assert g[key + '_oks'].shape == (nl, nd) and g[key + '_exc'].shape == (nd,)
        n_exc, n_det = n_exc + int(g[key + '_exc'].sum()), n_det + nd
        if not (nd and nl):
            assert not g[key + '_ck'].any() and not g[key + '_cb'].any()
            continue
        oks = R.kpt_iou64(gk, pk, R.area_f32(lab), R.sigma_of(kpt_shape))
        assert np.abs(oks - g[key + '_oks64']).max() <= 1e-12 and np.abs(oks - g[key + '_oks']).max() <= d64 + 1e-12, key
        exc = g[key + '_exc']
        assert np.array_equal(exc, R.near_level(oks, lab[:, 0], det[:, 5])), key
        assert not (R.match(oks, lab[:, 0], det[:, 5]) != g[key + '_ck'])[~exc].any(), key
        assert np.array_equal(R.match(R.box_iou_f32(lab[:, 1:], det[:, :4]), lab[:, 0], det[:, 5]), g[key + '_cb']), key
    assert n_exc <= 0.02 * n_det


# ------------------------------------------------------------------------------------------------ GPU
_BATCH = {}


def _batch(name):
    """The images of a case in the kernel's batch layout (device tensors, built once per case and left unchanged) + the host inputs."""
    if name in _BATCH:
        return _BATCH[name]
    kpt_shape, imgs, keys = _native_images(name)
    nkpt, ndim = kpt_shape
    counts = [im[0].shape[0] for im in imgs]
    nl = [im[2].shape[0] for im in imgs]
    b, max_det, max_lab = len(imgs), max(max(counts), 1), max(max(nl), 1)
    rows = np.zeros((b, max_det, 6 + nkpt * ndim), np.float32)
    labels = np.zeros((b, max_lab, 5), np.float32)
    gk = np.zeros((b, max_lab, nkpt, 3), np.float32)
    for i, (det, pk, lab, g) in enumerate(imgs):
        rows[i, :counts[i], :6], rows[i, :counts[i], 6:] = det, pk.reshape(counts[i], nkpt * ndim)
        labels[i, :nl[i]], gk[i, :nl[i]] = lab, g
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rows_d, labels_d = t(rows), t(labels)
    c = dict(imgs=imgs, keys=keys, kpt_shape=kpt_shape, b=b, counts=counts, nl=nl, max_det=max_det, max_lab=max_lab, rows=rows_d, labels=labels_d,
             dense=rows_d[:, :, 6:].contiguous().view(b, max_det, nkpt, ndim), gk=t(gk), counts_dev=torch.tensor(counts, dtype=torch.int32).to(DEV),
             nlab=torch.tensor(nl, dtype=torch.int32).to(DEV), sigma=t(np.asarray(R.sigma_of(kpt_shape), np.float32)),
             area=((labels_d[:, :, 3] - labels_d[:, :, 1]) * (labels_d[:, :, 4] - labels_d[:, :, 2]) * 0.53).contiguous())
    _BATCH[name] = c
    return c


def _oks_guarded(c, pred):
    from mgdt_yolo_amd import ops
    n = c['b'] * c['max_lab'] * c['max_det']
    buf = torch.full((n + 128,), 7.5, dtype=torch.float32, device=DEV)
    out = ops.kpt_iou_batch(pred, c['counts_dev'], c['max_det'], c['gk'], c['area'], c['nlab'], c['sigma'], out=buf[64:64 + n])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:64] == 7.5).all() and (host[64 + n:] == 7.5).all(), 'guard values around the OKS block were overwritten'
    return out.view(c['b'], c['max_lab'], c['max_det']).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ALL_CASES)
def test_oks_matrix_is_within_the_derived_bound_of_float64(name):
    """The measured maximum is printed per case.  On an MI355X: 2.1e-8 (t1), 1.7e-7 (t2), 1.1e-7 (k5), 1.3e-7 (chain_pad, chain_gain)."""
    g = fixture()
    c = _batch(name)
    got = _oks_guarded(c, c['dense'])
    in_place = _oks_guarded(c, c['rows'])
    assert np.array_equal(got.view(np.uint32), in_place.view(np.uint32)), 'keypoints read in place from the NMS rows must give the dense result bit for bit'
    assert np.array_equal(c['area'].cpu().numpy()[0, :c['nl'][0]], R.area_f32(c['imgs'][0][2]))
    worst = 0.0
    for i, key in enumerate(c['keys']):
        nd, nl = c['counts'][i], c['nl'][i]
        assert not np.isnan(got[i]).any()
        if nd and nl:
            worst = max(worst, float(np.abs(got[i, :nl, :nd].astype(np.float64) - g[key + '_oks64']).max()))
        pad = got[i].copy()
        pad[:nl, :nd] = 0
        assert not pad.any(), 'entries past nlab / counts must be written as zero'
    print(f'{name}: max |device - fp64| {worst:.3e} (bound {bound(g, name):.3e}, reference fp32 vs fp64 {float(g[name + "_d64"]):.3e})')
    assert worst <= bound(g, name)
    if name == 't2':
        assert not got[0, 3, :].any() and not got[0, 5, :].any(), 'a label without a visible keypoint / with a zero-area box gives 0'


@pytest.mark.gpu
def test_zero_area_label_on_coincident_keypoints_contributes_one_and_no_nan():
    from mgdt_yolo_amd.yolo.utils.metrics import kpt_iou
    gk = torch.tensor([[[10., 20., 2.], [30., 40., 1.], [5., 5., 0.]]], device=DEV)
    pk = torch.tensor([[[10., 20.], [30., 41.], [9., 9.]], [[10., 20.], [30., 40.], [0., 0.]]], device=DEV)
    got = kpt_iou(gk, pk, torch.zeros(1, device=DEV), [0.1, 0.1, 0.1]).cpu().numpy()
    assert got.shape == (1, 2) and not np.isnan(got).any()
    assert got[0, 0] == np.float32(0.5) and got[0, 1] == np.float32(1.0)      # (1 + 0) / 2 and (1 + 1) / 2 visible keypoints


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['t1', 't2', 'k5'])
def test_metrics_kpt_iou_per_image_equals_the_batch_matrix(name):
    from mgdt_yolo_amd.yolo.utils.metrics import kpt_iou
    c = _batch(name)
    batch = _oks_guarded(c, c['dense'])
    for i, (det, pk, lab, gk) in enumerate(c['imgs']):
        nd, nl = c['counts'][i], c['nl'][i]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        got = kpt_iou(t(gk), t(pk), t(R.area_f32(lab)), R.sigma_of(c['kpt_shape'])).cpu().numpy()
        assert got.shape == (nl, nd) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(batch[i, :nl, :nd]).view(np.uint32)), (name, i)


def _check_correct(g, c, cb, ck, name):
    """Batch `correct` matrices against the fixture -> stats rows (device tensors), number of excepted detections."""
    stats, excepted = [], 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for i, key in enumerate(c['keys']):
        nd, nl = c['counts'][i], c['nl'][i]
        exc = g[key + '_exc']
        assert np.array_equal(cb[i, :nd], g[key + '_cb']), (key, 'boxes')
        diff = (ck[i, :nd] != g[key + '_ck']).any(1)
        assert not (diff & ~exc).any(), (key, 'keypoints: detections', np.nonzero(diff & ~exc)[0].tolist())
        assert not cb[i, nd:].any() and not ck[i, nd:].any(), 'rows past counts must be False'
        excepted += int(exc.sum())
        det, lab = c['imgs'][i][0], c['imgs'][i][2]
        if nd or nl:
            stats.append((t(cb[i, :nd]), t(ck[i, :nd]), t(det[:, 4]), t(det[:, 5]), t(lab[:, 0])))
    return stats, excepted


def _check_summary(g, v, name, excepted):
    s = v.get_stats()
    got = np.array([s[k] for k in KEYS])
    print(name, 'summary', got.tolist(), 'max |delta|', float(np.abs(got - g[name + '_summary']).max()), 'excepted', excepted)
    if excepted == 0:
        assert np.abs(got - g[name + '_summary']).max() <= 1e-6
    assert v.ap.shape == v.ap_pose.shape and len(v.ap_class_index) == v.ap.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ALL_CASES)
def test_correct_matrices_equal_the_reference_per_image_and_in_batch(name):
    from mgdt_yolo_amd.yolo.v8.pose import PoseValidator
    g = fixture()
    c = _batch(name)
    v = PoseValidator(device=DEV)
    v.init_metrics(nc=2, kpt_shape=c['kpt_shape'])
    cb, ck = v.match_batch(c['rows'], c['counts_dev'], c['dense'], c['labels'], c['nlab'], c['gk'])
    cb2, ck2 = v.match_batch(c['rows'], c['counts_dev'], c['rows'], c['labels'], c['nlab'], c['gk'])
    assert torch.equal(cb, cb2) and torch.equal(ck, ck2)
    cb, ck = cb.cpu().numpy(), ck.cpu().numpy()
    stats, excepted = _check_correct(g, c, cb, ck, name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for i, (det, pk, lab, gk) in enumerate(c['imgs']):
        nd = c['counts'][i]
        one_b = v._process_batch(t(det), t(lab)).cpu().numpy()
        one_k = v._process_batch(t(det), t(lab), t(pk), t(gk)).cpu().numpy()
        assert one_b.shape == (nd, 10) and np.array_equal(one_b, cb[i, :nd]) and np.array_equal(one_k, ck[i, :nd]), (name, i, 'per image != batch')
    v.stats = stats
    _check_summary(g, v, name, excepted)
    assert v.nt_per_class.sum() == sum(c['nl'])


@pytest.mark.gpu
@pytest.mark.parametrize('order', ['sorted', 'unsorted'])
@pytest.mark.parametrize('tag', list(R.CHAIN_BOXES))
def test_whole_chain_from_the_fixture_rows_through_update_metrics(tag, order):
    """update_metrics on a dataloader-style dict (normalised labels, ori_shape, ratio_pad) for the padded letter-box and for the one with gain != 1;
    batch_idx once in an unsorted order."""
    import pose_ref as PR
    from mgdt_yolo_amd.yolo.v8.pose import PoseValidator
    g = fixture()
    name = f'chain_{tag}'
    c = _batch(name)
    shape, rp = R.CHAIN_BOXES[tag]
    rows, batch = R.chain_inputs(PR.load_fixture())
    perm = np.arange(len(batch['batch_idx']))
    if order == 'unsorted':                   # the images interleaved, each image's labels in their own order
        perm = np.argsort(np.tile(np.arange(R.CHAIN_LABELS), 2), kind='stable')
        assert (np.diff(batch['batch_idx'][perm]) < 0).any()
    H, W = R.FRAME
    data = {k: torch.from_numpy(batch[k][perm]) for k in batch}
    data.update(img=torch.zeros(2, 3, H, W), ori_shape=[shape] * 2, ratio_pad=[rp] * 2)
    v = PoseValidator(device=DEV)
    v.init_metrics(nc=1, max_det=100)
    per = [torch.from_numpy(r).to(DEV) for r in rows]
    v.update_metrics(per, v.preprocess(data))
    assert v.seen == 2 and len(v.stats) == 2
    cb = np.stack([s[0].cpu().numpy() for s in v.stats])
    ck = np.stack([s[1].cpu().numpy() for s in v.stats])
    _, excepted = _check_correct(g, c, cb, ck, name)
    _check_summary(g, v, name, excepted)
    # images without detections / without labels
    v.init_metrics(nc=1, max_det=100)
    empty = dict(data, cls=data['cls'][:0], bboxes=data['bboxes'][:0], keypoints=data['keypoints'][:0], batch_idx=data['batch_idx'][:0])
    v.update_metrics(per, v.preprocess(empty))
    assert v.seen == 2 and len(v.stats) == 2 and not any(bool(s[1].any()) for s in v.stats) and v.stats[0][1].shape == (100, 10)
    v.update_metrics([per[0][:0], per[1]], v.preprocess(data))
    assert v.seen == 4 and len(v.stats) == 4 and v.stats[2][0].shape == (0, 10) and v.stats[2][4].numel() == R.CHAIN_LABELS


@pytest.mark.gpu
def test_match_batch_replays_in_a_captured_graph_equal_to_eager():
    from mgdt_yolo_amd.yolo.v8.pose import PoseValidator
    c = _batch('t2')
    v = PoseValidator(device=DEV)
    v.init_metrics(nc=2)
    v.iouv = v.iouv.to(DEV)
    v._sigma(torch.device(DEV))

    def step():
        return v.match_batch(c['rows'], c['counts_dev'], c['dense'], c['labels'], c['nlab'], c['gk'])
    eager = [x.clone() for x in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(3):
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, out))
    assert bool(eager[1].any())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_validator_on_the_models_own_predictions_matches_the_cpu_restatement(dt):
    """postprocess -> update_metrics -> get_stats on the seeded yolov8-pose n (2x96x160, validator settings) against a CPU pipeline built from
    tests/poseval_ref.py on the SAME GPU predictions (the model's parity is pinned by test_pose.py; this isolates the validator).  Labels: every
    other of an image's first detections with its keypoints jittered and its box moved by a few pixels, plus two that match nothing
    (poseval_ref.labels_from), handed over normalised.  Keypoint `correct`: equal outside detections with a same-class candidate within 1e-5 of a
    level; the eight numbers within 1e-3, as in test_map50_parity_with_the_cpu_reference_pipeline; the metric must be non-trivial (>= 5 true
    positives at 0.5, fewer at 0.95, boxes and keypoints).  bf16: the same run with the figures printed and no bound asserted."""
    strict = dt == torch.float32
    import pose_ref as PR
    from mgdt_yolo_amd.models import get_config
    from mgdt_yolo_amd.nn.tasks import PoseModel
    from mgdt_yolo_amd.seeding import seeded_images
    from mgdt_yolo_amd.yolo.v8.pose import PoseValidator
    from oracle import metrics as OM
    H, W = 96, 160
    m = PoseModel(get_config('yolov8-pose', 'n'), data_kpt_shape=(17, 3), verbose=False)
    PR.seed_pose_(m, 0)
    m = m.eval().set_compute_dtype(dt).to(DEV)
    x = seeded_images(2, H, W, seed=PR.IMG_SEED).to(DEV).to(dt)
    with torch.no_grad():
        preds = m(x)
    v = PoseValidator(device=DEV)
    v.init_metrics(nc=1, conf=0.001, iou=0.7, max_det=100)
    per = v.postprocess(preds)
    counts = [int(p.shape[0]) for p in per]
    assert min(counts) > 30 or not strict
    rows = [p.cpu().numpy() for p in per]
    labs = [R.labels_from(np.random.default_rng([17, i]), rows[i][:, :6], rows[i][:, 6:].reshape(-1, 17, 3), 14, 1, False, frame=(H, W)) for i in range(2)]
    cls = np.concatenate([l[:, 0:1] for l, _ in labs])
    box = np.concatenate([np.stack([(l[:, 1] + l[:, 3]) / 2 / W, (l[:, 2] + l[:, 4]) / 2 / H, (l[:, 3] - l[:, 1]) / W, (l[:, 4] - l[:, 2]) / H], 1) for l, _ in labs])
    kp = np.concatenate([k / np.array([W, H, 1], np.float32) for _, k in labs]).astype(np.float32)
    bidx = np.repeat(np.arange(2, dtype=np.float32), 14)
    rp = ((1.0, 1.0), (0.0, 0.0))
    batch = dict(img=x, cls=torch.from_numpy(cls), bboxes=torch.from_numpy(box.astype(np.float32)), keypoints=torch.from_numpy(kp),
                 batch_idx=torch.from_numpy(bidx), ori_shape=[(H, W)] * 2, ratio_pad=[rp] * 2)
    v.update_metrics(per, v.preprocess(batch))
    assert v.seen == 2 and len(v.stats) == 2
    got = v.get_stats()
    # ---- the same on the CPU
    stats = []
    for i in range(2):
        sel = bidx == i
        lab, tk = R.native_labels((H, W), cls[sel], box[sel].astype(np.float32), kp[sel], (H, W), rp)
        predn = R.scale_boxes_f32((H, W), rows[i], (H, W), rp)
        pk = R.scale_coords_f32((H, W), rows[i][:, 6:].reshape(-1, 17, 3), (H, W), rp)
        dcls = rows[i][:, 5]
        oks = R.kpt_iou64(tk, pk, R.area_f32(lab), R.OKS_SIGMA)
        cb = R.match(R.box_iou_f32(lab[:, 1:], predn), lab[:, 0], dcls)
        ck = R.match(oks, lab[:, 0], dcls)
        near = R.near_level(oks, lab[:, 0], dcls)
        dev_cb, dev_ck = v.stats[i][0].cpu().numpy(), v.stats[i][1].cpu().numpy()
        diff = (ck != dev_ck).any(1)
        print(f'image {i}: {counts[i]} detections, {int(sel.sum())} labels, tp boxes {cb.sum(0).tolist()} keypoints {ck.sum(0).tolist()}, near a level '
              f'{int(near.sum())}, detections differing from the device: boxes {int((cb != dev_cb).any(1).sum())} keypoints {np.nonzero(diff)[0].tolist()}')
        assert not (diff & ~near).any() or not strict
        stats.append((cb, ck, rows[i][:, 4], dcls, lab[:, 0]))
    cb, ck, conf, pcls, tcls = [np.concatenate(a, 0) for a in zip(*stats)]
    if strict:
        for c in (cb, ck):
            assert c[:, 0].sum() >= 5 and c[:, 9].sum() < c[:, 0].sum(), 'the metric must be non-trivial'
    want = []
    for tp in (cb, ck):
        if tp.any():
            _, _, p, rr, _, ap, _ = OM.ap_per_class(tp, conf, pcls, tcls)
            want += [p.mean(), rr.mean(), ap[:, 0].mean(), ap.mean()]
        else:
            want += [0.0] * 4
    gg = np.array([got[k] for k in KEYS])
    print('device', gg.tolist())
    print('cpu   ', [float(w) for w in want])
    print(f'{dt}: max |device - cpu| over the eight numbers {float(np.abs(gg - np.array(want)).max()):.3e}')
    assert np.abs(gg - np.array(want)).max() <= 1e-3 or not strict
