"""Training augmentation on the device (csrc/augment.hip, yolo/data/augment.py ImagePool / TrainAugment).

Pinned to the reference (tests/golden/aug_NN.npz, recorded from its own v8_transforms + Format by tests/golden/gen_aug.py): the order of the random
draws and every parameter they give, the pixels of the mosaic / letter-box canvas, the surviving boxes and their order.  Pinned to the float64
restatement tests/aug_ref.py only: the rounding of the bilinear warp and the 8-bit BGR <-> HSV conversions (cv2 is not installed; its fixed-point
warp and colour tables may differ by one level)."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import aug_ref as AR
from mgdt_yolo_amd import _lib
from mgdt_yolo_amd import ops as hip
from mgdt_yolo_amd.yolo.data.augment import AugParams, ImagePool, TrainAugment, fill_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
OK, BAD_SHAPE, BAD_ARG = 0, -1, -4
_POOLS = {}


def pool_data(S):
    if S not in _POOLS:
        _POOLS[S] = AR.make_pool(S)
    return _POOLS[S]


def shapes_of(S):
    return [im.shape[:2] for im in pool_data(S)[0]]


def fixture_rects(g, b):
    S, shapes = int(g['S']), shapes_of(int(g['S']))
    if g['mosaic'][b]:
        ids = g['mix'][b].tolist()
        return AR.mosaic_rects(S, int(g['yc'][b]), int(g['xc'][b]), ids, [shapes[i] for i in ids])
    i = int(g['mix'][b, 0])
    return AR.letterbox_rect(S, i, shapes[i])


def sampled(case, device=None):
    """TrainAugment of the case on the shared pool + the parameters it draws from the case's seeds."""
    images, labels = pool_data(case['S'])
    aug = TrainAugment(ImagePool(images, labels, case['S'], device=device), hyp=case['hyp'], max_labels=32)
    random.seed(case['seed'])
    np.random.seed(case['seed'])
    return aug, aug.sample(AR.INDICES)


def explicit(items, luts=None):
    """AugParams from plain values: items = [dict(rects, pads, canvas, M, s, flipud, fliplr, mosaic)]; luts (B, 3, 256) or None (no HSV step)."""
    P = AugParams(len(items))
    for b, it in enumerate(items):
        if luts is not None:
            P.luts[b] = luts[b]
        fill_record(P.records[b], it['rects'], it['pads'], it['canvas'], it['M'], it.get('s', 1.0), it.get('flipud', False), it.get('fliplr', False),
                    it.get('mosaic', False), -1 if luts is None else b * 768)
    return P


def hwc_bgr(img):
    """(3, S, S) RGB planes of the device -> (S, S, 3) BGR numpy."""
    return img.permute(1, 2, 0).flip(-1).cpu().numpy()


# ============================================================================================================================== CPU
@pytest.mark.parametrize('case', AR.CASES, ids=[c['name'] for c in AR.CASES])
def test_restatement_reproduces_the_reference(case, golden):
    g = golden(case['name'])
    S = case['S']
    images, labels = pool_data(S)
    assert int(g['seed']) == case['seed'] and json.loads(str(g['hyp']))['mosaic'] == case['hyp'].get('mosaic', 1.0)
    for b in range(len(AR.INDICES)):
        rects, pads = fixture_rects(g, b)
        size = 2 * S if g['mosaic'][b] else S
        assert np.array_equal(AR.canvas(images, rects, size), g['canvas'][b]), (case['name'], b)
        r = AR.boxes(labels, shapes_of(S), rects, pads, size, g['M'][b], float(g['s'][b]), S, bool(g['mosaic'][b]), bool(g['flipud'][b]), bool(g['fliplr'][b]))
        n = int(g['n'][b])
        assert len(r['cls']) == n and np.array_equal(r['cls'], g['cls'][b, :n])
        assert r['margin'] >= AR.MARGIN
        if n:
            assert np.abs(r['xywh'] * S - g['bboxes'][b, :n].astype(np.float64) * S).max() <= 1e-4


@pytest.mark.parametrize('case', AR.CASES, ids=[c['name'] for c in AR.CASES])
def test_sample_reproduces_every_recorded_parameter(case, golden):
    g = golden(case['name'])
    aug, P = sampled(case)
    assert random.random() == float(g['next_random'])
    assert np.array_equal(P.mosaic, g['mosaic']) and np.array_equal(P.indices, g['mix'])
    assert np.array_equal(P.yc, g['yc']) and np.array_equal(P.xc, g['xc'])
    assert P.M.dtype == np.float32 and P.M.tobytes() == g['M'].tobytes()
    assert np.array_equal(P.scale, g['s'])
    assert np.array_equal(P.luts, g['luts'])
    assert np.array_equal(P.flipud, g['flipud']) and np.array_equal(P.fliplr, g['fliplr'])
    for b in range(len(P)):
        rects, pads = fixture_rects(g, b)
        rec = P.records[b]
        assert rec['nrect'] == len(rects) and rec['canvas'] == g['canvas'][b].shape[0] and rec['lut'] == b * 768
        assert rec['flags'] == int(g['flipud'][b]) | int(g['fliplr'][b]) << 1 | int(g['mosaic'][b]) << 2
        assert rec['rect'][:len(rects)].tolist() == [list(r) for r in rects]
        assert rec['pad'][:len(rects)].tolist() == [list(map(float, p)) for p in pads]
        assert rec['inv'].tobytes() == AR.inverse6(g['M'][b]).tobytes() and rec['m'].tobytes() == g['M'][b][:2].tobytes()
        assert rec['scale'] == np.float32(g['s'][b])


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'mgdt.h')).read()
    lib = _lib.lib()
    for name in ('mgdt_aug_check', 'mgdt_aug_warp_fwd', 'mgdt_aug_labels_fwd'):
        assert re.search(r'\bint ' + name + r'\(', hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert 'mgdt_aug_record' in hdr and 'mgdt_aug_image' in hdr
    assert hip.AUG_RECORD.itemsize == 224 and hip.AUG_IMAGE.itemsize == 24


def test_bad_arguments_are_refused_without_a_gpu():
    """Every refusal comes from the host wrapper before any launch: the device pointers below are never dereferenced."""
    lib = _lib.lib()
    aug, P = sampled(AR.CASES[0])
    tab, B, S = aug.pool.table, len(P), 64
    dev = C.c_void_p(0x10000)
    hp = lambda a: C.c_void_p(a.ctypes.data)

    def check(rec=P.records, images=tab, batch=B, pool_bytes=aug.pool.pool_bytes, n_labels=aug.pool.n_labels, lut_bytes=B * 768, imgsz=S):
        return lib.mgdt_aug_check(None if rec is None else hp(rec), batch, None if images is None else hp(images), len(tab), pool_bytes, n_labels, lut_bytes, imgsz)

    def warp(rec=P.records, pool=dev, images_dev=dev, rec_dev=dev, luts=dev, out=dev, batch=B, imgsz=S):
        return lib.mgdt_aug_warp_fwd(pool, aug.pool.pool_bytes, images_dev, hp(tab), len(tab), rec_dev, None if rec is None else hp(rec), luts, B * 768, batch,
                                     imgsz, out, None)

    def labels(rec=P.records, rec_dev=dev, gt=dev, cap=16, batch=B, nl=dev):
        return lib.mgdt_aug_labels_fwd(dev, aug.pool.n_labels, dev, hp(tab), len(tab), rec_dev, None if rec is None else hp(rec), batch, S, cap, gt, dev, nl, dev, None)

    def changed(**kw):
        r = P.records.copy()
        for k, v in kw.items():
            r[k][1] = v
        return r

    assert check() == OK
    assert check(rec=None) == BAD_ARG and check(images=None) == BAD_ARG
    assert b'null' in lib.mgdt_last_error()
    assert check(batch=0) == BAD_SHAPE and check(imgsz=62) == BAD_SHAPE and check(imgsz=0) == BAD_SHAPE
    assert check(pool_bytes=aug.pool.pool_bytes - 1) == BAD_SHAPE                      # the last image ends outside the pool
    assert check(n_labels=aug.pool.n_labels - 1) == BAD_SHAPE
    assert check(rec=changed(nrect=5)) == BAD_SHAPE and check(rec=changed(canvas=4 * S)) == BAD_SHAPE and check(rec=changed(flags=8)) == BAD_SHAPE
    assert check(rec=changed(lut=B * 768)) == BAD_ARG and check(rec=changed(lut=2)) == BAD_ARG and check(lut_bytes=0) == BAD_ARG
    for bad in (-1, len(tab)):
        r = P.records.copy()
        r['rect'][2, 1, 0] = bad
        assert check(rec=r) == BAD_ARG                                                    # source id outside the pool
        assert warp(rec=r) == BAD_ARG and labels(rec=r) == BAD_ARG
    assert b'source id' in lib.mgdt_last_error()
    r = P.records.copy()
    r['rect'][0, 0, 5] += 1                                                               # one column more than the source image has
    assert check(rec=r) == BAD_SHAPE
    r = P.records.copy()
    r['inv'][3, 2] = np.nan
    assert check(rec=r) == BAD_ARG
    for kw in (dict(pool=None), dict(images_dev=None), dict(rec_dev=None), dict(rec=None), dict(out=None), dict(luts=None),
               dict(rec_dev=C.c_void_p(0x10004)), dict(images_dev=C.c_void_p(0x10004)), dict(out=C.c_void_p(0x10001)), dict(luts=C.c_void_p(0x10002))):
        assert warp(**kw) == BAD_ARG, kw
    assert warp(batch=0) == BAD_SHAPE and warp(imgsz=66) == BAD_SHAPE
    for kw in (dict(rec_dev=None), dict(rec=None), dict(gt=None), dict(nl=None), dict(rec_dev=C.c_void_p(0x10004)), dict(gt=C.c_void_p(0x10002))):
        assert labels(**kw) == BAD_ARG, kw
    assert labels(cap=20) == BAD_SHAPE and labels(cap=0) == BAD_SHAPE and labels(batch=70000) == BAD_SHAPE


def test_unsupported_requests_raise():
    images, labels = pool_data(64)
    pool = ImagePool(images, labels, 64, device=None)
    for hyp in (dict(mixup=0.1), dict(copy_paste=0.5), dict(perspective=0.0005), dict(mosaic_n=9), dict(segments=True), dict(keypoints=True),
                dict(albumentations=True)):
        with pytest.raises(NotImplementedError):
            TrainAugment(pool, hyp=hyp)
    with pytest.raises(ValueError, match='long side'):
        ImagePool([np.zeros((40, 50, 3), np.uint8)], [np.zeros((0, 5), np.float32)], 64, device=None)
    with pytest.raises(ValueError, match='boxes only'):
        ImagePool([np.zeros((64, 50, 3), np.uint8)], [np.zeros((2, 39), np.float32)], 64, device=None)
    with pytest.raises(ValueError):
        TrainAugment(pool, imgsz=96)
    with pytest.raises(ValueError):
        TrainAugment(pool).sample([8])
    assert TrainAugment(pool).hyp['fliplr'] == 0.0 and TrainAugment(pool).hyp['mosaic'] == 1.0


# ============================================================================================================================== GPU
def shift(tx, ty):
    """Scale 1 and an integral translation: output (x, y) is canvas (x + tx, y + ty)."""
    M = np.eye(3, dtype=np.float32)
    M[0, 2], M[1, 2] = -tx, -ty
    return M


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['aug_00', 'aug_01', 'aug_04'])
def test_placement_is_exact(name, golden):
    """M a pure integer shift: the output is the crop of the canvas, channel order reversed.  The canvases are the reference's recorded ones; the
    mosaic cases add centres at both ends of [S/2, 3S/2) (restated canvas, equal to the reference's rule by the CPU test above)."""
    g = golden(name)
    S = int(g['S'])
    images, labels = pool_data(S)
    aug = TrainAugment(ImagePool(images, labels, S, DEV), max_labels=32)
    items, want = [], []
    offs = [(0, 0), (S, S), (S // 2, S // 2), (S // 4 + 1, S - 3), (S - 1, 7)] if name != 'aug_04' else [(0, 0)] * 5
    for b, (tx, ty) in enumerate(offs):
        rects, pads = fixture_rects(g, b)
        cv = g['canvas'][b]
        items.append(dict(rects=rects, pads=pads, canvas=cv.shape[0], M=shift(tx, ty), mosaic=bool(g['mosaic'][b])))
        want.append(cv[ty:ty + S, tx:tx + S])
    if name != 'aug_04':
        shapes = shapes_of(S)
        for (yc, xc), ids, (tx, ty) in (((S // 2, S // 2), [3, 0, 1, 7], (0, 0)), ((3 * S // 2 - 1, 3 * S // 2 - 1), [3, 7, 1, 0], (S, S)),
                                        ((S // 2, 3 * S // 2 - 1), [0, 1, 2, 3], (S // 2, 0)), ((S, S), [3, 7, 3, 7], (S // 2, S // 2))):
            rects, pads = AR.mosaic_rects(S, yc, xc, ids, [shapes[i] for i in ids])
            items.append(dict(rects=rects, pads=pads, canvas=2 * S, M=shift(tx, ty), mosaic=True))
            want.append(AR.canvas(images, rects, 2 * S)[ty:ty + S, tx:tx + S])
    out = aug.apply(explicit(items))['img']
    assert out.shape == (len(items), 3, S, S) and out.dtype == torch.uint8 and out.is_contiguous()
    gaps = 0
    for b, w in enumerate(want):
        assert np.array_equal(hwc_bgr(out[b]), w), (name, b)
        gaps += int((w == 114).all(-1).sum() > S)
    assert gaps >= 1, 'no case left a 114 gap'


def _affine(S, canvas, angle, scale, shear, tx, ty):
    from mgdt_yolo_amd.yolo.data.augment import rotation_matrix_2d
    Cm, R, Sh, T = (np.eye(3, dtype=np.float32) for _ in range(4))
    Cm[0, 2] = Cm[1, 2] = -canvas / 2
    R[:2] = rotation_matrix_2d(angle, scale)
    Sh[0, 1], Sh[1, 0] = np.tan(np.deg2rad(shear)), np.tan(np.deg2rad(-shear / 2))
    T[0, 2], T[1, 2] = tx * S, ty * S
    return T @ Sh @ R @ Cm


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['aug_00', 'aug_01', 'aug_02', 'aug_03', 'aug_05'])
def test_warp_is_the_rounded_bilinear_value(name, golden):
    """Recorded parameters (and three explicit ones: scale 0.5, 1.5 with rotation and shear, and scale 1 with a half-pixel shift), no HSV step (the
    reference skips it when every gain is 0: 'identity tables' through the 8-bit colour round trip would not be an identity).
    |out - v| <= 0.5 + delta: v the float64 bilinear value from the same six float32 words, delta what moving the source point by 4 float32 ulp of the
    largest source coordinate changes in v, both from tests/aug_ref.py alone; 1e-9 is the float64 rounding of v itself."""
    g = golden(name)
    S = int(g['S'])
    images, labels = pool_data(S)
    aug = TrainAugment(ImagePool(images, labels, S, DEV), max_labels=32)
    items = []
    for b in range(len(AR.INDICES)):
        rects, pads = fixture_rects(g, b)
        items.append(dict(rects=rects, pads=pads, canvas=g['canvas'][b].shape[0], M=g['M'][b], s=float(g['s'][b]), mosaic=bool(g['mosaic'][b])))
    cvs = [g['canvas'][b] for b in range(len(items))]
    for k, (angle, scale, shear, tx, ty) in enumerate(((10.0, 0.5, 5.0, 0.45, 0.55), (-7.0, 1.5, -5.0, 0.58, 0.41), (0.0, 1.0, 0.0, 0.5 + 0.5 / S, 0.5 + 1.5 / S))):
        items.append(dict(items[k], M=_affine(S, cvs[k].shape[0], angle, scale, shear, tx, ty), s=scale))
        cvs.append(cvs[k])
    out = aug.apply(explicit(items))['img']
    for b, it in enumerate(items):
        inv6 = AR.inverse6(it['M'])
        v, delta = AR.warp(cvs[b], inv6, S), AR.warp_delta(cvs[b], inv6, S)
        err = np.abs(hwc_bgr(out[b]).astype(np.float64) - v)
        print(f'{name}[{b}]: max |out - v| {err.max():.6f}, max delta {delta.max():.2e}, worst excess {(err - 0.5 - delta).max():.2e}')
        assert (err <= 0.5 + delta + 1e-9).all(), (name, b, float((err - 0.5 - delta).max()))
        assert (hwc_bgr(out[b]) != 114).any()


def _hsv_images(S, luts, rng):
    """Gray pixels, pure primaries and secondaries at several levels, the hue wrap on both sides of 179 / 0, random pixels elsewhere.  The inputs are
    chosen so that few pixels sit on a rounding boundary of the restatement (with clipped tables V = S = 255 is common, and 255 f / 30 is a half
    for every odd f): a random pixel that does is drawn again, a constructed one is taken from the same construction at a lower top level."""
    def constructed(top):
        blk = np.zeros((10, S, 3), np.int64)
        ramp = np.arange(S) * top // (S - 1)
        blk[0] = ramp[:, None]                                                    # grays: S = 0
        for k, c in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1))):
            blk[1 + k] = ramp[:, None] * np.array(c)
        blk[7, :, 2], blk[7, :, 1], blk[7, :, 0] = top, 0, np.arange(S) % 16      # R = max, G < B: H / 2 just below 180
        blk[8, :, 2], blk[8, :, 1], blk[8, :, 0] = top, np.arange(S) % 16, 0      # ... and just above 0
        blk[9, :, 2], blk[9, :, 1], blk[9, :, 0] = top - top // 5, top * 2 // 5 + np.arange(S) % 3, top * 2 // 5 + 1      # G - B in {-1, 0, 1} around the wrap, low saturation
        return blk.astype(np.uint8)
    im = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    im[:10] = constructed(255)
    for top in (254, 240, 222, 200, 190, 170, 150, 131, 120, 101, 88, 64):
        near = AR.hsv(im, luts)[1]
        rest = near.copy()
        rest[:10] = False
        im[rest] = rng.integers(0, 256, (int(rest.sum()), 3), dtype=np.uint8)
        im[:10][near[:10]] = constructed(top)[near[:10]]
    im[10, :8] = constructed(255)[7, 1:9]                                         # a few pixels that DO sit on a boundary where the tables clip (the one-level rule is exercised)
    return im


@pytest.mark.gpu
def test_hsv_equals_the_exact_evaluation(golden):
    """Identity warp, tables: recorded ones and the extreme gains (1 +- 0.015, 1 +- 0.7, 1 +- 0.4).  The output equals the restatement except where one
    of its pre-rounding values (H / 2, S, an output channel) lies within 1e-3 of a rounding boundary: there the value may move by one level."""
    S = 64
    x = np.arange(0, 256, dtype=np.float64)
    tables = [golden('aug_00')['luts'][0], golden('aug_02')['luts'][3]]
    for r in ((1.015, 1.7, 1.4), (0.985, 0.3, 0.6)):
        tables.append(np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)]))
    rng = np.random.default_rng(5)
    images = [_hsv_images(S, t, rng) for t in tables]
    aug = TrainAugment(ImagePool(images, [np.zeros((0, 5), np.float32)] * len(images), S, DEV))
    items = [dict(rects=[(i, 0, 0, S, S, 0, 0)], pads=[(0.0, 0.0)], canvas=S, M=np.eye(3, dtype=np.float32)) for i in range(len(images))]
    out = aug.apply(explicit(items, np.stack(tables)))['img']
    for i, (im, t) in enumerate(zip(images, tables)):
        want, near = AR.hsv(im, t)
        got = hwc_bgr(out[i])
        bad = (got != want).any(-1)
        print(f'hsv[{i}]: {int(near.sum())} of {S * S} pixels near a rounding boundary, {int(bad.sum())} differ from the restatement')
        assert near.mean() < 0.01, (i, float(near.mean()))
        assert not (bad & ~near).any(), (i, np.argwhere(bad & ~near)[:5].tolist())
        for y, xx in np.argwhere(bad):                                           # on a boundary: some one-level move of H / 2, S or a channel explains it
            px = im[y:y + 1, xx:xx + 1]
            ok = any((np.abs(AR.hsv(px, t, dh=dh, ds=ds)[0].astype(int) - got[y, xx].astype(int)) <= 1).all() for dh in (-1, 0, 1) for ds in (-1, 0, 1))
            assert ok, (i, y, xx, im[y, xx].tolist(), got[y, xx].tolist(), want[y, xx].tolist())
        assert (want != im).any()


@pytest.mark.gpu
def test_flips_mirror_pixels_and_labels(golden):
    g = golden('aug_02')
    aug, P = sampled(AR.CASES[2], DEV)
    runs = {}
    for ud in (False, True):
        for lr in (False, True):
            Q = AugParams(len(P))
            Q.records[:], Q.luts[:] = P.records, P.luts
            Q.records['flags'] = (P.records['flags'] & 4) | int(ud) | int(lr) << 1
            o = aug.apply(Q)
            runs[ud, lr] = {k: v.clone() for k, v in o.items()}
    base = runs[False, False]
    S = 64
    for (ud, lr), o in runs.items():
        dims = [d for d, f in ((2, ud), (3, lr)) if f]
        assert torch.equal(o['img'], base['img'].flip(dims) if dims else base['img']), (ud, lr)
        assert torch.equal(o['nlabels'], base['nlabels']) and int(o['nlabels'].sum()) > 0
        want = base['labels'].clone()
        live = torch.arange(want.shape[1], device=DEV)[None, :] < base['nlabels'][:, None]
        if ud:
            want[..., 2] = torch.where(live, 1 - want[..., 2], want[..., 2])
        if lr:
            want[..., 1] = torch.where(live, 1 - want[..., 1], want[..., 1])
        assert torch.equal(o['labels'][..., [0, 3, 4]], want[..., [0, 3, 4]])
        assert (o['labels'] - want).abs().max().item() <= 2.0 ** -22          # 1 - x and the round trip through pixels: a few ulp of 1
        wg = base['gt'].clone()
        if ud:
            wg[..., 2], wg[..., 4] = torch.where(live, S - base['gt'][..., 4], wg[..., 2]), torch.where(live, S - base['gt'][..., 2], wg[..., 4])
        if lr:
            wg[..., 1], wg[..., 3] = torch.where(live, S - base['gt'][..., 3], wg[..., 1]), torch.where(live, S - base['gt'][..., 1], wg[..., 3])
        assert (o['gt'] - wg).abs().max().item() <= S * 2.0 ** -21


@pytest.mark.gpu
@pytest.mark.parametrize('case', AR.CASES, ids=[c['name'] for c in AR.CASES])
def test_labels_equal_the_reference(case, golden):
    g = golden(case['name'])
    S = case['S']
    aug, P = sampled(case, DEV)
    o = aug.apply(P)
    n = o['nlabels'].cpu().numpy()
    assert np.array_equal(n, g['n']) and not o['flags'].any().item()
    lab, gt = o['labels'].cpu().numpy(), o['gt'].cpu().numpy()
    for b in range(len(n)):
        k = int(n[b])
        assert np.array_equal(lab[b, :k, 0], g['cls'][b, :k]) and np.array_equal(gt[b, :k, 0], g['cls'][b, :k])
        assert not lab[b, k:].any() and not gt[b, k:].any()
        if k:
            ref = g['bboxes'][b, :k].astype(np.float64)
            px = ref * S
            xyxy = np.concatenate([px[:, :2] - px[:, 2:] / 2, px[:, :2] + px[:, 2:] / 2], 1)
            el, eg = np.abs(lab[b, :k, 1:] - ref).max(), np.abs(gt[b, :k, 1:] - xyxy).max()
            print(f"{case['name']}[{b}]: {k} boxes, labels err {el:.2e}, gt err {eg:.2e} px")
            assert el <= 1e-3 / S and eg <= 1e-3
    d = aug.to_dict(o)
    assert d['img'] is o['img'] and d['bboxes'].shape == (int(n.sum()), 4) and d['cls'].shape == (int(n.sum()), 1)
    assert np.array_equal(d['batch_idx'].numpy(), np.repeat(np.arange(len(n)), n).astype(np.float32))


@pytest.mark.gpu
def test_label_edge_cases():
    S = 64
    rng = np.random.default_rng(11)
    many = np.concatenate([rng.integers(0, 5, (30, 1)), rng.uniform(0.3, 0.7, (30, 2)), rng.uniform(0.1, 0.3, (30, 2))], 1).astype(np.float32)
    few = many[:3].copy()
    images = [rng.integers(0, 256, (S, S, 3), dtype=np.uint8) for _ in range(3)]
    pool = ImagePool(images, [few, many, np.zeros((0, 5), np.float32)], S, DEV)
    eye = np.eye(3, dtype=np.float32)
    tiny = np.diag([0.02, 0.02, 1.0]).astype(np.float32)
    one = lambda i, M, s=1.0: dict(rects=[(i, 0, 0, S, S, 0, 0)], pads=[(0.0, 0.0)], canvas=S, M=M, s=s)
    P = explicit([one(0, eye), one(1, eye), one(2, eye), one(1, tiny, 0.02)])
    big = TrainAugment(pool, max_labels=32).apply(P)
    assert big['nlabels'].tolist() == [3, 30, 0, 0] and big['flags'].tolist() == [0, 0, 0, 0]      # no labels; every label filtered (boxes under 2 px)
    assert not big['labels'][2:].any().item() and not big['gt'][2:].any().item()
    assert torch.equal(big['labels'][1, :30, 0].cpu(), torch.from_numpy(many[:, 0]))
    aug = TrainAugment(pool, max_labels=16)
    small = aug.apply(P)
    assert small['labels'].shape == (4, 16, 5)
    assert small['nlabels'].tolist() == [3, 16, 0, 0] and small['flags'].tolist() == [0, 1, 0, 0]
    assert torch.equal(small['labels'], big['labels'][:, :16]) and torch.equal(small['gt'], big['gt'][:, :16])
    assert torch.equal(small['img'], big['img'])
    with pytest.raises(RuntimeError, match='max_labels'):
        aug.to_dict(small)


@pytest.mark.gpu
def test_batching_and_capture():
    """Image i alone equals image i of the batch; a captured apply replayed with new records equals the eager call bit for bit (a host read inside
    apply would have failed the capture)."""
    aug, P = sampled(AR.CASES[3], DEV)
    full = {k: v.clone() for k, v in aug.apply(P).items()}
    solo = TrainAugment(aug.pool, hyp=AR.CASES[3]['hyp'], max_labels=32)
    for i in range(len(P)):
        Q = AugParams(1)
        Q.records[0], Q.luts[0] = P.records[i], P.luts[i]
        Q.records['lut'] = 0
        o = solo.apply(Q)
        for k in full:
            assert torch.equal(o[k][0], full[k][i]), (i, k)
    random.seed(77)
    np.random.seed(77)
    P2 = aug.sample((7, 2, 4, 0, 3))
    want = {k: v.clone() for k, v in aug.apply(P2).items()}
    assert not torch.equal(want['img'], full['img'])
    aug.apply(P)                                           # buffers exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = aug.apply(P)
    aug.load(P2)
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(o[k], want[k]), k
    aug.load(P)
    graph.replay()
    for k in full:
        assert torch.equal(o[k], full[k]), k


def _train_batch(S=160, B=2):
    images, labels = AR.make_pool(S)
    aug = TrainAugment(ImagePool(images, labels, S, DEV), max_labels=48)
    random.seed(5)                                       # 6 and 20 boxes: the host dict needs 32 label slots, the device batch brings its 48
    np.random.seed(5)
    batch = aug((0, 1)[:B])
    host = aug.to_dict(batch)
    assert batch['nlabels'].tolist() == [6, 20]
    return batch, host


def _model(nc=8):                                      # the pool has classes 0..4; the bf16 reverse pass of the head wants nc % 4 == 0
    from mgdt_yolo_amd.models import get_config
    from mgdt_yolo_amd.nn.tasks import DetectionModel
    from mgdt_yolo_amd.seeding import seed_state_dict_
    return seed_state_dict_(DetectionModel(get_config('mspa_c2f_gd_yolov8', 'n', nc), verbose=False), 0).to(DEV)


@pytest.mark.gpu
def test_loss_through_the_dense_labels_equals_the_host_dict():
    from mgdt_yolo_amd.yolo.utils.loss import loss_and_head_grads, v8DetectionLoss
    batch, host = _train_batch()
    assert 'gt' in batch and 'gt' not in host and batch['gt'].shape[1] == 48
    m = _model().train()
    feats = m._predict_once(batch['img'])
    t0, i0, g0 = loss_and_head_grads(v8DetectionLoss(m), feats, batch)
    t1, i1, g1 = loss_and_head_grads(v8DetectionLoss(m), feats, host)
    assert torch.isfinite(t0).item() and t0.item() > 0
    assert torch.equal(t0, t1) and torch.equal(i0, i1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    c0, c1 = v8DetectionLoss(m), v8DetectionLoss(m)
    (l0, it0), (l1, it1) = c0(feats, batch), c1(feats, host)
    assert torch.equal(l0, l1) and torch.equal(it0, it1) and torch.equal(l0, t0)


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('amp', [False, True], ids=['f32', 'bf16'])
def test_trainer_step_on_the_device_batch_equals_the_host_dict(amp, graph):
    """graph=True: the captured step starts with the second optimizer step, so three steps run; with batch['gt'] the label slots are gt.shape[1]."""
    from mgdt_yolo_amd.yolo.engine.trainer import DetectionTrainer
    batch, host = _train_batch()
    res = []
    for b in (batch, host):
        tr = DetectionTrainer(_model(), lr0=0.01, amp=amp, graph=graph)
        losses = [tr.step(b)[0].item() for _ in range(3 if graph else 1)]
        if graph and b is batch:
            assert sorted(tr._graphs) == [48]
        res.append((losses, tr.state.data.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
