"""RTDETRValidator: mgdt_rtdetr_val_post_fwd and the validator against the reference's recorded outputs (case i of tests/golden/rtdetr_loss_NN.npz:
RTDETRValidator.postprocess / update_metrics and DetectionValidator.get_stats run by tests/golden/gen_rtdetr_loss.py).  The recorded confidences are
pairwise distinct (asserted by the generator), so the row order is comparable; ties are checked on a constructed input."""
import os

import numpy as np
import pytest
import torch

import rtdetr_loss_ref as LR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
DEV = 'cuda:0'
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return LR.load_fixtures(GOLDEN)


# ================================================================================================================ CPU
def test_row_order_restatement_reproduces_the_fixture(fx):
    for si, im in enumerate(LR.make_val_inputs()):
        for k in ('boxes', 'scores', 'labels'):
            assert LR.checksum(im[k]) == float(fx[f'i_sum_{k}_{si}']), k
        rows = LR.val_rows(torch.from_numpy(im['boxes']), torch.from_numpy(im['scores'])).numpy()
        want = fx[f'i_rows_{si}']
        assert rows.shape == want.shape == (LR.VAL['nq'][si], 6)
        assert np.array_equal(rows[:, 4:], want[:, 4:]) and np.abs(rows[:, :4] - want[:, :4]).max() <= 1e-6
        assert len(np.unique(want[:, 4])) == len(want) and (np.diff(want[:, 4]) < 0).all()
    t = torch.tensor([[0.2, 0.7], [0.7, 0.1], [0.7, 0.7], [0.9, 0.0]])
    tied = LR.val_rows(torch.arange(16.0).reshape(4, 4), t)
    assert tied[:, 5].tolist() == [0.0, 1.0, 0.0, 0.0] and tied[:, 0].tolist() == [12 - 7, 0 - 1, 4 - 3, 8 - 5], 'the tie in query order'


def test_refusals():
    from mgdt_yolo_amd.vit.rtdetr import RTDETRValidator
    for k in ('single_cls', 'save_json', 'save_txt', 'plots'):
        with pytest.raises(RuntimeError, match=f'{k}=True is host-side tooling'):
            RTDETRValidator('cpu', args={k: True})
    v = RTDETRValidator('cpu', args={'conf': 0.001})
    for call in (lambda: v.build_dataset('images'), lambda: v.pred_to_json(None, None), lambda: v.plot_predictions(None, None, 0)):
        with pytest.raises(RuntimeError, match='host-side tooling'):
            call()


# ================================================================================================================ GPU
def batch_of(imgs, ori):
    lab = [torch.from_numpy(im['labels']) for im in imgs]
    return dict(cls=torch.cat([l[:, :1] for l in lab]), bboxes=torch.cat([l[:, 1:] for l in lab]),
                batch_idx=torch.cat([torch.full((len(l),), float(i)) for i, l in enumerate(lab)]), ori_shape=list(ori))


@gpu
def test_postprocess_update_metrics_and_stats(fx):
    """rows within 1e-6 (normalised) in the reference's order, the recorded `correct` matrices exactly, the recorded metrics exactly (as the detection
    validator's test compares its own); one image per call as in the generator (100 and 300 rows), both through ONE validator"""
    from mgdt_yolo_amd.vit.rtdetr import RTDETRValidator
    v = RTDETRValidator(DEV)
    v.init_metrics(nc=LR.VAL['nc'])
    imgs = LR.make_val_inputs()
    for si, im in enumerate(imgs):
        preds = (torch.from_numpy(im['boxes'])[None, None].to(DEV), torch.from_numpy(im['scores'])[None, None].to(DEV))
        per = v.postprocess(preds)
        want = fx[f'i_rows_{si}']
        got = per[0].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got[:, 4:], want[:, 4:]), 'confidence, class and order'
        assert np.abs(got[:, :4] - want[:, :4]).max() <= 1e-6
        v.update_metrics(per, v.preprocess(dict(batch_of([im], [LR.VAL['ori_shape'][si]]), img=torch.zeros(1, 3, 32, 32))))
        assert np.array_equal(v.stats[-1][0].cpu().numpy(), fx[f'i_correct_{si}'])
    res = v.get_stats()
    assert v.seen == 2
    for k, want in zip(fx['i_metric_keys'], fx['i_metrics']):
        if str(k) != 'fitness':
            assert res[str(k)] == float(want), (k, res[str(k)], float(want))


@gpu
def test_a_batch_equals_its_images_one_by_one(fx):
    """two images of 100 rows in one batch with different ori_shapes, one without labels, one whose labels match no predicted class"""
    from mgdt_yolo_amd.vit.rtdetr import RTDETRValidator
    im = LR.make_val_inputs()[0]
    boxes = torch.from_numpy(np.stack([im['boxes'], im['boxes'][::-1].copy(), im['boxes']])).to(DEV)
    scores = torch.from_numpy(np.stack([im['scores'], im['scores'][::-1].copy(), im['scores']])).to(DEV)
    lab = torch.from_numpy(im['labels'])
    other = lab.clone()
    other[:, 0] = LR.VAL['nc'] + 3                       # a class no prediction has
    batch = dict(cls=torch.cat([lab[:, :1], other[:, :1]]), bboxes=torch.cat([lab[:, 1:], other[:, 1:]]),
                 batch_idx=torch.cat([torch.zeros(len(lab)), torch.full((len(lab),), 2.0)]), ori_shape=[(480, 640), (375, 500), (100, 200)],
                 img=torch.zeros(3, 3, 32, 32))
    v = RTDETRValidator(DEV)
    v.init_metrics(nc=LR.VAL['nc'] + 4)
    per = v.postprocess((boxes[None], scores[None]))
    assert len(per) == 3 and all(tuple(p.shape) == (100, 6) for p in per)
    assert torch.equal(per[0], per[2]) and np.array_equal(per[0].cpu().numpy()[:, 4:], fx['i_rows_0'][:, 4:])
    assert torch.equal(per[1][:, 4:], per[0][:, 4:]), 'the reversed image: distinct confidences, the same order'
    v.update_metrics(per, v.preprocess(batch))
    assert v.seen == 3 and len(v.stats) == 3
    assert np.array_equal(v.stats[0][0].cpu().numpy(), fx['i_correct_0'])
    assert not v.stats[1][0].any() and v.stats[1][3].numel() == 0, 'no labels: nothing correct, the row is still counted'
    assert not v.stats[2][0].any() and v.stats[2][3].numel() == len(lab), 'no matching class'


@gpu
@pytest.mark.parametrize('nq', (1, 100, 300))
def test_val_post_order_ties_and_nan(nq):
    """all nq rows, no threshold; equal confidences by ascending query index; NaN last; boxes scaled by wh"""
    from mgdt_yolo_amd import ops
    r = np.random.RandomState(nq)
    nc = 3
    boxes = torch.from_numpy(np.concatenate([r.uniform(0.1, 0.9, (2, nq, 2)), r.uniform(0.05, 0.4, (2, nq, 2))], -1)).float()
    scores = torch.from_numpy(np.round(r.uniform(0, 1, (2, nq, nc)) * 8) / 8).float()      # 9 levels: many ties
    if nq >= 100:
        scores[1, 7] = float('nan')
        scores[1, 40, 1] = float('nan')
    wh = torch.tensor([[640.0, 480.0], [500.0, 375.0]])
    rows, counts = ops.rtdetr_val_post(boxes.to(DEV), scores.to(DEV), wh.to(DEV))
    rows, counts = rows.cpu(), counts.cpu()
    assert counts.tolist() == [nq, nq] and tuple(rows.shape) == (2, nq, 6)
    for b in range(2):
        sc = scores[b]
        nan = torch.isnan(sc).any(-1)
        want = LR.val_rows(boxes[b][~nan], sc[~nan])
        order = torch.from_numpy(np.argsort(-sc[~nan].max(-1).values.numpy(), kind='stable'))
        n = int((~nan).sum())
        scale = torch.tensor([wh[b, 0], wh[b, 1], wh[b, 0], wh[b, 1]])
        assert torch.equal(rows[b, :n, 4:], want[:, 4:]) and (rows[b, :n, :4] - want[:, :4] * scale).abs().max() <= 1e-6 * 640
        qidx = torch.nonzero(~nan).flatten()[order]
        ties = rows[b, :n, 4][1:] == rows[b, :n, 4][:-1]
        assert bool((qidx[1:][ties] > qidx[:-1][ties]).all()), 'equal confidences by ascending query index'
        assert torch.isnan(rows[b, n:, 4]).all() and rows[b, n:].shape[0] == int(nan.sum())
    none, _ = ops.rtdetr_val_post(boxes.to(DEV), scores.to(DEV))
    assert torch.equal(none.cpu()[0, :, 4:], rows[0, :, 4:])
