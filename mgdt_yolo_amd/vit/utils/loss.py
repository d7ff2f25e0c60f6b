"""reference: vit/utils/loss.py - DETRLoss / RTDETRDetectionLoss.  A whole criterion call without denoising is TWO launches: mgdt_detr_match_fwd
(costs + exact assignment of every layer and image) and mgdt_detr_loss_fwd (the three losses of every layer and, when asked for, the gradients of
their sum with respect to the head outputs); no host read, no per-layer or per-image loop.  A denoising pass is a second mgdt_detr_loss_fwd whose
assignment is built from `dn_pos_idx`; the generation of the denoising queries (get_cdn_group) is not built.  use_fl=False and the mask / dice
losses are not built."""
import torch
from torch import nn

from ... import ops as hip
from .ops import HungarianMatcher, _targets

__all__ = ('DETRLoss', 'RTDETRDetectionLoss', 'loss_and_head_grads')

_NAMES = ('loss_class', 'loss_bbox', 'loss_giou')
_ZERO = {}


def _zero(device):
    """a 0-d zero on `device`, made once (a host scalar cannot be copied while a graph is being captured)"""
    device = torch.device(device)
    if device not in _ZERO:
        _ZERO[device] = torch.zeros((), device=device)
    return _ZERO[device]


class _DetrLossFn(torch.autograd.Function):
    """(2, 3) = the last layer's losses and the auxiliary layers' sums of one mgdt_detr_loss_fwd; the launch also leaves the gradient of their plain
    sum with respect to boxes and logits, which backward scales.  Every entry must reach the final loss with the same weight (the criterion's dict
    summed, as the reference's trainer does): another weighting has no single scale and gives NaN gradients."""

    @staticmethod
    def forward(ctx, boxes, logits, crit, gb, gc, assign, num_pairs):
        out, _, d_boxes, d_logits = crit._launch(boxes.detach(), logits.detach(), gb, gc, assign, num_pairs, 1.0, True)
        ctx.save_for_backward(d_boxes, d_logits)
        ctx.aux = boxes.shape[0] > 1
        return out[-2:]

    @staticmethod
    def backward(ctx, g):
        d_boxes, d_logits = ctx.saved_tensors
        g = g if ctx.aux else g[:1]
        w = g.reshape(-1)[0]
        w = torch.where((g == w).all(), w, torch.full_like(w, float('nan')))
        return d_boxes * w, d_logits * w, None, None, None, None, None


class DETRLoss(nn.Module):

    def __init__(self, nc=80, loss_gain=None, aux_loss=True, use_fl=True, use_vfl=False, use_uni_match=False, uni_match_ind=0):
        super().__init__()
        if not use_fl:
            raise NotImplementedError('DETRLoss: use_fl=False (plain BCE class loss) is not built')
        if loss_gain is None:
            loss_gain = {'class': 1, 'bbox': 5, 'giou': 2, 'no_object': 0.1, 'mask': 1, 'dice': 1}
        self.nc = nc
        self.matcher = HungarianMatcher(cost_gain={'class': 2, 'bbox': 5, 'giou': 2})
        self.loss_gain, self.aux_loss, self.use_fl, self.use_vfl = loss_gain, aux_loss, use_fl, use_vfl
        self.use_uni_match, self.uni_match_ind = use_uni_match, uni_match_ind
        self.device = None

    def _get_loss_mask(self, *a, **k):
        raise NotImplementedError('DETRLoss: the mask and dice losses are not built')

    _dice_loss = _get_loss_mask

    def _launch(self, boxes, logits, gb, gc, assign, num_pairs, gscale, want_grads):
        g = self.loss_gain
        return hip.detr_loss(boxes.float().contiguous(), logits.float().contiguous(), gb, gc, assign, num_pairs, gains=(g['class'], g['bbox'], g['giou']),
                             use_vfl=self.use_vfl, gscale=gscale, want_grads=want_grads)

    def _assign(self, pred_bboxes, pred_scores, gb, gc, gt_groups, gt_off=None):
        layers = pred_bboxes.shape[0]
        k = -1
        if self.use_uni_match and self.aux_loss and layers > 1:
            # the reference matches the last layer on its own costs and every auxiliary layer on layer uni_match_ind's (of the auxiliary stack)
            k = self.uni_match_ind % (layers - 1)
        a = self.matcher.assign(pred_bboxes, pred_scores, gb, gc, gt_groups, layer_of_match=k, gt_off=gt_off)
        if k >= 0:
            last = self.matcher.assign(pred_bboxes[-1:], pred_scores[-1:], gb, gc, gt_groups, gt_off=gt_off)
            a = torch.cat((a[:-1], last))
        return a

    def _dict(self, out, postfix):
        """the kernel's last two rows (the last layer, the sum of the others) -> the reference's dict; views only, no launch"""
        loss = {f'{n}{postfix}': out[-2, i] for i, n in enumerate(_NAMES)}
        if self.aux_loss:
            loss.update({f'{n}_aux{postfix}': out[-1, i] for i, n in enumerate(_NAMES)})
        return loss

    def _pass(self, pred_bboxes, pred_scores, gb, gc, assign, num_pairs, postfix):
        if not self.aux_loss:
            pred_bboxes, pred_scores, assign = pred_bboxes[-1:], pred_scores[-1:], assign[-1:]
        if pred_bboxes.requires_grad or pred_scores.requires_grad:
            out = _DetrLossFn.apply(pred_bboxes, pred_scores, self, gb, gc, assign.contiguous(), num_pairs)
        else:
            out = self._launch(pred_bboxes, pred_scores, gb, gc, assign.contiguous(), num_pairs, 1.0, False)[0]
        return self._dict(out, postfix)

    def forward(self, pred_bboxes, pred_scores, batch, postfix='', **kwargs):
        """pred_bboxes (l, B, nq, 4), pred_scores (l, B, nq, nc) raw; batch: 'cls' (G,), 'bboxes' (G, 4), 'gt_groups' (host list).  match_indices=:
        a (l, B, nq) int32 device assignment (or (B, nq), shared by every layer) with num_pairs= its pairs per layer, in place of the matcher."""
        self.device = pred_bboxes.device
        gb, gc = _targets(batch['bboxes'], batch['cls'], self.device)
        gt_groups = [int(n) for n in batch['gt_groups']]
        assign = kwargs.get('match_indices')
        if assign is None:
            assign, num_pairs = self._assign(pred_bboxes, pred_scores, gb, gc, gt_groups, batch.get('gt_off')), sum(gt_groups)
        else:
            num_pairs = kwargs['num_pairs']
            if assign.dim() == 2:
                assign = assign[None].expand(pred_bboxes.shape[0], -1, -1)
        return self._pass(pred_bboxes, pred_scores, gb, gc, assign, num_pairs, postfix)


class RTDETRDetectionLoss(DETRLoss):

    def forward(self, preds, batch, dn_bboxes=None, dn_scores=None, dn_meta=None):
        pred_bboxes, pred_scores = preds
        total_loss = super().forward(pred_bboxes, pred_scores, batch)
        if dn_meta is not None:
            dn_pos_idx, dn_num_group = dn_meta['dn_pos_idx'], dn_meta['dn_num_group']
            assert len(batch['gt_groups']) == len(dn_pos_idx)
            match_indices = self.get_dn_match_indices(dn_pos_idx, dn_num_group, batch['gt_groups'])
            assign = torch.full(tuple(dn_bboxes.shape[1:3]), -1, dtype=torch.int32)
            for i, (q, g) in enumerate(match_indices):
                assign[i, q.long()] = g.to(torch.int32)
            num_pairs = sum(len(q) for q, _ in match_indices)
            total_loss.update(super().forward(dn_bboxes, dn_scores, batch, postfix='_dn', match_indices=assign.to(self.device), num_pairs=num_pairs))
        else:
            total_loss.update({f'{k}_dn': _zero(self.device) for k in list(total_loss.keys())})
        return total_loss

    @staticmethod
    def get_dn_match_indices(dn_pos_idx, dn_num_group, gt_groups):
        """Per image (positive denoising queries, the global index of the ground truth each one reconstructs): every group repeats the image's
        ground truths in order."""
        out, start = [], 0
        for i, num_gt in enumerate(gt_groups):
            if num_gt > 0:
                gt_idx = (torch.arange(num_gt, dtype=torch.int32) + start).repeat(dn_num_group)
                assert len(dn_pos_idx[i]) == len(gt_idx), f'Expected the same length, but got {len(dn_pos_idx[i])} and {len(gt_idx)} respectively.'
                out.append((dn_pos_idx[i], gt_idx))
            else:
                out.append((torch.zeros([0], dtype=torch.int32), torch.zeros([0], dtype=torch.int32)))
            start += num_gt
        return out


def loss_and_head_grads(crit, preds, batch, gscale=1.0, match_indices=None):
    """The explicit form a reverse pass of the decoder starts from: (loss dict, d_boxes (l, B, nq, 4), d_logits (l, B, nq, nc)), the gradients of
    gscale * (the sum of the dict's entries), without denoising.  Two launches (one when `match_indices`, a (l, B, nq) int32 assignment, is given)."""
    pred_bboxes, pred_scores = preds
    crit.device = pred_bboxes.device
    gb, gc = _targets(batch['bboxes'], batch['cls'], crit.device)
    gt_groups = [int(n) for n in batch['gt_groups']]
    assign = crit._assign(pred_bboxes, pred_scores, gb, gc, gt_groups, batch.get('gt_off')) if match_indices is None else match_indices
    if not crit.aux_loss:
        raise NotImplementedError('loss_and_head_grads: aux_loss=False is not built (pass the last layer alone)')
    out, _, d_boxes, d_logits = crit._launch(pred_bboxes.detach(), pred_scores.detach(), gb, gc, assign.contiguous(), sum(gt_groups), gscale, True)
    loss = crit._dict(out, '')
    if isinstance(crit, RTDETRDetectionLoss):
        loss.update({f'{k}_dn': _zero(crit.device) for k in list(loss.keys())})
    return loss, d_boxes, d_logits
