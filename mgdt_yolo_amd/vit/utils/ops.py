"""reference: vit/utils/ops.py:12-111 - HungarianMatcher.  Costs and the exact assignment of every (layer, image) in ONE launch
(mgdt_detr_match_fwd); the reference copies the cost matrix to the host and calls scipy per image and per layer.  `get_cdn_group` (the random
denoising queries) is not built."""
import torch
from torch import nn

from ... import ops as hip

__all__ = ('HungarianMatcher',)


def _targets(gt_bboxes, gt_cls, device):
    """the flat ground truths as the kernels read them: (G, 4) fp32 and (G,) int32 on the device"""
    return (gt_bboxes.to(device=device, dtype=torch.float32).reshape(-1, 4).contiguous(),
            gt_cls.to(device=device).reshape(-1).to(torch.int32).contiguous())


class HungarianMatcher(nn.Module):
    """The reference's constructor and `forward`.  `assign` is the device form for any number of layers.  The softmax class cost (use_fl=False) and
    the mask costs (with_mask=True) are not built."""

    def __init__(self, cost_gain=None, use_fl=True, with_mask=False, num_sample_points=12544, alpha=0.25, gamma=2.0):
        super().__init__()
        if not use_fl:
            raise NotImplementedError('HungarianMatcher: use_fl=False (the softmax class cost) is not built')
        if with_mask:
            raise NotImplementedError('HungarianMatcher: with_mask=True (mask and dice costs) is not built')
        if cost_gain is None:
            cost_gain = {'class': 1, 'bbox': 5, 'giou': 2, 'mask': 1, 'dice': 1}
        self.cost_gain, self.use_fl, self.with_mask, self.num_sample_points, self.alpha, self.gamma = cost_gain, use_fl, with_mask, num_sample_points, alpha, gamma

    def assign(self, pred_bboxes, pred_scores, gt_bboxes, gt_cls, gt_groups, layer_of_match=-1, gt_off=None, want_cost=False):
        """pred_bboxes (layers, B, nq, 4), pred_scores (layers, B, nq, nc) raw logits, gt_bboxes (G, 4), gt_cls (G,), gt_groups: the host's list of
        per-image counts -> assign (layers, B, nq) int32 on the device: the global ground-truth index of each query or -1 [, the cost block].  One
        launch, no host read.  layer_of_match = k >= 0: layer k's assignment for every layer (use_uni_match)."""
        gb, gc = _targets(gt_bboxes, gt_cls, pred_bboxes.device)
        g = self.cost_gain
        return hip.detr_match(pred_bboxes.detach().float().contiguous(), pred_scores.detach().float().contiguous(), gb, gc, [int(n) for n in gt_groups], gt_off=gt_off,
                              gains=(g['class'], g['bbox'], g['giou']), alpha=self.alpha, gamma=self.gamma, layer_of_match=layer_of_match, want_cost=want_cost)

    def forward(self, pred_bboxes, pred_scores, gt_bboxes, gt_cls, gt_groups, masks=None, gt_mask=None):
        """pred_bboxes (B, nq, 4), pred_scores (B, nq, nc) -> the reference's list of (int32 queries ascending, int32 global gt index) CPU tensors, one
        pair per image (one host read)."""
        if masks is not None or gt_mask is not None:
            raise NotImplementedError('HungarianMatcher: mask costs are not built')
        bs = pred_scores.shape[0]
        if sum(gt_groups) == 0:
            return [(torch.tensor([], dtype=torch.int32), torch.tensor([], dtype=torch.int32)) for _ in range(bs)]
        a = self.assign(pred_bboxes[None], pred_scores[None], gt_bboxes, gt_cls, gt_groups)[0].cpu()
        out = []
        for i in range(bs):
            q = torch.nonzero(a[i] >= 0).flatten()
            out.append((q.to(torch.int32), a[i][q].to(torch.int32)))
        return out
