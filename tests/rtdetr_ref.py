"""Restatements of the RT-DETR decoder head in plain torch (reference nn/modules/head.py:275-464, nn/modules/transformer.py:187-378,
nn/modules/utils.py:36-80, vit/rtdetr/predict.py), written from the formulas, not copied.  Every function computes in the dtype of its inputs, so the
same code gives the float64 truth and the CPU fp32 run whose distance to it sizes the fp32 bounds of the GPU tests.  Also: the case table shared by
the fixture generator (tests/golden/gen_rtdetr.py) and the tests."""
import math

import numpy as np
import torch

NH, DH, NP, HD = 8, 32, 4, 256
IMG_SEED = 3
WEIGHT_SEED = 0

# tag -> (head row arguments after nc or None for the YAML's own row, nc, input (B, H, W))
CASES = {
    'A': (None, 80, (2, 160, 160)),                 # square maps, L = 525
    'B': (None, 80, (2, 128, 192)),                 # non-square maps, L = 504: 168 invalid tokens, all tied, all selected
    'C': ([256, 100, 4, 8, 2], 3, (1, 96, 160)),    # nq 100, 2 layers, a class count the MFMA route does not take, L = 315: 126 tied invalid tokens > nq
    'D': ([256, 100, 4, 8, 2], 3, (1, 96, 96)),     # the same head on square maps, L = 189: no invalid token, distinct queries
}
BF16 = ('A', 'B')                                   # cases with a recorded bf16 emulation
CHAINED = ('C', 'D')                                # cases whose head inputs and per-layer boxes are recorded in float64


def case_cfg(tag):
    """the model dict of a case (the repository's own graph table; the generator checks it against the reference's YAML)"""
    from mgdt_yolo_amd.models import get_config
    row, nc, _ = CASES[tag]
    cfg = get_config('yolov8-rtdetr', 'n', nc)
    if row is not None:
        cfg['head'][-1][3] = ['nc'] + list(row)
    return cfg


def case_nq_ndl(tag):
    row = CASES[tag][0]
    return (300, 6) if row is None else (row[1], row[4])


def level_shapes(h, w):
    return [(-(-h // s), -(-w // s)) for s in (8, 16, 32)]


# ---------------------------------------------------------------------------------------------------------------- pieces
def deform_attn(value, shapes, ref, off, wl):
    """value (B, L, 256), ref (B, nq, 4), off (B, nq, 8*nl*4*2), wl (B, nq, 8*nl*4) -> (B, nq, 256)"""
    B, L, _ = value.shape
    nq, nl = ref.shape[1], len(shapes)
    v = value.reshape(B, L, NH, DH)
    off = off.reshape(B, nq, NH, nl, NP, 2)
    w = torch.softmax(wl.reshape(B, nq, NH, nl * NP), -1).reshape(B, nq, NH, nl, NP)
    loc = ref[:, :, None, None, None, :2] + off / NP * ref[:, :, None, None, None, 2:] * 0.5
    out = torch.zeros(B, nq, NH, DH, dtype=value.dtype)
    bi = torch.arange(B)[:, None, None, None].expand(B, nq, NH, NP)
    hi = torch.arange(NH)[None, None, :, None].expand(B, nq, NH, NP)
    start = 0
    for l, (H, W) in enumerate(shapes):
        vl = v[:, start:start + H * W].reshape(B, H, W, NH, DH)
        start += H * W
        px, py = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
        x0, y0 = torch.floor(px), torch.floor(py)
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi = x0 + dx, y0 + dy
                wt = (1 - (px - xi).abs()) * (1 - (py - yi).abs())
                ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
                xc, yc = xi.clamp(0, W - 1).long(), yi.clamp(0, H - 1).long()
                g = vl[bi, yc, xc, hi]                                     # (B, nq, NH, NP, DH)
                out += (g * (wt * ok * w[:, :, :, l])[..., None]).sum(3)
    return out.reshape(B, nq, HD)


def mha(q, k, v):
    B, n, _ = q.shape
    sp = lambda t: t.reshape(B, n, NH, DH).permute(0, 2, 1, 3)
    s = (sp(q) * math.sqrt(1.0 / DH)) @ sp(k).transpose(-1, -2)
    return (torch.softmax(s, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, n, HD)


def add_ln(x, res, gamma, beta, eps=1e-5, valid=None, fill=None):
    if valid is not None:
        x = torch.where(valid[None, :, None], x, fill.expand_as(x))
    if res is not None:
        x = x + res
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def anchors(shapes, dtype):
    """(anchor logits (L, 4) with +inf rows for invalid tokens, valid (L,)): (x + 0.5, y + 0.5) divided by (h, w) in this order, as the reference does"""
    rows = []
    for i, (h, w) in enumerate(shapes):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing='ij')
        a = torch.stack([(xs + 0.5) / torch.tensor(h, dtype=dtype), (ys + 0.5) / torch.tensor(w, dtype=dtype),
                         torch.full_like(xs, 1.0) * 0.05 * (2.0 ** i), torch.full_like(xs, 1.0) * 0.05 * (2.0 ** i)], -1)
        rows.append(a.reshape(h * w, 4))
    a = torch.cat(rows, 0)
    valid = ((a > 1e-2) & (a < 1 - 1e-2)).all(-1)
    return torch.where(valid[:, None], torch.log(a / (1 - a)), torch.full_like(a, float('inf'))), valid


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def refine(delta, ref):
    return torch.sigmoid(delta + inverse_sigmoid(ref))


def stable_topk(scores, k):
    """(B, L) -> (B, k) int64: descending score, equal scores by ascending index"""
    s = scores.detach().cpu().numpy()
    return torch.from_numpy(np.stack([np.argsort(-r, kind='stable')[:k] for r in s]).astype(np.int64))


def post(boxes, scores, conf, classes=None, wh=None):
    """boxes (B, nq, 4) xywh, scores (B, nq, nc) -> per image (n, 6) [x1, y1, x2, y2, conf, cls] in query order"""
    out = []
    for i in range(boxes.shape[0]):
        b = boxes[i]
        xyxy = torch.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], -1)
        sc, cl = scores[i].max(-1)
        keep = sc > conf
        if classes is not None:
            keep &= torch.isin(cl, torch.as_tensor(list(classes)))
        if wh is not None:
            xyxy = xyxy * torch.as_tensor([wh[i][0], wh[i][1], wh[i][0], wh[i][1]], dtype=xyxy.dtype)
        out.append(torch.cat([xyxy, sc[:, None], cl[:, None].to(xyxy.dtype)], -1)[keep])
    return out


# ---------------------------------------------------------------------------------------------------------------- the head
def _lin(sd, name, x, relu=False):
    y = x @ sd[name + '.weight'].T + sd[name + '.bias']
    return torch.relu(y) if relu else y


def _mlp(sd, name, x, n):
    for j in range(n):
        x = _lin(sd, f'{name}.layers.{j}', x, relu=j < n - 1)
    return x


def head_forward(sd, feats, nq, ndl, index=None, bn_eps=1e-3, trace=None):
    """The eval forward of RTDETRDecoder on its input maps `feats` (list of (B, C, h, w)) with the head's state dict `sd` (keys without the layer
    prefix) -> dict(score_max, index, enc_bboxes, enc_scores, dec_bboxes, dec_scores).  `index` replaces the selection; `trace`: list receiving the
    refined boxes after each layer."""
    dt = feats[0].dtype
    shapes = [(int(f.shape[2]), int(f.shape[3])) for f in feats]
    toks = []
    for i, f in enumerate(feats):
        w = sd[f'input_proj.{i}.0.weight'][:, :, 0, 0]
        y = f.flatten(2).permute(0, 2, 1) @ w.T
        g, b, mu, var = (sd[f'input_proj.{i}.1.{n}'] for n in ('weight', 'bias', 'running_mean', 'running_var'))
        toks.append((y - mu) / torch.sqrt(var + bn_eps) * g + b)
    memory = torch.cat(toks, 1)
    anc, valid = anchors(shapes, dt)
    x = _lin(sd, 'enc_output.0', torch.where(valid[None, :, None], memory, torch.zeros_like(memory)))
    features = add_ln(x, None, sd['enc_output.1.weight'], sd['enc_output.1.bias'])
    logits = _lin(sd, 'enc_score_head', features)
    score_max = logits.max(-1).values
    if index is None:
        index = stable_topk(score_max, nq)
    B = memory.shape[0]
    bi = torch.arange(B)[:, None]
    embed = features[bi, index]
    enc_scores = logits[bi, index]
    ref = torch.sigmoid(_mlp(sd, 'enc_bbox_head', embed, 3) + anc[index])
    enc_bboxes = ref
    for i in range(ndl):
        p = f'decoder.layers.{i}.'
        pos = _mlp(sd, 'query_pos_head', ref, 2)
        W, bias = sd[p + 'self_attn.in_proj_weight'], sd[p + 'self_attn.in_proj_bias']
        qk_in = embed + pos
        q, k, v = qk_in @ W[:HD].T + bias[:HD], qk_in @ W[HD:2 * HD].T + bias[HD:2 * HD], embed @ W[2 * HD:].T + bias[2 * HD:]
        embed = add_ln(_lin(sd, p + 'self_attn.out_proj', mha(q, k, v)), embed, sd[p + 'norm1.weight'], sd[p + 'norm1.bias'])
        qc = embed + pos
        samp = deform_attn(_lin(sd, p + 'cross_attn.value_proj', memory), shapes, ref, _lin(sd, p + 'cross_attn.sampling_offsets', qc),
                           _lin(sd, p + 'cross_attn.attention_weights', qc))
        embed = add_ln(_lin(sd, p + 'cross_attn.output_proj', samp), embed, sd[p + 'norm2.weight'], sd[p + 'norm2.bias'])
        embed = add_ln(_lin(sd, p + 'linear2', _lin(sd, p + 'linear1', embed, relu=True)), embed, sd[p + 'norm3.weight'], sd[p + 'norm3.bias'])
        ref = refine(_mlp(sd, f'dec_bbox_head.{i}', embed, 3), ref)
        if trace is not None:
            trace.append(ref)
    scores = torch.sigmoid(_lin(sd, f'dec_score_head.{ndl - 1}', embed))
    return dict(score_max=score_max, index=index, enc_bboxes=enc_bboxes, enc_scores=enc_scores, dec_bboxes=ref, dec_scores=scores)


def head_state(model, dtype=torch.float64):
    """the head's state dict without the layer prefix, converted"""
    n = len(model.model) - 1
    pre = f'model.{n}.'
    return {k[len(pre):]: (v.to(dtype) if v.is_floating_point() else v) for k, v in model.state_dict().items() if k.startswith(pre)}


def load_fixtures(golden_dir):
    """every array of tests/golden/rtdetr_NN.npz in one dict"""
    import glob
    import os
    out = {}
    for p in sorted(glob.glob(os.path.join(golden_dir, 'rtdetr_[0-9][0-9].npz'))):
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out
