"""Generate tests/golden/rtdetr_NN.npz and tests/golden/rtdetr_yaml.json: RT-DETR fixtures from the reference's own Python modules (BUILD CONTAINER ONLY).

    python tests/golden/gen_rtdetr.py

Recipe of gen_pose.py: ref_import unchanged, plus two shell packages `ultralytics.vit` / `ultralytics.vit.utils` pointing at the reference's folders
(the real vit/__init__ pulls in SAM and the exporter); weights from seeding.seed_state_dict_, images from seeded_images, CPU.  torch.topk is
intercepted inside the reference call to record the scores it ranks and its indices, and to force indices.  Recorded:
  - rtdetr_yaml.json: the reference's models/v8/yolov8-rtdetr.yaml parsed to a dict (a settings fixture);
  - per case of tests/rtdetr_ref.py:CASES: state-dict keys / shapes, parameter count, `sampling_offsets.bias` of layer 0, `enc_score_head.bias`;
    score_max (B, L), the reference's own top-k indices, and the selection in this library's order (descending score, equal scores by ascending token
    index); with THAT index forced: enc_bboxes, enc_scores, dec_bboxes, dec_scores in fp32, the same from the .double() copy, and the largest
    fp32-vs-fp64 difference per quantity (box in input pixels = normalised x (w, h), confidence, score_max);
  - cases C and D: the head's input maps of the .double() model and the refined boxes after each decoder layer (fp32 and fp64);
  - case A: the predictor's rows (vit/rtdetr/predict.py:13-33, tensor source) at a conf chosen HERE from the score distribution.
The generator asserts the conditions that make an exact selection comparable and walks the image seed until they hold (printing what it tried): no
score_max within max(1e-5, 16 x d64(score_max)) of the midpoint between the nq-th and (nq+1)-th score; the tied group of invalid tokens entirely
inside or outside the selection; fp32 and fp64 select the same set; (case A) pairwise distinct final confidences.  Case C cannot meet the second
condition at any seed: its 126 invalid tokens share the top score and nq is 100, so the cut falls inside the tied group, whose tokens are identical
queries.  There the generator asserts instead that every other token is off the group's score by the same margin and that torch.topk chose the same
untied tokens: whichever tied tokens fill the rest, the values are the same.  Case D (the same head on a square input, no invalid token) is this
repository's addition, so that nq 100 / nc 3 / two layers are also pinned with distinct queries.
Cases A and B also record the largest differences of a bf16 EMULATION (bf16_emulation below) to the fp32 outputs, indices forced: free-running bf16
swaps a few of the 300 queries, so bf16 end-to-end parity is tested with forced indices.  The GPU box never runs this file.
"""
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_import  # noqa: E402
import rtdetr_ref as RR  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402

torch.set_num_threads(8)
ns = ref_import.load()
REF = ref_import.REF
for name, sub in (('ultralytics.vit', 'vit'), ('ultralytics.vit.utils', os.path.join('vit', 'utils'))):
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(REF, sub)]
    sys.modules[name] = pkg
REFY = os.path.join(REF, 'models', 'v8')
_TOPK = torch.topk


class TopkTap:
    """with TopkTap(force=None) as t: ...  -> t.values / t.indices of the (single) torch.topk call inside; `force`: the indices it returns instead"""

    def __init__(self, force=None):
        self.force, self.calls = force, 0

    def __enter__(self):
        def topk(inp, k, dim=-1, **kw):
            self.calls += 1
            r = _TOPK(inp, k, dim=dim, **kw)
            self.values, self.indices = inp.detach().clone(), r.indices.clone()
            if self.force is None:
                return r
            assert tuple(self.force.shape) == tuple(r.indices.shape)
            return types.SimpleNamespace(values=torch.gather(inp, dim, self.force), indices=self.force.clone())
        torch.topk = topk
        return self

    def __exit__(self, *exc):
        torch.topk = _TOPK
        return False


def save(arrs, limit=900 * 1024):
    import glob
    for old in glob.glob(os.path.join(HERE, 'rtdetr_[0-9][0-9].npz')):
        os.remove(old)
    shards, cur, size = [], {}, 0
    for k, v in arrs.items():
        v = np.asarray(v)
        assert v.nbytes <= limit, (k, v.nbytes)
        if size + v.nbytes > limit:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    shards.append(cur)
    for n, sh in enumerate(shards):
        path = os.path.join(HERE, f'rtdetr_{n:02d}.npz')
        np.savez_compressed(path, **sh)
        sz = os.path.getsize(path)
        print(f'rtdetr_{n:02d}: {len(sh)} arrays, {sz / 1024:.1f} KiB')
        assert sz < (1 << 20), f'{path} is {sz} bytes: over the 1 MiB limit of a committed file'


def build(tag, tmp):
    row, nc, _ = RR.CASES[tag]
    path = os.path.join(REFY, 'yolov8n-rtdetr.yaml')
    if row is not None:
        src = open(os.path.join(REFY, 'yolov8-rtdetr.yaml')).read().splitlines()
        out, done = [], False
        for line in src:
            if 'RTDETRDecoder' in line and line.lstrip().startswith('- [['):
                line = line[:line.index('- [[')] + f'- [[15, 18, 21], 1, RTDETRDecoder, [nc, {", ".join(map(str, row))}]]'
                done = True
            out.append(line)
        assert done
        os.makedirs(os.path.join(tmp, tag), exist_ok=True)
        path = os.path.join(tmp, tag, 'yolov8n-rtdetr.yaml')
        open(path, 'w').write('\n'.join(out) + '\n')
    m = ns.tasks.RTDETRDetectionModel(path, nc=nc, verbose=False)
    seed_state_dict_(m, RR.WEIGHT_SEED)
    return m.eval()


def structure(arrs, tag, m):
    sd = m.state_dict()
    arrs[f'{tag}_keys'] = np.array(list(sd.keys()))
    arrs[f'{tag}_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    arrs[f'{tag}_nparams'] = np.array(sum(p.numel() for p in m.parameters()), np.int64)
    arrs[f'{tag}_stride'] = m.stride.numpy()


def init_values(arrs, tag, tmp):
    """the deterministic initial values of a freshly built (unseeded) reference model"""
    row, nc, _ = RR.CASES[tag]
    path = os.path.join(REFY, 'yolov8n-rtdetr.yaml') if row is None else os.path.join(tmp, tag, 'yolov8n-rtdetr.yaml')
    m = ns.tasks.RTDETRDetectionModel(path, nc=nc, verbose=False)
    h = m.model[-1]
    arrs[f'{tag}_init_offsets_bias'] = h.decoder.layers[0].cross_attn.sampling_offsets.bias.detach().numpy()
    arrs[f'{tag}_init_enc_score_bias'] = h.enc_score_head.bias.detach().numpy()
    assert float(h.decoder.layers[0].cross_attn.attention_weights.weight.abs().max()) == 0.0
    assert float(h.enc_bbox_head.layers[-1].weight.abs().max()) == 0.0 and float(h.dec_bbox_head[-1].layers[-1].bias.abs().max()) == 0.0


def run(m, x, force=None, want_inputs=False, want_layers=False):
    """one reference forward -> dict; the per-layer refined boxes are rebuilt from the box heads' outputs with the reference's inverse_sigmoid"""
    head = m.model[-1]
    grabbed, hooks = {'delta': []}, []
    if want_inputs:
        hooks.append(head.register_forward_pre_hook(lambda _m, a: grabbed.__setitem__('inputs', [t.detach().clone() for t in a[0]])))
    if want_layers:
        for bh in head.dec_bbox_head:
            hooks.append(bh.register_forward_hook(lambda _m, _i, o: grabbed['delta'].append(o.detach().clone())))
    with torch.no_grad(), TopkTap(force) as tap:
        dec_b, dec_s, enc_b, enc_s, meta = m(x)
    for h in hooks:
        h.remove()
    assert tap.calls == 1 and meta is None and dec_b.shape[0] == 1
    out = dict(score_max=tap.values, topk=tap.indices, dec_bboxes=dec_b[0], dec_scores=dec_s[0], enc_bboxes=enc_b, enc_scores=enc_s)
    if want_inputs:
        out['inputs'] = grabbed['inputs']
    if want_layers:
        inv = sys.modules['ultralytics.nn.modules.utils'].inverse_sigmoid
        ref, layers = enc_b, []
        for d in grabbed['delta']:
            ref = torch.sigmoid(d + inv(ref))
            layers.append(ref)
        assert torch.equal(layers[-1], dec_b[0])
        out['layers'] = torch.stack(layers)
    return out


def bf16_emulation(m):
    """A copy of `m` that rounds to bf16 exactly what the HIP bf16 path rounds: the input; in front of the head every parameter and the output of every
    Conv (gen_pose.py's recipe); in the head the input projections (parameters, output = the token memory), the weight and the output of enc_output's
    linear (its bias stays fp32 in the GEMM epilogue; a zeroed token's output is the rounded bias) and the weight and output of every value_proj.
    Scores, selection and the whole query side stay fp32."""
    e = copy.deepcopy(m)
    r = lambda t: t.to(torch.bfloat16).to(torch.float32)
    hook = lambda _m, _i, o: r(o)
    head = e.model[-1]
    with torch.no_grad():
        for mod in list(e.model)[:-1]:
            for p in mod.parameters():
                p.copy_(r(p))
        for seq in head.input_proj:
            for p in seq.parameters():
                p.copy_(r(p))
            seq.register_forward_hook(hook)
        lins = [head.enc_output[0]] + [l.cross_attn.value_proj for l in head.decoder.layers]
        for lin in lins:
            lin.weight.copy_(r(lin.weight))
            lin.register_forward_hook(hook)
    for mod in e.modules():
        if isinstance(mod, ns.modules.Conv):
            mod.register_forward_hook(hook)
    return e, r


def try_seed(tag, m, m64, seed):
    _, nc, (b, h, w) = RR.CASES[tag]
    nq, _ = RR.case_nq_ndl(tag)
    x = seeded_images(b, h, w, seed=seed)
    free = run(m, x)
    free64 = run(m64, x.double())
    sm, sm64 = free['score_max'], free64['score_max']
    d_sm = float((sm.double() - sm64).abs().max())
    idx = RR.stable_topk(sm, nq)
    idx64 = RR.stable_topk(sm64, nq)
    why = []
    _, valid = RR.anchors(RR.level_shapes(h, w), torch.float32)
    inval = set(torch.nonzero(~valid).flatten().tolist())
    L = sm.shape[1]
    margin = max(1e-5, 16 * d_sm)
    for i in range(b):
        sel, sel_ref = set(idx[i].tolist()), set(free['topk'][i].tolist())
        if inval and (inval & sel) and not inval <= sel:
            # the cut falls inside the tied group: the selection is every token above the group plus some of its (identical) tokens, and any
            # choice among them gives the same values.  Every other token must then be off the group's score by the margin, and the reference must
            # have chosen the same untied tokens and as many tied ones.
            rest = [t for t in range(L) if t not in inval]
            lead = float((sm[i, rest].double() - sm[i, sorted(inval)[0]].double()).abs().min()) if rest else float('inf')
            if lead <= margin:
                why.append(f'image {i}: a token lies {lead:.2e} from the tied group\'s score (needs > {margin:.2e})')
            if sel - inval != sel_ref - inval:
                why.append(f'image {i}: torch.topk chose other untied tokens')
        else:
            if L > nq:
                srt = torch.sort(sm[i].double(), descending=True).values
                gap = float((sm[i].double() - (srt[nq - 1] + srt[nq]) / 2).abs().min())
                if gap <= margin:
                    why.append(f'image {i}: a score_max lies {gap:.2e} from the selection boundary (needs > {margin:.2e})')
            if inval and not (inval <= sel or not (inval & sel)):
                why.append(f'image {i}: the tied invalid group straddles the selection')
            if sel != sel_ref:
                why.append(f'image {i}: the stable selection differs from torch.topk as a set')
        if sel != set(idx64[i].tolist()):
            why.append(f'image {i}: fp32 and fp64 select different sets')
    return x, idx, d_sm, len(inval), why


def run_case(arrs, tag, tmp):
    _, nc, (b, h, w) = RR.CASES[tag]
    nq, ndl = RR.case_nq_ndl(tag)
    m = build(tag, tmp)
    structure(arrs, tag, m)
    init_values(arrs, tag, tmp)
    m64 = copy.deepcopy(m).double()
    seed = RR.IMG_SEED
    while True:
        x, idx, d_sm, ninv, why = try_seed(tag, m, m64, seed)
        r = run(m, x, force=idx, want_layers=tag in RR.CHAINED)
        if tag == 'A':
            conf = r['dec_scores'].max(-1).values
            for i in range(b):
                if len(torch.unique(conf[i])) != nq:
                    why.append(f'image {i}: final confidences are not pairwise distinct')
        print(f'{tag}: image seed {seed}: d64(score_max) {d_sm:.2e}, invalid tokens {ninv}, ' + ('ok' if not why else '; '.join(why)))
        if not why:
            break
        seed += 1
        assert seed < RR.IMG_SEED + 20
    assert seed == RR.IMG_SEED, f'{tag}: the conditions hold at image seed {seed}, not rtdetr_ref.IMG_SEED = {RR.IMG_SEED}: change it'
    r64 = run(m64, x.double(), force=idx, want_inputs=tag in RR.CHAINED, want_layers=tag in RR.CHAINED)
    assert torch.equal(r['score_max'].double(), run(m, x)['score_max'].double())
    wh = torch.tensor([w, h, w, h], dtype=torch.float64)
    d = dict(box=float(((r['dec_bboxes'].double() - r64['dec_bboxes']) * wh).abs().max()),
             conf=float((r['dec_scores'].double() - r64['dec_scores']).abs().max()),
             enc_box=float(((r['enc_bboxes'].double() - r64['enc_bboxes']) * wh).abs().max()),
             enc_score=float((r['enc_scores'].double() - r64['enc_scores']).abs().max()),
             score_max=d_sm)
    print(f'{tag}: fp32 vs fp64 (indices forced) ' + '  '.join(f'{k} {v:.3e}' for k, v in d.items()))
    arrs[f'{tag}_d64'] = np.array([d[k] for k in ('box', 'conf', 'enc_box', 'enc_score', 'score_max')], np.float64)
    arrs[f'{tag}_score_max'] = r['score_max'].numpy()
    arrs[f'{tag}_topk_ref'] = r['topk'].numpy()
    arrs[f'{tag}_index'] = idx.numpy()
    arrs[f'{tag}_ninvalid'] = np.array(ninv, np.int64)
    for k in ('enc_bboxes', 'enc_scores', 'dec_bboxes', 'dec_scores'):
        arrs[f'{tag}_{k}'] = r[k].numpy()
        arrs[f'{tag}_{k}64'] = r64[k].numpy()
    arrs[f'{tag}_score_max64'] = r64['score_max'].numpy()
    if tag in RR.BF16:
        e, rnd = bf16_emulation(m)
        rb = run(e, rnd(x), force=idx)
        db = dict(box=float(((rb['dec_bboxes'] - r['dec_bboxes']).double() * wh).abs().max()),
                  conf=float((rb['dec_scores'] - r['dec_scores']).abs().max()),
                  enc_box=float(((rb['enc_bboxes'] - r['enc_bboxes']).double() * wh).abs().max()),
                  enc_score=float((rb['enc_scores'] - r['enc_scores']).abs().max()),
                  score_max=float((rb['score_max'] - r['score_max']).abs().max()))
        swapped = max(len(set(a.tolist()) - set(b_.tolist())) for a, b_ in zip(RR.stable_topk(rb['score_max'], nq), idx))
        print(f'{tag}: bf16 emulation (indices forced) ' + '  '.join(f'{k} {v:.3e}' for k, v in db.items()) + f'; free-running it would swap up to {swapped} queries')
        arrs[f'{tag}_dbf16'] = np.array([db[k] for k in ('box', 'conf', 'enc_box', 'enc_score', 'score_max')], np.float64)
    if tag in RR.CHAINED:
        arrs[f'{tag}_layers'] = r['layers'].numpy()
        arrs[f'{tag}_layers64'] = r64['layers'].numpy()
        for i, t in enumerate(r64['inputs']):
            arrs[f'{tag}_input64_{i}'] = t.numpy()
    if tag == 'A':
        conf = r['dec_scores'].max(-1).values
        thr = round(float(conf.median()), 4)
        arrs['A_pred_conf'] = np.array(thr, np.float64)
        for i in range(b):      # vit/rtdetr/predict.py:18-24 on a tensor source: no scaling
            bbox = ns.ops.xywh2xyxy(r['dec_bboxes'][i])
            score, cls = r['dec_scores'][i].max(-1, keepdim=True)
            keep = score.squeeze(-1) > thr
            rows = torch.cat([bbox, score, cls], -1)[keep]
            print(f'A: predictor rows of image {i} at conf {thr}: {len(rows)}')
            assert 5 <= len(rows) <= nq - 5
            arrs[f'A_pred_rows_{i}'] = rows.numpy()


def main():
    import yaml
    with open(os.path.join(REFY, 'yolov8-rtdetr.yaml'), errors='ignore', encoding='utf-8') as f:
        d = yaml.safe_load(f)
    with open(os.path.join(HERE, 'rtdetr_yaml.json'), 'w') as f:
        json.dump(d, f, indent=1)
        f.write('\n')
    ours = RR.case_cfg('A')
    assert ours['backbone'] == d['backbone'] and [r[:3] for r in ours['head']] == [r[:3] for r in d['head']], 'the graph table differs from the YAML'
    arrs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag in RR.CASES:
            run_case(arrs, tag, tmp)
    save(arrs)


if __name__ == '__main__':
    main()
