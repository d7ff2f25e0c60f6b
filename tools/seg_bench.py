"""Per-step times of the segmentation kernels at B = 32, 640x640, bf16, seeded weights, through SegmentationPredictor's post-processing
(NMS with mask columns at conf 0.25 / iou 0.7 / max_det 300, process_mask(upsample=True) for the whole batch).

    python tools/seg_bench.py [--models mspa_c2f_gd_yolov8-seg yolov8-seg] [--batch 32] [--imgsz 640] [--steps 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/seg_bench.py --steps 20 --no-events      # the kernels' own times

Prints one JSON line per model: HIP-event times (ops.profile, median over the steps, same process for both variants) of deconv2x2_fwd,
seg_concat_fwd, nms_masks_fwd and seg_masks_fwd, the mask kernel with tile skipping disabled (the only comparison there is), detections per
image, the bytes the mask kernel must write (sum(counts) * H * W) and read (protos once per block of 16 detections), its share of the 8 TB/s
HBM peak, and the share of (detection, tile) pairs its skip rule drops (counted on the host by ops.seg_skip_share)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgdt_yolo_amd import ops  # noqa: E402
from mgdt_yolo_amd.models import get_config  # noqa: E402
from mgdt_yolo_amd.nn.tasks import SegmentationModel  # noqa: E402
from mgdt_yolo_amd.seeding import seed_state_dict_, seeded_images  # noqa: E402
from mgdt_yolo_amd.yolo.v8.segment import SegmentationPredictor  # noqa: E402

HBM_PEAK = 8.0e12
KERNELS = ('deconv2x2_fwd', 'seg_concat_fwd', 'nms_masks_fwd', 'seg_masks_fwd')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=['mspa_c2f_gd_yolov8-seg', 'yolov8-seg'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-events', action='store_true', help='plain steps only (for a run under rocprofv3)')
    a = ap.parse_args()
    dev = 'cuda:0'
    for name in a.models:
        m = seed_state_dict_(SegmentationModel(get_config(name, 'n', 80), verbose=False), 0).eval().to(dev)
        p = SegmentationPredictor(dict(imgsz=a.imgsz, half=True, max_det=300))
        p.setup_model(m)
        x = seeded_images(a.batch, a.imgsz, a.imgsz, seed=7).to(dev).to(torch.bfloat16)
        for _ in range(a.warmup):
            res = p(x)
        torch.cuda.synchronize()
        if a.no_events:
            for skip in (True, False):
                ops.SEG_MASK_SKIP = skip
                for _ in range(a.steps):
                    p(x)
            ops.SEG_MASK_SKIP = True
            torch.cuda.synchronize()
            print(json.dumps({'model': name, 'steps': a.steps, 'note': 'first half of the seg_mask_kernel calls after warm-up: skipping on, second half: off'}))
            continue
        times = {k: [] for k in KERNELS}
        noskip = []
        for _ in range(a.steps):
            with ops.profile() as pr:
                p(x)
            for k in KERNELS:
                times[k].append(sum(ms for n, _, ms in pr.rows if n == k))
            ops.SEG_MASK_SKIP = False
            try:
                with ops.profile() as pr:
                    p(x)
            finally:
                ops.SEG_MASK_SKIP = True
            noskip.append(sum(ms for n, _, ms in pr.rows if n == 'seg_masks_fwd'))
        counts = [int(b.shape[0]) for b, _ in res]
        total = sum(counts)
        with torch.no_grad():
            cat, (_, _, proto) = p.model(x)
        from mgdt_yolo_amd.yolo.utils.ops import nms_masks_batch
        _, rows, _, cnt = nms_masks_batch(cat, 32, 0.25, 0.7, max_det=300)
        mh, mw = proto.shape[2:]
        skipped, pairs = ops.seg_skip_share(rows.cpu(), cnt, mh, mw, (a.imgsz, a.imgsz), 'process_mask_up')
        wr = total * a.imgsz * a.imgsz
        rd = sum(-(-c // 16) for c in counts) * mh * mw * 32 * 2
        med = {k: statistics.median(v) for k, v in times.items()}
        t_mask = med['seg_masks_fwd'] * 1e-3
        print(json.dumps({'model': name, 'batch': a.batch, 'imgsz': a.imgsz, 'steps': a.steps,
                          'ms': {k: round(v, 4) for k, v in med.items()}, 'seg_masks_no_skip_ms': round(statistics.median(noskip), 4),
                          'detections_per_image': round(total / a.batch, 1), 'mask_bytes_written': wr, 'mask_bytes_read': rd,
                          'mask_fraction_of_hbm_peak': round((wr + rd) / t_mask / HBM_PEAK, 4) if t_mask > 0 else None,
                          'pairs_skipped_share': round(skipped / max(pairs, 1), 4)}))


if __name__ == '__main__':
    main()
