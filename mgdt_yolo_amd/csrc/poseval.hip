// Pose validation (reference yolo/utils/metrics.py:150-169 kpt_iou, yolo/v8/pose/val.py:110-141 PoseValidator._process_batch): object keypoint
// similarity of every (label, detection) pair of a batch in one launch.
//
//   kpt_iou        oks[image][label][detection] = sum_k exp(-e_k) [vis_k != 0] / (sum_k [vis_k != 0] + eps),
//                  e_k = d_k / (2 sigma_k)^2 / (area + eps) / 2, d_k = dx^2 + dy^2.  A workgroup owns (image, KI_TD detections, KI_TL labels).  The
//                  label tile is staged in LDS as x, y, the visibility mask, coef[l][k] = 1 / ((2 sigma_k)^2 (area_l + eps) 2) and
//                  inv[l] = 1 / (count_l + eps); the detection tile's keypoints are read as ONE run of consecutive floats (the tile's rows are
//                  consecutive in memory whatever the row stride; only the keypoint columns of a row are loaded) and transposed through LDS
//                  to [k][detection] (row stride KI_SROW, odd: the strided writes spread over the banks).  A lane owns one detection, a wave
//                  KI_TL / 4 labels: the label values are wave-uniform LDS broadcasts, the detection values conflict-free reads of consecutive
//                  lanes, an invisible keypoint is skipped by a wave-uniform branch, and every output row segment is KI_TD consecutive floats.
//                  Keypoints are processed in chunks of KI_KC, so the LDS footprint (about 25 KB) does not depend on nkpt; the sum over k keeps
//                  its ascending order across chunks.
//                  Entries past nlab[i] / counts[i] are WRITTEN as zero.  A label without a visible keypoint gives 0 (sum 0 times a finite
//                  inv); a zero-area label gives coef = 1 / ((2 sigma)^2 eps 2), finite for eps > 0: e = 0 where d = 0 (the term is 1) and
//                  exp(-huge) = 0 elsewhere, never 0 * inf.
// Compiled with -ffp-contract=off: d = dx * dx + dy * dy rounds after every operation, like the reference's tensor expression.
#include "common.h"

#define KI_TD 64                   // detections per workgroup (one per lane)
#define KI_TL 16                   // labels per workgroup (4 per wave)
#define KI_KC 32                   // keypoints per LDS chunk
#define KI_SROW (KI_TD + 1)
#define KI_MAX_DET 1024            // the limits of mask_iou (segval.hip): one blocking rule serves both similarity matrices, and
#define KI_MAX_LAB 256             // val_match_iou's LDS (levels * max_lab ints) holds every matrix this kernel can write
#define KI_MAX_NKPT (POSE_MAX_NK / 2)
#define KI_MAX_STRIDE (1 << 20)    // floats between two detections: KI_TD * stride stays an int

struct KptIouArgs {
  const float* pred; const int32_t* counts; const float* gt; const float* area; const int32_t* nlab; const float* sigma; float* oks;
  int pred_stride, pred_ndim, max_det, max_lab, nkpt;
  float eps;
};

__global__ __launch_bounds__(256) void kpt_iou_kernel(const KptIouArgs a) {
  __shared__ float Px[KI_KC * KI_SROW], Py[KI_KC * KI_SROW];                 // [k][detection]
  __shared__ float Lx[KI_TL * KI_KC], Ly[KI_TL * KI_KC], Lc[KI_TL * KI_KC], Lm[KI_TL * KI_KC];     // [label][k]: x, y, coef, mask (0 / 1)
  __shared__ float Linv[KI_TL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, d0 = blockIdx.x * KI_TD, l0 = blockIdx.y * KI_TL;
  const int nd = min(max(a.counts[b], 0), a.max_det), nl = min(max(a.nlab[b], 0), a.max_lab);
  const int ndt = min(KI_TD, nd - d0), nlt = min(KI_TL, nl - l0);             // live detections / labels of this tile (<= 0: none)
  const int d = d0 + lane;
  float* out = a.oks + ((long)b * a.max_lab + l0) * a.max_det + d;
  constexpr int LPW = KI_TL / 4;
  if (ndt <= 0 || nlt <= 0) {                                                 // block-uniform: a tile of padding, before any barrier
    if (d < a.max_det) {
#pragma unroll
      for (int j = 0; j < LPW; ++j)
        if (l0 + wave + 4 * j < a.max_lab) out[(long)(wave + 4 * j) * a.max_det] = 0.f;
    }
    return;
  }
  const float* P = a.pred + ((long)b * a.max_det + d0) * (long)a.pred_stride;
  const float* G = a.gt + ((long)b * a.max_lab + l0) * a.nkpt * 3;
  const int nkd = a.nkpt * a.pred_ndim;
  if (tid < KI_TL) {                                                          // inv[l]: the visible keypoints of a label, all chunks
    float cnt = 0.f;
    if (tid < nlt)
      for (int k = 0; k < a.nkpt; ++k) cnt += G[((long)tid * a.nkpt + k) * 3 + 2] != 0.f ? 1.f : 0.f;
    Linv[tid] = 1.f / (cnt + a.eps);
  }
  float acc[LPW];
#pragma unroll
  for (int j = 0; j < LPW; ++j) acc[j] = 0.f;
  for (int k0 = 0; k0 < a.nkpt; k0 += KI_KC) {
    const int kc = min(KI_KC, a.nkpt - k0);
    __syncthreads();                                                          // the previous chunk's readers are done (first chunk: Linv is written)
    // ---- the label tile: kc * 3 consecutive floats per label, three of them per thread; entries past nlt / kc get mask 0
    for (int i = tid; i < KI_TL * KI_KC; i += 256) {
      const int l = i / KI_KC, kk = i - l * KI_KC;
      float m = 0.f;
      if (l < nlt && kk < kc) {
        const float* g = G + ((long)l * a.nkpt + k0 + kk) * 3;
        const float s2 = 2.f * a.sigma[k0 + kk];
        Lx[i] = g[0];
        Ly[i] = g[1];
        Lc[i] = 1.f / (s2 * s2 * (a.area[(long)b * a.max_lab + l0 + l] + a.eps) * 2.f);
        m = g[2] != 0.f ? 1.f : 0.f;
      }
      Lm[i] = m;
    }
    // ---- the detection tile: one run of ndt * stride floats, keypoint columns only (nothing past a row's keypoints is read)
    for (int i = tid; i < ndt * a.pred_stride; i += 256) {                    // <= 64 * 2^20: the host bounds the stride
      const int row = i / a.pred_stride, col = i - row * a.pred_stride;
      if (col >= nkd) continue;
      const int k = col / a.pred_ndim, c = col - k * a.pred_ndim, kk = k - k0;
      if (c >= 2 || kk < 0 || kk >= kc) continue;
      (c == 0 ? Px : Py)[kk * KI_SROW + row] = P[i];
    }
    __syncthreads();
    if (lane < ndt) {
      for (int kk = 0; kk < kc; ++kk) {
        const float px = Px[kk * KI_SROW + lane], py = Py[kk * KI_SROW + lane];
#pragma unroll
        for (int j = 0; j < LPW; ++j) {
          const int li = (wave + 4 * j) * KI_KC + kk;
          if (Lm[li] != 0.f) {                                                // wave-uniform
            const float dx = Lx[li] - px, dy = Ly[li] - py;
            const float dd = dx * dx + dy * dy;
            acc[j] += expf(-(dd * Lc[li]));
          }
        }
      }
    }
  }
  if (d < a.max_det) {
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int l = wave + 4 * j;
      if (l0 + l < a.max_lab) out[(long)l * a.max_det] = (lane < ndt && l < nlt) ? acc[j] * Linv[l] : 0.f;
    }
  }
}

extern "C" int mgdt_kpt_iou_fwd(const float* pred, int pred_stride, int pred_ndim, const int32_t* counts, int n, int max_det, const float* gt_kpts,
                                const float* area, const int32_t* nlab, int max_lab, int nkpt, const float* sigma, float eps, float* oks,
                                mgdt_stream s) {
  if (!pred || !counts || !gt_kpts || !area || !nlab || !sigma || !oks) MGDT_FAIL(MGDT_BAD_ARG, "kpt_iou: null pointer");
  if (n < 1 || n > 65535 || max_det < 1 || max_det > KI_MAX_DET || max_lab < 1 || max_lab > KI_MAX_LAB || nkpt < 1 || nkpt > KI_MAX_NKPT ||
      (pred_ndim != 2 && pred_ndim != 3) || pred_stride < nkpt * pred_ndim || pred_stride > KI_MAX_STRIDE)
    MGDT_FAIL(MGDT_BAD_SHAPE, "kpt_iou: n=%d (<= 65535) max_det=%d (<= %d) max_lab=%d (<= %d) nkpt=%d (<= %d) pred_ndim=%d (2 or 3) pred_stride=%d (nkpt * pred_ndim .. %d)",
              n, max_det, KI_MAX_DET, max_lab, KI_MAX_LAB, nkpt, KI_MAX_NKPT, pred_ndim, pred_stride, KI_MAX_STRIDE);
  if ((long)n * max_lab * max_det > 0x7fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "kpt_iou: n * max_lab * max_det = %ld exceeds 2^31 - 1", (long)n * max_lab * max_det);
  KptIouArgs a;
  a.pred = pred; a.counts = counts; a.gt = gt_kpts; a.area = area; a.nlab = nlab; a.sigma = sigma; a.oks = oks;
  a.pred_stride = pred_stride; a.pred_ndim = pred_ndim; a.max_det = max_det; a.max_lab = max_lab; a.nkpt = nkpt; a.eps = eps;
  kpt_iou_kernel<<<dim3(cdiv(max_det, KI_TD), cdiv(max_lab, KI_TL), n), 256, 0, (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("kpt_iou_fwd");
  return MGDT_OK;
}
