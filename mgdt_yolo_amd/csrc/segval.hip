// Instance-segmentation validation (reference yolo/v8/segment/val.py:131-166 SegmentationValidator._process_batch, yolo/utils/metrics.py:131-147
// mask_iou): mask IoU of every (label, detection) pair of a batch, ground truth brought to the predictions' resolution.  The matching from the IoU
// matrix is val_match.hip's.
//
//   mask_iou       inter[image][label][detection] = sum over pixels of gt * pred on the 0 / 1 mask BYTES with v_mfma_i32_16x16x64_i8: the labels are
//                  the M rows (A operand), 16 detections the N columns (B operand), pixels are K.  A wave owns (image, 16 detections, a K range) and
//                  all label tiles of the image; a step covers 256 pixels: lane (c, g) loads the 64-byte run [256 s + 64 g, + 64) of detection c with
//                  four 16-byte loads and uses piece i as the B fragment of MFMA i.  The A fragment of lane (r, g) is the SAME four pieces of label
//                  row r, so whatever order the instruction gives the 64 k-values of a fragment, both operands agree (the order of K inside a dot
//                  product is free).  Index-map ground truth (one uint8 map per image, value j + 1 = label j) is expanded in registers: the 16 bytes
//                  of the map under a piece are compared with the lane's own label number by a carry-free byte-equality expression (4 pixels per
//                  VALU op); the (nl, H, W) repeat of the reference is never written anywhere.  Instance ground truth is loaded like the predictions.
//                  Areas are v_dot4_u32_u8 sums of the same registers.  Partial sums of the K ranges are combined with integer vector atomics in a
//                  zeroed workspace (order-independent, exact); a second small kernel turns them into
//                  iou = inter / ((area_gt + area_pred) - inter + eps) in float32 (IEEE division), bit-equal to the reference's float32 matmul, whose
//                  0 / 1 sums are exact below 2^24.  Every predicted mask byte is read once.
//   gt_resample    F.interpolate(bilinear, align_corners=False) + > 0.5 of each binary ground-truth mask (val.py:146-148), from either form, written as
//                  instance masks at the predictions' size (the weights of seg_tap in segment.hip: PyTorch's CPU arithmetic).
#include "common.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;

#define MI_MAX_LAB 256             // label rows of one image (16 MFMA tiles); the index map holds at most 255 labels (uint8, 0 = background)
#define MI_MAX_DET 1024            // detections of one image
#define MI_MAX_HW (1 << 24)        // pixels of one mask: int32 sums and their float32 images stay exact
#define MI_STEP 256                // pixels per wave step

struct MaskIouArgs {
  const uint8_t* pred; const int32_t* counts; const int32_t* offsets;
  const uint8_t* gt; const int32_t* nlab; const int32_t* lab_off;
  int32_t* inter; int32_t* area_p; int32_t* area_g;       // [n][LP][DP], [n][DP], [n][LP]
  int max_det, max_lab, DP, LP, hw, index_map, vec, steps_per_split;
};

// 16 mask bytes at p (n_valid of them inside the mask; the rest read as 0)
__device__ __forceinline__ i32x4 mi_load16(const uint8_t* p, int n_valid, int vec) {
  if (n_valid >= 16 && vec) return *(const i32x4*)p;
  i32x4 v = {0, 0, 0, 0};
  if (n_valid > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned w = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < n_valid) w |= (unsigned)p[4 * q + e] << (8 * e);
      v[q] = (int)w;
    }
  }
  return v;
}

// per byte: 1 where x == rep, else 0.  y | 0x80 >= 0x80 in every byte, so the subtraction never borrows across bytes.
__device__ __forceinline__ int mi_eq_bytes(int x, unsigned rep) {
  const unsigned y = (unsigned)x ^ rep;
  const unsigned t = (y | 0x80808080u) - 0x01010101u;
  return (int)((~(t | y) & 0x80808080u) >> 7);
}

__device__ __forceinline__ unsigned mi_ones(const i32x4 v, unsigned acc) {
#pragma unroll
  for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_udot4((unsigned)v[q], 0x01010101u, acc, false);
  return acc;
}

template <int LT>
__global__ __launch_bounds__(256) void mask_iou_kernel(const MaskIouArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, tile = blockIdx.y * 4 + wave;
  const int nd = min(a.counts[b], a.max_det), nl = min(a.nlab[b], a.max_lab);
  if (tile * 16 >= nd || nl < 1) return;                      // wave-uniform; the kernel has no barrier
  const int c = lane & 15, g = lane >> 4;
  const int lt = (nl + 15) >> 4;
  const int hw = a.hw, vec = a.vec;
  const uint8_t* P = a.pred + ((long)a.offsets[b] + min(tile * 16 + c, nd - 1)) * hw;
  const uint8_t* G = a.gt + (a.index_map ? (long)b : (long)a.lab_off[b]) * hw;
  i32x4 acc[LT];
  unsigned ag[LT], ap = 0;
#pragma unroll
  for (int t = 0; t < LT; ++t) { acc[t] = i32x4{0, 0, 0, 0}; ag[t] = 0; }
  const int k_begin = blockIdx.x * a.steps_per_split * MI_STEP;
  const int k_end = min(hw, k_begin + a.steps_per_split * MI_STEP);
  for (int k0 = k_begin; k0 < k_end; k0 += MI_STEP) {
    const int p = k0 + 64 * g;
    i32x4 bf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bf[i] = mi_load16(P + p + 16 * i, hw - (p + 16 * i), vec);
#pragma unroll
    for (int i = 0; i < 4; ++i) ap = mi_ones(bf[i], ap);
    if (a.index_map) {
      i32x4 ix[4];                                             // the 16 lanes of a group read the same bytes
#pragma unroll
      for (int i = 0; i < 4; ++i) ix[i] = mi_load16(G + p + 16 * i, hw - (p + 16 * i), vec);
#pragma unroll
      for (int t = 0; t < LT; ++t) {
        if (t < lt) {
          const int row = 16 * t + c;
          const unsigned rep = (unsigned)(row + 1) * 0x01010101u;
          const int keep = row < nl ? -1 : 0;                  // row 255 would wrap to the background value
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            i32x4 af;
#pragma unroll
            for (int q = 0; q < 4; ++q) af[q] = mi_eq_bytes(ix[i][q], rep) & keep;
            acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[i], acc[t], 0, 0, 0);
            if (tile == 0) ag[t] = mi_ones(af, ag[t]);
          }
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < LT; ++t) {
        if (t < lt) {
          const uint8_t* A = G + (long)min(16 * t + c, nl - 1) * hw + p;
          i32x4 af[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = mi_load16(A + 16 * i, hw - (p + 16 * i), vec);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf[i], acc[t], 0, 0, 0);
            if (tile == 0) ag[t] = mi_ones(af[i], ag[t]);
          }
        }
      }
    }
  }
  // D: column (detection) lane & 15, rows (labels) 4 g + e
  const int d = tile * 16 + c;
  if (d < nd) {
    if (ap) atomicAdd(&a.area_p[(long)b * a.DP + d], (int)ap);
#pragma unroll
    for (int t = 0; t < LT; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int l = 16 * t + 4 * g + e;
        if (t < lt && l < nl && acc[t][e]) atomicAdd(&a.inter[((long)b * a.LP + l) * a.DP + d], acc[t][e]);
      }
    }
  }
  if (tile == 0) {
#pragma unroll
    for (int t = 0; t < LT; ++t) {
      const int l = 16 * t + c;                                // the A fragment's row: label l, this lane group's quarter of the pixels
      if (t < lt && l < nl && ag[t]) atomicAdd(&a.area_g[(long)b * a.LP + l], (int)ag[t]);
    }
  }
}

__global__ __launch_bounds__(256) void mask_iou_final_kernel(const MaskIouArgs a, int n, float eps, float* __restrict__ iou) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)a.max_lab * a.max_det;
  if (i >= per * n) return;
  const int b = (int)(i / per), r = (int)(i - (long)b * per), l = r / a.max_det, d = r - l * a.max_det;
  const int nd = min(a.counts[b], a.max_det), nl = min(a.nlab[b], a.max_lab);
  float v = 0.f;
  if (l < nl && d < nd) {
    const float inter = (float)a.inter[((long)b * a.LP + l) * a.DP + d];
    const float uni = ((float)a.area_g[(long)b * a.LP + l] + (float)a.area_p[(long)b * a.DP + d]) - inter;
    v = inter / (uni + eps);
  }
  iou[i] = v;
}

static inline int round16(int x) { return (x + 15) / 16 * 16; }

extern "C" size_t mgdt_mask_iou_workspace_bytes(int n, int max_det, int max_lab) {
  if (n < 1 || max_det < 1 || max_lab < 1) return 0;
  const size_t dp = round16(max_det), lp = round16(max_lab);
  return (size_t)n * (lp * dp + dp + lp) * sizeof(int32_t);
}

extern "C" int mgdt_mask_iou_fwd(const uint8_t* pred, const int32_t* counts, const int32_t* offsets, int n, int max_det, const uint8_t* gt,
                                 int gt_index_map, const int32_t* nlab, const int32_t* lab_offsets, int max_lab, int hw, float eps, float* iou,
                                 void* ws, size_t ws_bytes, mgdt_stream s) {
  if (!pred || !counts || !offsets || !gt || !nlab || !iou || !ws || (!gt_index_map && !lab_offsets)) MGDT_FAIL(MGDT_BAD_ARG, "mask_iou: null pointer");
  if (n < 1 || n > 65535 || max_det < 1 || max_det > MI_MAX_DET || max_lab < 1 || max_lab > (gt_index_map ? MI_MAX_LAB - 1 : MI_MAX_LAB) || hw < 1 ||
      hw > MI_MAX_HW)
    MGDT_FAIL(MGDT_BAD_SHAPE, "mask_iou: n=%d (<= 65535) max_det=%d (<= %d) max_lab=%d (<= %d; %d as an index map) hw=%d (<= %d)", n, max_det, MI_MAX_DET,
              max_lab, MI_MAX_LAB, MI_MAX_LAB - 1, hw, MI_MAX_HW);
  if ((long)n * max_lab * max_det > 0x7fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "mask_iou: n * max_lab * max_det = %ld exceeds 2^31 - 1", (long)n * max_lab * max_det);
  if (ws_bytes < mgdt_mask_iou_workspace_bytes(n, max_det, max_lab)) MGDT_FAIL(MGDT_BAD_ARG, "mask_iou: workspace of %zu bytes is too small", ws_bytes);
  MaskIouArgs a;
  a.pred = pred; a.counts = counts; a.offsets = offsets; a.gt = gt; a.nlab = nlab; a.lab_off = lab_offsets;
  a.max_det = max_det; a.max_lab = max_lab; a.DP = round16(max_det); a.LP = round16(max_lab); a.hw = hw; a.index_map = gt_index_map ? 1 : 0;
  a.vec = hw % 16 == 0 && (((uintptr_t)pred | (uintptr_t)gt) & 15) == 0;
  a.inter = (int32_t*)ws; a.area_p = a.inter + (size_t)n * a.LP * a.DP; a.area_g = a.area_p + (size_t)n * a.DP;
  const int tiles = a.DP / 16, groups = cdiv(tiles, 4), steps = cdiv(hw, MI_STEP);
  // K ranges: enough waves to fill the machine (about 8192), at least 4 steps each
  int splits = std::max(1, std::min(cdiv(8192, (long)n * tiles), std::max(1, steps / 4)));
  a.steps_per_split = cdiv(steps, splits);
  splits = cdiv(steps, a.steps_per_split);
  if (hipMemsetAsync(ws, 0, mgdt_mask_iou_workspace_bytes(n, max_det, max_lab), (hipStream_t)s) != hipSuccess)
    MGDT_FAIL(MGDT_LAUNCH_FAIL, "mask_iou: clearing the workspace failed");
  const dim3 grid(splits, groups, n);
  const int lt = a.LP / 16;
  if (lt <= 1) mask_iou_kernel<1><<<grid, 256, 0, (hipStream_t)s>>>(a);
  else if (lt <= 2) mask_iou_kernel<2><<<grid, 256, 0, (hipStream_t)s>>>(a);
  else if (lt <= 4) mask_iou_kernel<4><<<grid, 256, 0, (hipStream_t)s>>>(a);
  else if (lt <= 8) mask_iou_kernel<8><<<grid, 256, 0, (hipStream_t)s>>>(a);
  else mask_iou_kernel<16><<<grid, 256, 0, (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("mask_iou_fwd");
  mask_iou_final_kernel<<<cdiv((long)n * max_lab * max_det, 256), 256, 0, (hipStream_t)s>>>(a, n, eps, iou);
  MGDT_CHECK_LAUNCH("mask_iou_fwd (final)");
  return MGDT_OK;
}

// ================================================================================================ ground truth at the predictions' size
struct GtResampleArgs {
  const uint8_t* gt; const int32_t* nlab; const int32_t* lab_off; uint8_t* out;
  int index_map, max_lab, h, w, oh, ow;
  float sy, sx;
};

__device__ __forceinline__ void gr_tap(float scale, int o, int n_in, int& i0, int& i1, float& w1) {     // == seg_tap (segment.hip)
  const float s = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, n_in - 1);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  w1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

__global__ __launch_bounds__(256) void gt_resample_kernel(const GtResampleArgs a) {
  const int b = blockIdx.z, l = blockIdx.y;
  if (l >= min(a.nlab[b], a.max_lab)) return;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.oh * a.ow) return;
  const int oy = o / a.ow, ox = o - oy * a.ow;
  int y0, y1, x0, x1;
  float h1, w1;
  gr_tap(a.sy, oy, a.h, y0, y1, h1);
  gr_tap(a.sx, ox, a.w, x0, x1, w1);
  const float h0 = 1.f - h1, w0 = 1.f - w1;
  const long plane = (long)a.h * a.w;
  const uint8_t* src = a.gt + (a.index_map ? (long)b : (long)a.lab_off[b] + l) * plane;
  const int want = a.index_map ? l + 1 : 1;
  auto at = [&](int y, int x) { return src[(long)y * a.w + x] == want ? 1.f : 0.f; };
  const float v = (at(y0, x0) * w0 + at(y0, x1) * w1) * h0 + (at(y1, x0) * w0 + at(y1, x1) * w1) * h1;
  a.out[((long)a.lab_off[b] + l) * a.oh * a.ow + o] = v > 0.5f ? 1 : 0;
}

extern "C" int mgdt_gt_masks_resample_fwd(const uint8_t* gt, int gt_index_map, const int32_t* nlab, const int32_t* lab_offsets, int n, int max_lab, int h,
                                          int w, int out_h, int out_w, uint8_t* out, mgdt_stream s) {
  if (!gt || !nlab || !lab_offsets || !out) MGDT_FAIL(MGDT_BAD_ARG, "gt_masks_resample: null pointer");
  if (n < 1 || n > 65535 || max_lab < 1 || max_lab > (gt_index_map ? MI_MAX_LAB - 1 : MI_MAX_LAB) || h < 1 || w < 1 || out_h < 1 || out_w < 1 ||
      (long)h * w > MI_MAX_HW || (long)out_h * out_w > MI_MAX_HW)
    MGDT_FAIL(MGDT_BAD_SHAPE, "gt_masks_resample: n=%d max_lab=%d (<= %d; %d as an index map) %dx%d -> %dx%d (<= %d pixels)", n, max_lab, MI_MAX_LAB,
              MI_MAX_LAB - 1, h, w, out_h, out_w, MI_MAX_HW);
  GtResampleArgs a;
  a.gt = gt; a.nlab = nlab; a.lab_off = lab_offsets; a.out = out; a.index_map = gt_index_map ? 1 : 0; a.max_lab = max_lab;
  a.h = h; a.w = w; a.oh = out_h; a.ow = out_w; a.sy = (float)h / (float)out_h; a.sx = (float)w / (float)out_w;
  gt_resample_kernel<<<dim3(cdiv((long)out_h * out_w, 256), max_lab, n), 256, 0, (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("gt_masks_resample_fwd");
  return MGDT_OK;
}
