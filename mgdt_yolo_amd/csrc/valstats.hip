// Detection validation beyond mAP: the confusion matrix (reference yolo/utils/metrics.py:209-253 ConfusionMatrix.process_batch) and the counting
// metrics (reference nn/cal_counting_metrics.py:70-121, restated for nc classes) of a whole batch in one launch.
//
//   val_confusion  one workgroup per image.  The labels are staged in LDS (boxes as given for the confusion part, truncated toward zero for the
//                  counting part when asked); a lane owns one detection per trip of a block-stride loop (max_det may exceed the 256 threads) and
//                  walks the labels, which are wave-uniform LDS broadcasts.  The image's label x detection IoU matrix is never stored:
//     confusion    pass 1 (per detection with conf > cm_conf): the label of the highest box_iou > cm_iou (the first np.unique, on the detection
//                  column of the IoU-sorted pairs); pass 2: an LDS atomicMax per label on (ordered IoU bits << 32 | ~detection) keeps the
//                  highest-IoU detection among those that chose it (the second np.unique).  Not a greedy matching: a detection whose best
//                  label went to another detection does not fall back on its second best.  matrix[cls(det)][cls(label)] for a label with a
//                  winner, matrix[nc][cls(label)] otherwise; matrix[cls(det)][nc] for a kept detection that won no label, but only in an image
//                  with at least one match (the reference's `if n:`).
//     counting     per detection with conf > cnt_conf: an LDS atomicMin per same-class label with IoU > cnt_iou leaves each label the FIRST
//                  such detection in NMS order (the script's `break`); a detection may serve several labels (the script does not retire it).
//                  TP = labels with one, FN = the others, FP = p - distinct matched detections (a bit set in LDS).  Per class and image the
//                  counts t (labels) and p (detections) give the int64 sums of which MAE, RMSE and R^2 are exact functions.
//                  Exact ties (equal IoU) resolve to the lower label / detection index, where numpy's unstable argsort decides in the reference.
//                  Classes are the float columns truncated like .int(); a label or detection whose class is outside [0, nc) takes part in the
//                  matching but adds nothing (the reference raises an IndexError there).
// Both accumulators are ADDED to with integer atomics only: the result does not depend on scheduling.
// Compiled with -ffp-contract=off: the confusion pass calls the box_iou of common.h, whose operations then round one by one, as in val_match.hip.
#include "common.h"

#define VS_THREADS 256
#define VS_MAX_DET 1024
#define VS_MAX_LAB 256             // one label per thread in the label phase
#define VS_MAX_NC 4096             // two LDS histograms of nc ints
#define VS_NONE 0x7fffffff

struct ValStatsArgs {
  const float* det; const int32_t* ndet; const float* lab; const int32_t* nlab;
  int32_t* matrix; long long* counts;
  int max_det, max_lab, nc, trunc;
  float cm_conf, cm_iou, cnt_conf, cnt_iou;
};

// float -> unsigned with the same order (negative values below positive ones)
__device__ __forceinline__ uint32_t vs_ordered(float f) {
  const uint32_t b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ void vs_add(long long* p, long long v) {
  if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

__global__ __launch_bounds__(VS_THREADS) void val_confusion_kernel(const ValStatsArgs a) {
  __shared__ float Lb[VS_MAX_LAB * 4];                     // label boxes as given
  __shared__ float Lt[VS_MAX_LAB * 4];                     // label boxes of the counting part
  __shared__ int Lc[VS_MAX_LAB];                           // label class, -1 outside [0, nc)
  __shared__ unsigned long long winner[VS_MAX_LAB];        // confusion pass 2: 0 = nobody chose the label
  __shared__ int first[VS_MAX_LAB];                        // counting: first matching detection
  __shared__ short choice[VS_MAX_DET];                     // confusion pass 1: label chosen by a detection, -1 none, -2 below cm_conf
  __shared__ uint32_t used[VS_MAX_DET / 32];               // counting: detections that served a label
  __shared__ int any_match;
  extern __shared__ int hist[];                            // counting: [nc] t | TP << 10 | distinct << 20 of the labels, [nc] p
  const int img = blockIdx.x, tid = threadIdx.x, nc = a.nc;
  const int nd = min(max(a.ndet[img], 0), a.max_det), nl = min(max(a.nlab[img], 0), a.max_lab);
  const float* D = a.det + (long)img * a.max_det * 6;
  const float* L = a.lab + (long)img * a.max_lab * 5;
  const bool do_cm = a.matrix != nullptr, do_cnt = a.counts != nullptr;
  int* hl = hist;
  int* hp = hist + nc;

  for (int l = tid; l < nl; l += VS_THREADS) {
    const int c = (int)L[l * 5];
    Lc[l] = (c >= 0 && c < nc) ? c : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = L[l * 5 + 1 + k];
      Lb[l * 4 + k] = v;
      Lt[l * 4 + k] = a.trunc ? truncf(v) : v;
    }
    winner[l] = 0ull;
    first[l] = VS_NONE;
  }
  if (tid < VS_MAX_DET / 32) used[tid] = 0u;
  if (tid == 0) any_match = 0;
  if (do_cnt)
    for (int i = tid; i < 2 * nc; i += VS_THREADS) hist[i] = 0;
  __syncthreads();

  // ---- detections: the best label of each (confusion), the first detection of each label (counting)
  for (int d = tid; d < nd; d += VS_THREADS) {
    const float x1 = D[d * 6], y1 = D[d * 6 + 1], x2 = D[d * 6 + 2], y2 = D[d * 6 + 3], conf = D[d * 6 + 4];
    const int dc = (int)D[d * 6 + 5];
    const bool keep_cm = do_cm && conf > a.cm_conf;
    const bool keep_cnt = do_cnt && conf > a.cnt_conf && dc >= 0 && dc < nc;
    if (keep_cnt) atomicAdd(&hp[dc], 1);
    const float area_d = (x2 - x1) * (y2 - y1);
    int best = -1;
    float bestv = 0.f;
    for (int l = 0; l < nl; ++l) {
      if (keep_cm) {
        const float iou = box_iou(Lb[l * 4], Lb[l * 4 + 1], Lb[l * 4 + 2], Lb[l * 4 + 3], x1, y1, x2, y2, area_d);
        if (iou > a.cm_iou && (best < 0 || iou > bestv)) { bestv = iou; best = l; }
      }
      if (keep_cnt && Lc[l] == dc) {
        const float lx1 = Lt[l * 4], ly1 = Lt[l * 4 + 1], lx2 = Lt[l * 4 + 2], ly2 = Lt[l * 4 + 3];
        const float inter = fmaxf(0.f, fminf(lx2, x2) - fmaxf(lx1, x1)) * fmaxf(0.f, fminf(ly2, y2) - fmaxf(ly1, y1));
        const float uni = (lx2 - lx1) * (ly2 - ly1) + area_d - inter;
        const float iou = uni > 0.f ? inter / uni : 0.f;
        if (iou > a.cnt_iou) atomicMin(&first[l], d);
      }
    }
    choice[d] = keep_cm ? (short)best : (short)-2;
    if (best >= 0) atomicMax(&winner[best], ((unsigned long long)vs_ordered(bestv) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)d));
  }
  __syncthreads();

  // ---- labels
  for (int l = tid; l < nl; l += VS_THREADS) {
    const int lc = Lc[l];
    if (do_cm) {
      const unsigned long long w = winner[l];
      if (w) {
        atomicOr(&any_match, 1);
        const int d = (int)(0xffffffffu - (uint32_t)w);
        const int dc = (int)D[d * 6 + 5];
        if (lc >= 0 && dc >= 0 && dc < nc) atomicAdd(&a.matrix[dc * (nc + 1) + lc], 1);
      } else if (lc >= 0) {
        atomicAdd(&a.matrix[nc * (nc + 1) + lc], 1);
      }
    }
    if (do_cnt && lc >= 0) {
      const int f = first[l];
      int add = 1;
      if (f != VS_NONE) {
        const uint32_t bit = 1u << (f & 31);
        add += 1 << 10;
        if (!(atomicOr(&used[f >> 5], bit) & bit)) add += 1 << 20;
      }
      atomicAdd(&hl[lc], add);
    }
  }
  __syncthreads();

  // ---- predicted background: kept detections that won no label, in an image with at least one match
  if (do_cm && any_match) {
    for (int d = tid; d < nd; d += VS_THREADS) {
      const int c = choice[d];
      if (c == -2) continue;
      if (c >= 0 && (int)(0xffffffffu - (uint32_t)winner[c]) == d) continue;
      const int dc = (int)D[d * 6 + 5];
      if (dc >= 0 && dc < nc) atomicAdd(&a.matrix[dc * (nc + 1) + nc], 1);
    }
  }
  // ---- the image's counts of every class
  if (do_cnt) {
    for (int c = tid; c < nc; c += VS_THREADS) {
      const int h = hl[c];
      const long long t = h & 1023, tp = (h >> 10) & 1023, dist = (h >> 20) & 1023, p = hp[c];
      long long* o = a.counts + (long)c * MGDT_COUNT_SLOTS;
      const long long diff = t - p;
      vs_add(o + 0, 1);
      vs_add(o + 1, t);
      vs_add(o + 2, p);
      vs_add(o + 3, t * t);
      vs_add(o + 4, t * p);
      vs_add(o + 5, diff * diff);
      vs_add(o + 6, diff < 0 ? -diff : diff);
      vs_add(o + 7, tp);
      vs_add(o + 8, p - dist);
      vs_add(o + 9, t - tp);
    }
  }
}

extern "C" int mgdt_val_confusion_fwd(const float* det, const int32_t* ndet, int n, int max_det, const float* labels, const int32_t* nlab, int max_lab,
                                      int nc, float cm_conf, float cm_iou, float cnt_conf, float cnt_iou, int cnt_trunc_labels, int32_t* matrix,
                                      int64_t* counts, mgdt_stream s) {
  if (!det || !ndet || !labels || !nlab) MGDT_FAIL(MGDT_BAD_ARG, "val_confusion: null pointer");
  if (!matrix && !counts) MGDT_FAIL(MGDT_BAD_ARG, "val_confusion: neither a matrix nor counts to add to");
  if (n < 1 || n > 65535 || max_det < 1 || max_det > VS_MAX_DET || max_lab < 1 || max_lab > VS_MAX_LAB || nc < 1 || nc > VS_MAX_NC)
    MGDT_FAIL(MGDT_BAD_SHAPE, "val_confusion: n=%d (1 .. 65535) max_det=%d (1 .. %d) max_lab=%d (1 .. %d) nc=%d (1 .. %d)", n, max_det, VS_MAX_DET,
              max_lab, VS_MAX_LAB, nc, VS_MAX_NC);
  static_assert(sizeof(long long) == sizeof(int64_t), "int64 slots");
  ValStatsArgs a;
  a.det = det; a.ndet = ndet; a.lab = labels; a.nlab = nlab; a.matrix = matrix; a.counts = (long long*)counts;
  a.max_det = max_det; a.max_lab = max_lab; a.nc = nc; a.trunc = cnt_trunc_labels != 0;
  a.cm_conf = cm_conf; a.cm_iou = cm_iou; a.cnt_conf = cnt_conf; a.cnt_iou = cnt_iou;
  const size_t lds = counts ? (size_t)2 * nc * sizeof(int) : 0;      // <= 32 KiB beside about 13 KiB of static LDS
  val_confusion_kernel<<<n, VS_THREADS, lds, (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("val_confusion_fwd");
  return MGDT_OK;
}
