// Validator matching (reference yolo/v8/detect/val.py:152-175 DetectionValidator._process_batch, and its segmentation / pose forms on a mask-IoU or
// OKS matrix) for a whole batch: one workgroup per image, one kernel template over the source of the similarity of (label l, detection d).
//   per IoU level t: best[d] = label with the largest similarity among {similarity >= level, same class};  a label keeps the LOWEST-INDEX detection
//   that chose it (np.unique(det) then np.unique(label) without the re-sort, as the fork is written);  correct[d][t] = d is kept.
// Exact ties between two labels of one detection (numpy's unstable argsort decides in the reference) resolve to the lower label index.
//   VmBoxes   box_iou(labels, detections) (metrics.py:52-72: common.h; this file is built with -ffp-contract=off) from the 6-float detection and
//             5-float label rows; the detection's box and area stay in registers
//   VmMatrix  iou[image][label][detection] as given (coalesced over detections); the classes are read through two strides
#include "common.h"

#define VM_T 16      // max IoU levels

struct VmBoxes {
  const float* det; const float* lab;     // [n][max_det][6], [n][max_lab][5]
  struct Det { float x1, y1, x2, y2, area, cls; };
  __device__ __forceinline__ void image(int img, int max_det, int max_lab) { det += (long)img * max_det * 6; lab += (long)img * max_lab * 5; }
  __device__ __forceinline__ Det load(int d) const {
    const float x1 = det[d * 6], y1 = det[d * 6 + 1], x2 = det[d * 6 + 2], y2 = det[d * 6 + 3];
    return {x1, y1, x2, y2, (x2 - x1) * (y2 - y1), det[d * 6 + 5]};
  }
  __device__ __forceinline__ float cls(int l) const { return lab[l * 5]; }
  __device__ __forceinline__ float sim(const Det& q, int l, int) const {
    return box_iou(lab[l * 5 + 1], lab[l * 5 + 2], lab[l * 5 + 3], lab[l * 5 + 4], q.x1, q.y1, q.x2, q.y2, q.area);
  }
};

struct VmMatrix {
  const float* iou; const float* det_cls; const float* lab_cls;     // [n][max_lab][max_det]; the class of detection 0 / label 0 of image 0
  int det_stride, lab_stride;                                       // floats from one detection / label to the next
  struct Det { int d; float cls; };
  __device__ __forceinline__ void image(int img, int max_det, int max_lab) {
    iou += (long)img * max_lab * max_det; det_cls += (long)img * max_det * det_stride; lab_cls += (long)img * max_lab * lab_stride;
  }
  __device__ __forceinline__ Det load(int d) const { return {d, det_cls[(long)d * det_stride]}; }
  __device__ __forceinline__ float cls(int l) const { return lab_cls[(long)l * lab_stride]; }
  __device__ __forceinline__ float sim(const Det& q, int l, int max_det) const { return iou[(long)l * max_det + q.d]; }
};

template <class Src>
__global__ __launch_bounds__(256) void val_match_kernel(Src src, const int32_t* __restrict__ ndet, int max_det, const int32_t* __restrict__ nlab, int max_lab,
                                                        const float* __restrict__ iouv, int T, uint8_t* __restrict__ correct) {
  extern __shared__ int winner[];     // [T][max_lab]: lowest detection index that chose the label
  const int img = blockIdx.x, tid = threadIdx.x;
  const int nd = min(ndet[img], max_det), nl = min(nlab[img], max_lab);
  src.image(img, max_det, max_lab);
  uint8_t* C = correct + (long)img * max_det * T;
  for (int i = tid; i < T * max_lab; i += 256) winner[i] = 0x7fffffff;
  __syncthreads();
  for (int d0 = 0; d0 < max_det; d0 += 256) {     // uniform trip count: barriers inside
    const int d = d0 + tid;
    int best[VM_T];
    float bestv[VM_T];
#pragma unroll
    for (int t = 0; t < VM_T; ++t) { best[t] = -1; bestv[t] = -1.f; }
    if (d < nd) {
      const typename Src::Det q = src.load(d);
      for (int l = 0; l < nl; ++l) {
        if (src.cls(l) != q.cls) continue;
        const float v = src.sim(q, l, max_det);
#pragma unroll
        for (int t = 0; t < VM_T; ++t)
          if (t < T && v >= iouv[t] && v > bestv[t]) { bestv[t] = v; best[t] = l; }
      }
#pragma unroll
      for (int t = 0; t < VM_T; ++t)
        if (t < T && best[t] >= 0) atomicMin(&winner[t * max_lab + best[t]], d);
    }
    __syncthreads();
    // detections of later rounds have larger indices: a winner found in this round is final
    if (d < max_det) {
#pragma unroll
      for (int t = 0; t < VM_T; ++t)
        if (t < T) C[d * T + t] = (d < nd && best[t] >= 0 && winner[t * max_lab + best[t]] == d) ? 1 : 0;
    }
    __syncthreads();
  }
}

extern "C" int mgdt_val_match_fwd(const float* det, const int32_t* ndet, int n, int max_det, const float* labels, const int32_t* nlab, int max_lab,
                                  const float* iouv, int n_iou, uint8_t* correct, mgdt_stream s) {
  if (!det || !ndet || !labels || !nlab || !iouv || !correct) MGDT_FAIL(MGDT_BAD_ARG, "val_match: null pointer");
  if (n < 1 || max_det < 1 || max_lab < 1 || n_iou < 1 || n_iou > VM_T || (size_t)n_iou * max_lab * sizeof(int) > 64 * 1024)
    MGDT_FAIL(MGDT_BAD_SHAPE, "val_match: n=%d max_det=%d max_lab=%d n_iou=%d (<= %d levels, levels*max_lab <= 16384)", n, max_det, max_lab, n_iou, VM_T);
  val_match_kernel<<<n, 256, (size_t)n_iou * max_lab * sizeof(int), (hipStream_t)s>>>(VmBoxes{det, labels}, ndet, max_det, nlab, max_lab, iouv, n_iou, correct);
  MGDT_CHECK_LAUNCH("val_match_fwd");
  return MGDT_OK;
}

extern "C" int mgdt_val_match_iou_fwd(const float* iou, int n, int max_lab, int max_det, const float* det_cls, int det_stride, const int32_t* ndet,
                                      const float* lab_cls, int lab_stride, const int32_t* nlab, const float* iouv, int n_iou, uint8_t* correct,
                                      mgdt_stream s) {
  if (!iou || !det_cls || !ndet || !lab_cls || !nlab || !iouv || !correct) MGDT_FAIL(MGDT_BAD_ARG, "val_match_iou: null pointer");
  if (n < 1 || max_det < 1 || max_lab < 1 || det_stride < 1 || lab_stride < 1 || n_iou < 1 || n_iou > VM_T ||
      (size_t)n_iou * max_lab * sizeof(int) > 64 * 1024)
    MGDT_FAIL(MGDT_BAD_SHAPE, "val_match_iou: n=%d max_det=%d max_lab=%d strides %d / %d n_iou=%d (<= %d levels, levels*max_lab <= 16384)", n, max_det,
              max_lab, det_stride, lab_stride, n_iou, VM_T);
  val_match_kernel<<<n, 256, (size_t)n_iou * max_lab * sizeof(int), (hipStream_t)s>>>(VmMatrix{iou, det_cls, lab_cls, det_stride, lab_stride}, ndet, max_det, nlab,
                                                                                       max_lab, iouv, n_iou, correct);
  MGDT_CHECK_LAUNCH("val_match_iou_fwd");
  return MGDT_OK;
}
