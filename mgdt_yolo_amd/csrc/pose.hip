// Pose-estimation inference (reference nn/modules/head.py:215-253 Pose / kpts_decode, yolo/v8/pose/predict.py:16-41,
// yolo/utils/ops.py:90-117 scale_boxes, :636-666 scale_coords / clip_coords).
//
//   pose_concat    (B, 4+nc, A) prediction of Detect + the per-level NHWC cv4 maps (nk keypoint channels per pixel, pixel stride >= nk: the
//                  padded-MFMA route leaves 52 channels for nk = 51) -> the (B, 4+nc+nk, A) prediction with the keypoints decoded
//                  (kpts_decode's non-export branch, fp32, the reference's operation order) and the raw (B, nk, A) keypoint map, one launch for
//                  all levels.  The inputs are channel-major (a pixel's channels are consecutive), the outputs anchor-major: a workgroup owns
//                  POSE_TA consecutive anchors, reads their pixels as consecutive 4-channel pieces (16 bytes fp32 / 8 bytes bf16 per lane,
//                  consecutive lanes -> consecutive pieces of one pixel), transposes through LDS, and writes every output row as POSE_TA
//                  consecutive floats.  The last workgroup's tail anchors are masked; anchors of one workgroup may lie in two levels.
//   pose_scale     the predictor's post-NMS step for a batch in one launch, in place on the padded NMS rows: boxes scale_boxes + clip + round
//                  half-to-even (torch.round), keypoint x / y scale_coords + clip_coords, confidence / class / visibility columns untouched.
// Compiled with -ffp-contract=off: the arithmetic is the reference's expression order in IEEE fp32.
#include "common.h"

#define POSE_MAX_LEVELS 4
#define POSE_TA 64                 // anchors per workgroup
#define POSE_SROW (POSE_TA + 1)    // LDS row stride (floats): odd, so the channel-major phase-1 writes spread over the banks

struct PoseCatArgs {
  const float* y; float* out; float* raw;
  const void* kp[POSE_MAX_LEVELS];
  long sn[POSE_MAX_LEVELS], sh[POSE_MAX_LEVELS], sp[POSE_MAX_LEVELS];   // level maps: image / row / pixel stride (elements)
  int lw[POSE_MAX_LEVELS], a_off[POSE_MAX_LEVELS + 1];
  float stride[POSE_MAX_LEVELS];
  int B, rows, nk, ndim, A, levels, vec;
};

template <typename T>
__global__ __launch_bounds__(256) void pose_concat_kernel(const PoseCatArgs a) {
  extern __shared__ __attribute__((aligned(16))) float S[];              // [nk][POSE_SROW] raw keypoint values of the tile
  const int tid = threadIdx.x, b = blockIdx.y, a0 = blockIdx.x * POSE_TA;
  const int na = min(POSE_TA, a.A - a0);                                  // anchors of this tile (tail tile: fewer)
  // ---- copied rows: 4 + nc rows of POSE_TA consecutive floats
  {
    const float* src = a.y + (long)b * a.rows * a.A + a0;
    float* dst = a.out + (long)b * (a.rows + a.nk) * a.A + a0;
    for (int i = tid; i < a.rows * POSE_TA; i += 256) {
      const int r = i / POSE_TA, c = i - r * POSE_TA;
      if (c < na) dst[(long)r * a.A + c] = src[(long)r * a.A + c];
    }
  }
  // ---- phase 1: channel-major reads -> LDS
  const int nk4 = (a.nk + 3) >> 2;
  for (int i = tid; i < POSE_TA * nk4; i += 256) {
    const int la = i / nk4, g = i - la * nk4;
    if (la >= na) continue;
    const int an = a0 + la;
    int l = 0;
    while (l + 1 < a.levels && an >= a.a_off[l + 1]) ++l;
    const int pix = an - a.a_off[l], py = pix / a.lw[l], px = pix - py * a.lw[l];
    const T* m = (const T*)a.kp[l] + (long)b * a.sn[l] + (long)py * a.sh[l] + (long)px * a.sp[l] + 4 * g;
    if (a.vec) {                                   // the pixel holds 4 * nk4 readable, 4-element aligned channels (checked by the host)
      const f32x4 v = load4<T>(m);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * g + e < a.nk) S[(4 * g + e) * POSE_SROW + la] = v[e];
    } else {
      for (int e = 0; e < 4; ++e)
        if (4 * g + e < a.nk) S[(4 * g + e) * POSE_SROW + la] = ldf<T>(m + e);
    }
  }
  __syncthreads();
  // ---- phase 2: anchor-major writes; thread -> one fixed anchor of the tile, channels tid / 64, + 4, ...
  const int la = tid & (POSE_TA - 1);
  if (la >= na) return;
  const int an = a0 + la;
  int l = 0;
  while (l + 1 < a.levels && an >= a.a_off[l + 1]) ++l;
  const int pix = an - a.a_off[l], py = pix / a.lw[l], px = pix - py * a.lw[l];
  const float ax = (float)px + 0.5f, ay = (float)py + 0.5f, st = a.stride[l];          // make_anchors(offset 0.5)
  float* dst = a.out + ((long)b * (a.rows + a.nk) + a.rows) * a.A + an;
  float* rw = a.raw + (long)b * a.nk * a.A + an;
  for (int k = tid / POSE_TA; k < a.nk; k += 256 / POSE_TA) {
    const float v = S[k * POSE_SROW + la];
    const int d = k % a.ndim;
    float o;
    if (d == 0) o = (v * 2.0f + (ax - 0.5f)) * st;
    else if (d == 1) o = (v * 2.0f + (ay - 0.5f)) * st;
    else o = 1.0f / (1.0f + expf(-v));
    dst[(long)k * a.A] = o;
    rw[(long)k * a.A] = v;
  }
}

extern "C" int mgdt_pose_concat_fwd(const float* y, int n, int rows, int a_total, const mgdt_view* const* kpt, const float* strides, int n_levels, int nk,
                                    int ndim, float* out, float* kpt_raw, int dtype, mgdt_stream s) {
  if (!y || !out || !kpt_raw || !kpt || !strides) MGDT_FAIL(MGDT_BAD_ARG, "pose_concat: null pointer");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "pose_concat: dtype %d", dtype);
  if (n < 1 || rows < 5 || a_total < 1 || nk < 1 || nk > POSE_MAX_NK || (ndim != 2 && ndim != 3) || nk % ndim || n_levels < 1 || n_levels > POSE_MAX_LEVELS || n > 65535)
    MGDT_FAIL(MGDT_BAD_SHAPE, "pose_concat: n=%d rows=%d a=%d nk=%d (<= %d, a multiple of ndim=%d in {2, 3}) levels=%d (<= %d)", n, rows, a_total, nk,
              POSE_MAX_NK, ndim, n_levels, POSE_MAX_LEVELS);
  PoseCatArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y; a.out = out; a.raw = kpt_raw; a.B = n; a.rows = rows; a.nk = nk; a.ndim = ndim; a.A = a_total; a.levels = n_levels; a.vec = 1;
  const size_t es = dtype_size(dtype);
  const int nk4 = (nk + 3) / 4 * 4;
  int off = 0;
  for (int l = 0; l < n_levels; ++l) {
    const mgdt_view* v = kpt[l];
    if (!view_ok(v) || v->n != n || v->c < nk || v->sc != 1 || v->sw < v->c)
      MGDT_FAIL(MGDT_BAD_SHAPE, "pose_concat: level %d must be an NHWC view of %d x h x w x (>= %d) channels", l, n, nk);
    if (!(strides[l] > 0.f)) MGDT_FAIL(MGDT_BAD_ARG, "pose_concat: stride of level %d", l);
    // 4-channel pieces: every pixel must hold nk rounded up to 4 readable elements (inside the view's channels or its pixel stride) and start 4-element aligned
    if (v->sn % 4 || v->sh % 4 || v->sw % 4 || ((uintptr_t)v->p % (4 * es)) || v->sw < nk4) a.vec = 0;
    a.kp[l] = v->p; a.sn[l] = v->sn; a.sh[l] = v->sh; a.sp[l] = v->sw; a.lw[l] = v->w; a.a_off[l] = off; a.stride[l] = strides[l];
    off += v->h * v->w;
  }
  a.a_off[n_levels] = off;
  if (off != a_total) MGDT_FAIL(MGDT_BAD_SHAPE, "pose_concat: the levels hold %d anchors, the prediction %d", off, a_total);
  const dim3 grid(cdiv(a_total, POSE_TA), n);
  const size_t lds = (size_t)nk * POSE_SROW * sizeof(float);
  MGDT_DISPATCH_DTYPE(dtype, (pose_concat_kernel<T><<<grid, 256, lds, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("pose_concat_fwd");
  return MGDT_OK;
}

// ================================================================================================ post-NMS scaling of boxes and keypoints
// meta[n][8] = {gain, kpt_pad_x, kpt_pad_y, h0, w0, box_pad_x, box_pad_y, normalize}: scale_coords keeps the fractional letter-box padding
// (ops.py:653-655), scale_boxes rounds it (ops.py:104-105); both pairs are computed on the host like the reference does.  `lead` = 6 (NMS rows:
// box, conf, cls in front of the keypoints) or 0 (bare coordinates: scale_coords / clip_coords on their own).
__global__ __launch_bounds__(256) void pose_scale_kernel(float* __restrict__ rows, const int32_t* __restrict__ counts, const float* __restrict__ meta,
                                                         int max_det, int lead, int nk, int ndim) {
  const int b = blockIdx.y, W = lead + nk;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int det = i / W, col = i - det * W;
  if (det >= min(counts[b], max_det)) return;
  const float* m = meta + (long)b * 8;
  const float gain = m[0], h0 = m[3], w0 = m[4];
  float* p = rows + ((long)b * max_det + det) * W + col;
  if (col >= lead) {
    const int d = (col - lead) % ndim;
    if (d < 2) {
      float v = (*p - (d == 0 ? m[1] : m[2])) / gain;
      v = fminf(fmaxf(v, 0.f), d == 0 ? w0 : h0);
      if (m[7] != 0.f) v = v / (d == 0 ? w0 : h0);                 // normalize=True (ops.py:663-665)
      *p = v;
    }
  } else if (col < 4) {
    const bool isx = !(col & 1);
    const float v = (*p - (isx ? m[5] : m[6])) / gain;
    *p = rintf(fminf(fmaxf(v, 0.f), isx ? w0 : h0));
  }
}

extern "C" int mgdt_pose_scale_fwd(float* rows, const int32_t* counts, const float* meta, int n, int max_det, int lead, int nk, int ndim, mgdt_stream s) {
  if (!rows || !counts || !meta) MGDT_FAIL(MGDT_BAD_ARG, "pose_scale: null pointer");
  if (n < 1 || n > 65535 || max_det < 1 || (lead != 0 && lead != 6) || nk < 0 || lead + nk < 1 || (ndim != 2 && ndim != 3) || nk % ndim ||
      (long)max_det * (lead + nk) > 0x7fffffffL)
    MGDT_FAIL(MGDT_BAD_SHAPE, "pose_scale: n=%d max_det=%d lead=%d (0 or 6) nk=%d ndim=%d", n, max_det, lead, nk, ndim);
  const dim3 grid(cdiv((long)max_det * (lead + nk), 256), n);
  pose_scale_kernel<<<grid, 256, 0, (hipStream_t)s>>>(rows, counts, meta, max_det, lead, nk, ndim);
  MGDT_CHECK_LAUNCH("pose_scale_fwd");
  return MGDT_OK;
}
