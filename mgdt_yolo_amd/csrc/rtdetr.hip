// RT-DETR decoder head (reference nn/modules/head.py:275-464 RTDETRDecoder, nn/modules/transformer.py:187-378, vit/rtdetr/predict.py).
// The dense linears run on the implicit-GEMM convolution (a token matrix (B, L, C) is an NHWC map of height 1); this file holds the rest.
//
//   msdeform_attn   multi-scale deformable attention sampling, 4-coordinate reference boxes.  One wave per (image, query): lane = head * 8 + piece,
//                   a lane owns 4 of its head's 32 channels, so the 8 lanes of a head read one corner's 32 channels as one 16-byte (fp32) or
//                   8-byte (bf16) load each = 128 / 64 contiguous bytes.  Softmax over the head's nl*4 weight logits and all accumulation in fp32.
//                   Sampling = grid_sample(align_corners=False, zero padding): pixel = loc * (W, H) - 0.5, the four neighbours, those outside skipped.
//   mha             self-attention over the queries, hd 256 = 8 heads x 32, no mask.  One wave per (image, head, 16 queries), keys streamed in tiles
//                   of 16 with a running maximum and sum (fp32): S^T = K Q^T and O^T += V^T P^T on the 16x16x4 fp32 matrix-core form.  The
//                   accumulator of S^T holds keys 4g..4g+3 of query lane & 15, so the row maximum / sum are 3 in-lane steps and 2 lane exchanges, and
//                   the same registers are the B operand of the PV product (its k index walks keys 4g + e: a permutation of the sum).
//   add_ln          out = LayerNorm(x [+ res]) over 256 channels (x fp32 or bf16, the rest fp32), eps 1e-5, one wave per row, two passes in registers.  Masked form: rows whose anchor
//                   is invalid (head.py:382) take `fill` (= enc_output[0].bias: the linear of a zeroed token) in place of x.
//   rowmax          per-token maximum of the class logits (B*L, nc) -> (B*L).
//   topk            (B, L) scores -> (B, k) int64 token indices, descending score, equal scores by ascending index: each element counts the
//                   elements that precede it in that total order (exact for any L; NaN ranks as -inf).
//   gather          selected tokens: feature rows -> embed, class logit rows -> enc_scores.  An index outside [0, L) is clamped.
//   ref_init        reference boxes sigmoid(delta + anchor(token)), anchor = log(a / (1 - a)) in fp32 or +inf (head.py:368-385, including its
//                   division of (x + 0.5, y + 0.5) by (h, w)).
//   refine          ref = sigmoid(delta + inverse_sigmoid(ref)) (transformer.py:362, utils.py:36-40).
//   sigmoid         element-wise, the final scores.
//   post            the predictor's postprocess for a batch: xywh -> xyxy, class maximum / argmax (lowest index on ties), conf threshold, class filter,
//                   scaling by each image's (w, h); kept rows compacted in query order into (B, nq, 6) (the rest zero) + counts.
#include "common.h"

#define RT_HD 256
#define RT_NH 8
#define RT_DH 32
#define RT_NP 4
#define RT_MAXL 4

struct RtLevels { int nl, L; int h[RT_MAXL], w[RT_MAXL], start[RT_MAXL]; };

static int rt_levels(const int* shapes, int nl, RtLevels* lv, const char* who) {
  if (!shapes || nl < 1 || nl > RT_MAXL) MGDT_FAIL(MGDT_BAD_SHAPE, "%s: nl = %d levels (1..%d)", who, nl, RT_MAXL);
  long off = 0;
  for (int l = 0; l < RT_MAXL; ++l) { lv->h[l] = 1; lv->w[l] = 1; lv->start[l] = 0; }
  for (int l = 0; l < nl; ++l) {
    const int h = shapes[2 * l], w = shapes[2 * l + 1];
    if (h < 1 || w < 1 || h > 16384 || w > 16384) MGDT_FAIL(MGDT_BAD_SHAPE, "%s: level %d is %d x %d", who, l, h, w);
    lv->h[l] = h; lv->w[l] = w; lv->start[l] = (int)off;
    off += (long)h * w;
    if (off > (1L << 24)) MGDT_FAIL(MGDT_BAD_SHAPE, "%s: more than 2^24 tokens", who);
  }
  lv->nl = nl; lv->L = (int)off;
  return MGDT_OK;
}

__device__ __forceinline__ float rt_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// anchor of token `tok` (head.py:368-385): a[4] = log(a / (1 - a)); returns the valid flag (every coordinate inside (0.01, 0.99))
__device__ __forceinline__ bool rt_anchor(const RtLevels& lv, int tok, float a[4]) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < RT_MAXL; ++i)
    if (i < lv.nl && tok >= lv.start[i]) l = i;
  int h = lv.h[0], w = lv.w[0], st = lv.start[0];
#pragma unroll
  for (int i = 1; i < RT_MAXL; ++i)
    if (i == l) { h = lv.h[i]; w = lv.w[i]; st = lv.start[i]; }
  const int r = tok - st, y = r / w, x = r - y * w;
  const float wh = 0.05f * (float)(1 << l);
  const float v[4] = {((float)x + 0.5f) / (float)h, ((float)y + 0.5f) / (float)w, wh, wh};     // (x, y) over (h, w), as the reference divides
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ok = ok && (v[i] > 0.01f) && (v[i] < 0.99f);
    a[i] = logf(v[i] / (1.0f - v[i]));
  }
  return ok;
}

// ================================================================================================ deformable attention
struct RtDeformArgs {
  const void* value; const float* ref; const float* off; const float* wl; float* out;
  long ldv, sbv, ldo, ldw;
  int nq;
  RtLevels lv;
};

template <typename T>
__global__ __launch_bounds__(256) void rt_msdeform_kernel(const RtDeformArgs a) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (q >= a.nq) return;
  const int hd = lane >> 3, c0 = hd * RT_DH + 4 * (lane & 7);
  const int nl = a.lv.nl, np = nl * RT_NP;
  const long row = (long)b * a.nq + q;
  const float* wl = a.wl + row * a.ldw + hd * np;
  const float* of = a.off + row * a.ldo + hd * np * 2;
  const float* rf = a.ref + row * 4;
  const float rx = rf[0], ry = rf[1], sx = rf[2] * 0.5f, sy = rf[3] * 0.5f;
  float m = -INFINITY;
  for (int i = 0; i < np; ++i) m = fmaxf(m, wl[i]);
  float den = 0.f;
  for (int i = 0; i < np; ++i) den += expf(wl[i] - m);
  const T* V = (const T*)a.value + (long)b * a.sbv + c0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < RT_MAXL; ++l) {
    if (l >= nl) break;
    const int H = a.lv.h[l], W = a.lv.w[l];
    const T* Vl = V + (long)a.lv.start[l] * a.ldv;
#pragma unroll
    for (int p = 0; p < RT_NP; ++p) {
      const int i = l * RT_NP + p;
      const float pw = expf(wl[i] - m) / den;
      const float lx = rx + of[2 * i] / (float)RT_NP * sx, ly = ry + of[2 * i + 1] / (float)RT_NP * sy;
      // clamped so that the integer conversion is defined; every pixel coordinate outside [-1, size] has no neighbour inside the map either way
      const float ix = fmaxf(fminf(lx * (float)W - 0.5f, (float)W + 1.f), -2.f), iy = fmaxf(fminf(ly * (float)H - 0.5f, (float)H + 1.f), -2.f);
      const float fx = floorf(ix), fy = floorf(iy);
      const int x0 = (int)fx, y0 = (int)fy;
      const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
#pragma unroll
      for (int cy = 0; cy < 2; ++cy) {
#pragma unroll
        for (int cx = 0; cx < 2; ++cx) {
          const int x = x0 + cx, y = y0 + cy;
          if (x < 0 || x >= W || y < 0 || y >= H) continue;
          const float cw = pw * (cx ? wx1 : wx0) * (cy ? wy1 : wy0);
          const f32x4 v = load4<T>(Vl + ((long)y * W + x) * a.ldv);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(cw, v[e], acc[e]);
        }
      }
    }
  }
  *(f32x4*)(a.out + row * RT_HD + c0) = acc;
}

extern "C" int mgdt_msdeform_attn_fwd(const void* value, long ld_value, long batch_stride_value, const int* shapes, int nl, int batch, int nq, const float* ref,
                                      const float* offsets, long ld_offsets, const float* weights, long ld_weights, float* out, int dtype, mgdt_stream s) {
  if (!value || !ref || !offsets || !weights || !out) MGDT_FAIL(MGDT_BAD_ARG, "msdeform_attn: null pointer");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "msdeform_attn: dtype %d", dtype);
  RtDeformArgs a;
  const int st = rt_levels(shapes, nl, &a.lv, "msdeform_attn");
  if (st != MGDT_OK) return st;
  if (batch < 1 || batch > 65535 || nq < 1) MGDT_FAIL(MGDT_BAD_SHAPE, "msdeform_attn: batch = %d (1..65535), nq = %d", batch, nq);
  const int pe = 4;                                                            // a lane's 4 values: one 16-byte (fp32) or 8-byte (bf16) load
  if (ld_value < RT_HD || ld_value % pe || batch_stride_value % pe || batch_stride_value < (long)a.lv.L * ld_value || ((uintptr_t)value % (pe * dtype_size(dtype))))
    MGDT_FAIL(MGDT_BAD_SHAPE, "msdeform_attn: value rows of %d channels, row stride %ld, image stride %ld (>= %d rows), aligned to a lane's 4 values", RT_HD, ld_value,
              batch_stride_value, a.lv.L);
  if (ld_offsets < RT_NH * nl * RT_NP * 2 || ld_weights < RT_NH * nl * RT_NP || ((uintptr_t)out % 16))
    MGDT_FAIL(MGDT_BAD_SHAPE, "msdeform_attn: offset rows hold %d values, weight rows %d; out 16-byte aligned", RT_NH * nl * RT_NP * 2, RT_NH * nl * RT_NP);
  a.value = value; a.ref = ref; a.off = offsets; a.wl = weights; a.out = out;
  a.ldv = ld_value; a.sbv = batch_stride_value; a.ldo = ld_offsets; a.ldw = ld_weights; a.nq = nq;
  const dim3 grid(cdiv(nq, 4), batch);
  MGDT_DISPATCH_DTYPE(dtype, (rt_msdeform_kernel<T><<<grid, 256, 0, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("msdeform_attn_fwd");
  return MGDT_OK;
}

// ================================================================================================ self-attention
struct RtMhaArgs { const float* q; const float* k; const float* v; float* out; long ldq, ldk, ldv; int nq; float scale; };

__global__ __launch_bounds__(64) void rt_mha_kernel(const RtMhaArgs a) {
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, hd = blockIdx.y, b = blockIdx.z;
  const int nq = a.nq;
  const long base = (long)b * nq;
  // B operand of S^T = K Q^T: query j, head channels 8g .. 8g + 7 (the k index of step t is channel 8g + t in both operands)
  const int qr = min(q0 + j, nq - 1);
  const float* qp = a.q + (base + qr) * a.ldq + hd * RT_DH + 8 * g;
  f32x4 qa = *(const f32x4*)qp, qb = *(const f32x4*)(qp + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { qa[e] *= a.scale; qb[e] *= a.scale; }
  float m = -INFINITY, den = 0.f;
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;                                   // O^T: channels 4g + e (o0) and 16 + 4g + e (o1) of query j
  for (int k0 = 0; k0 < nq; k0 += 16) {
    const int kr = min(k0 + j, nq - 1);                                         // A operand: key j of the tile (clamped; masked below)
    const float* kp = a.k + (base + kr) * a.ldk + hd * RT_DH + 8 * g;
    const f32x4 ka = *(const f32x4*)kp, kb = *(const f32x4*)(kp + 4);
    f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], qa[e], sc, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[e], qb[e], sc, 0, 0, 0);
    // sc[e] = S[query j][key k0 + 4g + e]
    float tm = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (k0 + 4 * g + e >= nq) sc[e] = -INFINITY;
      tm = fmaxf(tm, sc[e]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 16));
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(m, tm);                                              // finite: key k0 of every tile exists
    const float alpha = expf(m - mn);
    float ts = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sc[e] = expf(sc[e] - mn); ts += sc[e]; }
    ts += __shfl_xor(ts, 16);
    ts += __shfl_xor(ts, 32);
    den = den * alpha + ts;
    m = mn;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
    // O^T += V^T P^T: step e multiplies keys k0 + 4g + e (B operand = sc[e]); A operand = V[that key][channel j] and [16 + j]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int vr = min(k0 + 4 * g + e, nq - 1);                               // a key past nq has weight 0
      const float* vp = a.v + (base + vr) * a.ldv + hd * RT_DH + j;
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[0], sc[e], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16], sc[e], o1, 0, 0, 0);
    }
  }
  if (q0 + j < nq) {
    const float inv = 1.0f / den;
    float* op = a.out + (base + q0 + j) * RT_HD + hd * RT_DH + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o0[e] *= inv; o1[e] *= inv; }
    *(f32x4*)op = o0;
    *(f32x4*)(op + 16) = o1;
  }
}

extern "C" int mgdt_mha_fwd(const float* q, long ld_q, const float* k, long ld_k, const float* v, long ld_v, int batch, int nq, float* out, mgdt_stream s) {
  if (!q || !k || !v || !out) MGDT_FAIL(MGDT_BAD_ARG, "mha: null pointer");
  if (batch < 1 || batch > 65535 || nq < 1 || nq > (1 << 20)) MGDT_FAIL(MGDT_BAD_SHAPE, "mha: batch = %d (1..65535), nq = %d", batch, nq);
  if (ld_q < RT_HD || ld_k < RT_HD || ld_v < RT_HD || ld_q % 4 || ld_k % 4 || ((uintptr_t)q % 16) || ((uintptr_t)k % 16) || ((uintptr_t)out % 16))
    MGDT_FAIL(MGDT_BAD_SHAPE, "mha: rows of %d channels (8 heads x 32), q / k row strides multiples of 4 (%ld, %ld, %ld), 16-byte aligned", RT_HD, ld_q, ld_k, ld_v);
  RtMhaArgs a{q, k, v, out, ld_q, ld_k, ld_v, nq, 0.17677669529663687f};        // sqrt(1 / 32), applied to q (F.multi_head_attention_forward)
  const dim3 grid(cdiv(nq, 16), RT_NH, batch);
  rt_mha_kernel<<<grid, 64, 0, (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("mha_fwd");
  return MGDT_OK;
}

// ================================================================================================ add + LayerNorm
struct RtLnArgs { const void* x; const float* res; const float* gamma; const float* beta; const float* fill; float* out; long ldx, ldr, rows; int masked; float eps; RtLevels lv; };

template <typename T>
__global__ __launch_bounds__(256) void rt_add_ln_kernel(const RtLnArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  const int c = 4 * lane;
  f32x4 v = load4<T>((const T*)a.x + row * a.ldx + c);
  if (a.masked) {
    float an[4];
    if (!rt_anchor(a.lv, (int)(row % a.lv.L), an)) {
      v = *(const f32x4*)(a.fill + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)(T)v[e];                       // as the linear's T output would hold it
    }
  }
  if (a.res) {
    const f32x4 r = *(const f32x4*)(a.res + row * a.ldr + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += r[e];
  }
  float sum = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  const float mean = sum * (1.0f / RT_HD);
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] -= mean; sq = fmaf(v[e], v[e], sq); }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o);
  const float rstd = 1.0f / sqrtf(sq * (1.0f / RT_HD) + a.eps);
  const f32x4 gm = *(const f32x4*)(a.gamma + c), bt = *(const f32x4*)(a.beta + c);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = v[e] * rstd * gm[e] + bt[e];
  *(f32x4*)(a.out + row * RT_HD + c) = o;
}

extern "C" int mgdt_add_layernorm_fwd(const void* x, int dtype, long ld_x, const float* res, long ld_res, const float* gamma, const float* beta, float eps, long rows,
                                      const float* fill, const int* shapes, int nl, float* out, mgdt_stream s) {
  if (!x || !gamma || !beta || !out) MGDT_FAIL(MGDT_BAD_ARG, "add_layernorm: null pointer");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "add_layernorm: dtype %d", dtype);
  if (rows < 1 || rows > (1L << 31) - 8) MGDT_FAIL(MGDT_BAD_SHAPE, "add_layernorm: rows = %ld", rows);
  if (ld_x < RT_HD || ld_x % 4 || (res && (ld_res < RT_HD || ld_res % 4)) || ((uintptr_t)x % (4 * dtype_size(dtype))) || ((uintptr_t)res % 16) || ((uintptr_t)gamma % 16) || ((uintptr_t)beta % 16) ||
      ((uintptr_t)out % 16) || ((uintptr_t)fill % 16))
    MGDT_FAIL(MGDT_BAD_SHAPE, "add_layernorm: rows of %d channels, row strides multiples of 4, 16-byte aligned pointers", RT_HD);
  RtLnArgs a;
  a.x = x; a.res = res; a.gamma = gamma; a.beta = beta; a.fill = fill; a.out = out; a.ldx = ld_x; a.ldr = ld_res; a.rows = rows; a.eps = eps;
  a.masked = fill != nullptr;
  if (a.masked) {
    const int st = rt_levels(shapes, nl, &a.lv, "add_layernorm");
    if (st != MGDT_OK) return st;
    if (rows % a.lv.L) MGDT_FAIL(MGDT_BAD_SHAPE, "add_layernorm: %ld rows are not whole images of %d tokens", rows, a.lv.L);
  } else {
    memset(&a.lv, 0, sizeof(a.lv));
  }
  MGDT_DISPATCH_DTYPE(dtype, (rt_add_ln_kernel<T><<<cdiv(rows, 4), 256, 0, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("add_layernorm_fwd");
  return MGDT_OK;
}

// ================================================================================================ query selection
__global__ __launch_bounds__(256) void rt_rowmax_kernel(const float* __restrict__ x, long rows, int nc, long ld, float* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  float m = -INFINITY;
  if (row < rows)
    for (int c = sub; c < nc; c += 16) m = fmaxf(m, x[row * ld + c]);
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (row < rows && sub == 0) out[row] = m;
}

extern "C" int mgdt_rtdetr_rowmax_fwd(const float* x, long rows, int nc, long ld, float* out, mgdt_stream s) {
  if (!x || !out) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_rowmax: null pointer");
  if (rows < 1 || rows > (1L << 34) || nc < 1 || ld < nc) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_rowmax: rows = %ld, nc = %d, row stride %ld", rows, nc, ld);
  rt_rowmax_kernel<<<cdiv(rows, 16), 256, 0, (hipStream_t)s>>>(x, rows, nc, ld, out);
  MGDT_CHECK_LAUNCH("rtdetr_rowmax_fwd");
  return MGDT_OK;
}

__global__ __launch_bounds__(256) void rt_topk_kernel(const float* __restrict__ scores, int L, int k, int64_t* __restrict__ index) {
  __shared__ float tile[256];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const float* sr = scores + (long)b * L;
  float mine = -INFINITY;
  if (i < L) { mine = sr[i]; if (mine != mine) mine = -INFINITY; }
  int rank = 0;
  for (int t0 = 0; t0 < L; t0 += 256) {
    const int jl = t0 + threadIdx.x;
    float v = -INFINITY;
    if (jl < L) { v = sr[jl]; if (v != v) v = -INFINITY; }
    __syncthreads();
    tile[threadIdx.x] = v;
    __syncthreads();
    const int n = min(256, L - t0);
    for (int u = 0; u < n; ++u) {
      const float o = tile[u];
      rank += (o > mine || (o == mine && t0 + u < i)) ? 1 : 0;
    }
  }
  if (i < L && rank < k) index[(long)b * k + rank] = i;
}

extern "C" int mgdt_rtdetr_topk_fwd(const float* scores, int batch, int L, int k, int64_t* index, mgdt_stream s) {
  if (!scores || !index) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_topk: null pointer");
  if (batch < 1 || batch > 65535 || k < 1 || L < k || L > (1 << 24)) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_topk: batch = %d (1..65535), L = %d, k = %d (1 <= k <= L <= 2^24)", batch, L, k);
  const dim3 grid(cdiv(L, 256), batch);
  rt_topk_kernel<<<grid, 256, 0, (hipStream_t)s>>>(scores, L, k, index);
  MGDT_CHECK_LAUNCH("rtdetr_topk_fwd");
  return MGDT_OK;
}

// ================================================================================================ gather, reference boxes
__global__ __launch_bounds__(256) void rt_gather_kernel(const float* __restrict__ feat, const float* __restrict__ scores, const int64_t* __restrict__ index, int L, int nq,
                                                        int nc, long lds_, float* __restrict__ embed, float* __restrict__ enc_scores) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (q >= nq) return;
  const long row = (long)b * nq + q;
  long tok = index[row];
  tok = tok < 0 ? 0 : (tok >= L ? L - 1 : tok);
  const long src = (long)b * L + tok;
  *(f32x4*)(embed + row * RT_HD + 4 * lane) = *(const f32x4*)(feat + src * RT_HD + 4 * lane);
  for (int c = lane; c < nc; c += 64) enc_scores[row * nc + c] = scores[src * lds_ + c];
}

extern "C" int mgdt_rtdetr_gather_fwd(const float* feat, const float* scores, long ld_scores, const int64_t* index, int batch, int L, int nq, int nc, float* embed,
                                      float* enc_scores, mgdt_stream s) {
  if (!feat || !scores || !index || !embed || !enc_scores) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_gather: null pointer");
  if (batch < 1 || batch > 65535 || L < 1 || nq < 1 || nc < 1 || ld_scores < nc) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_gather: batch = %d, L = %d, nq = %d, nc = %d", batch, L, nq, nc);
  if (((uintptr_t)feat % 16) || ((uintptr_t)embed % 16)) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_gather: 16-byte aligned feature rows");
  const dim3 grid(cdiv(nq, 4), batch);
  rt_gather_kernel<<<grid, 256, 0, (hipStream_t)s>>>(feat, scores, index, L, nq, nc, ld_scores, embed, enc_scores);
  MGDT_CHECK_LAUNCH("rtdetr_gather_fwd");
  return MGDT_OK;
}

__global__ __launch_bounds__(256) void rt_ref_init_kernel(const float* __restrict__ delta, long ldd, const int64_t* __restrict__ index, long n, int nq, const RtLevels lv,
                                                          float* __restrict__ ref) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  long tok = index[row];
  tok = tok < 0 ? 0 : (tok >= lv.L ? lv.L - 1 : tok);
  float an[4];
  const bool ok = rt_anchor(lv, (int)tok, an);
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = ok ? rt_sigmoid(delta[row * ldd + e] + an[e]) : 1.0f;      // sigmoid(finite + inf) = 1
  *(f32x4*)(ref + row * 4) = o;
}

extern "C" int mgdt_rtdetr_ref_init_fwd(const float* delta, long ld_delta, const int64_t* index, int batch, int nq, const int* shapes, int nl, float* ref, mgdt_stream s) {
  if (!delta || !index || !ref) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_ref_init: null pointer");
  RtLevels lv;
  const int st = rt_levels(shapes, nl, &lv, "rtdetr_ref_init");
  if (st != MGDT_OK) return st;
  if (batch < 1 || nq < 1 || ld_delta < 4 || ((uintptr_t)ref % 16)) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_ref_init: batch = %d, nq = %d, row stride %ld", batch, nq, ld_delta);
  const long n = (long)batch * nq;
  rt_ref_init_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)s>>>(delta, ld_delta, index, n, nq, lv, ref);
  MGDT_CHECK_LAUNCH("rtdetr_ref_init_fwd");
  return MGDT_OK;
}

__global__ __launch_bounds__(256) void rt_refine_kernel(const float* __restrict__ delta, long ldd, const float* __restrict__ ref, long n, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i >> 2;
  const int e = (int)(i & 3);
  const float x = fminf(fmaxf(ref[i], 0.f), 1.f);                              // utils.py:36-40, eps 1e-5
  const float inv = logf(fmaxf(x, 1e-5f) / fmaxf(1.0f - x, 1e-5f));
  out[i] = rt_sigmoid(delta[row * ldd + e] + inv);
}

extern "C" int mgdt_rtdetr_refine_fwd(const float* delta, long ld_delta, const float* ref, long rows, float* out, mgdt_stream s) {
  if (!delta || !ref || !out) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_refine: null pointer");
  if (rows < 1 || rows > (1L << 31) || ld_delta < 4) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_refine: rows = %ld, row stride %ld", rows, ld_delta);
  rt_refine_kernel<<<cdiv(rows * 4, 256), 256, 0, (hipStream_t)s>>>(delta, ld_delta, ref, rows * 4, out);
  MGDT_CHECK_LAUNCH("rtdetr_refine_fwd");
  return MGDT_OK;
}

__global__ __launch_bounds__(256) void rt_sigmoid_kernel(const float* __restrict__ x, long rows, int nc, long ld, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * nc) return;
  const long row = i / nc;
  out[i] = rt_sigmoid(x[row * ld + (i - row * nc)]);
}

extern "C" int mgdt_rtdetr_sigmoid_fwd(const float* x, long rows, int nc, long ld, float* out, mgdt_stream s) {
  if (!x || !out) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_sigmoid: null pointer");
  if (rows < 1 || nc < 1 || ld < nc || rows * nc > (1L << 40)) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_sigmoid: rows = %ld, nc = %d, row stride %ld", rows, nc, ld);
  rt_sigmoid_kernel<<<cdiv(rows * nc, 256), 256, 0, (hipStream_t)s>>>(x, rows, nc, ld, out);
  MGDT_CHECK_LAUNCH("rtdetr_sigmoid_fwd");
  return MGDT_OK;
}

// ================================================================================================ postprocess
__global__ __launch_bounds__(256) void rt_post_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, int nq, int nc, float conf,
                                                      const uint8_t* __restrict__ keep_class, const float* __restrict__ wh, float* __restrict__ rows,
                                                      int32_t* __restrict__ counts) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float sw = wh ? wh[2 * b] : 1.f, sh = wh ? wh[2 * b + 1] : 1.f;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int q0 = 0; q0 < nq; q0 += 256) {
    const int q = q0 + tid;
    bool keep = false;
    float best = -INFINITY;
    int cls = 0;
    if (q < nq) {
      const float* sr = scores + ((long)b * nq + q) * nc;
      for (int c = 0; c < nc; ++c) {
        const float v = sr[c];
        if (v > best) { best = v; cls = c; }
      }
      keep = best > conf && (!keep_class || keep_class[cls]);
    }
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    int off = carry;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (keep) {
      const float* bx = boxes + ((long)b * nq + q) * 4;
      const float dw = bx[2] / 2.f, dh = bx[3] / 2.f;                          // ops.xywh2xyxy
      float* o = rows + ((long)b * nq + off + before) * 6;
      o[0] = (bx[0] - dw) * sw; o[1] = (bx[1] - dh) * sh; o[2] = (bx[0] + dw) * sw; o[3] = (bx[1] + dh) * sh;
      o[4] = best; o[5] = (float)cls;
    }
    __syncthreads();
    if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  const int total = carry;
  for (int i = total * 6 + tid; i < nq * 6; i += 256) rows[(long)b * nq * 6 + i] = 0.f;
  if (tid == 0) counts[b] = total;
}

extern "C" int mgdt_rtdetr_post_fwd(const float* boxes, const float* scores, int batch, int nq, int nc, float conf, const uint8_t* keep_class, const float* wh, float* rows,
                                    int32_t* counts, mgdt_stream s) {
  if (!boxes || !scores || !rows || !counts) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_post: null pointer");
  if (batch < 1 || nq < 1 || nc < 1 || nq > (1 << 24)) MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_post: batch = %d, nq = %d, nc = %d", batch, nq, nc);
  rt_post_kernel<<<batch, 256, 0, (hipStream_t)s>>>(boxes, scores, nq, nc, conf, keep_class, wh, rows, counts);
  MGDT_CHECK_LAUNCH("rtdetr_post_fwd");
  return MGDT_OK;
}
