// Image classification (reference nn/modules/head.py:256-272 Classify, yolo/utils/loss.py:395-401 v8ClassificationLoss,
// yolo/v8/classify/val.py + yolo/utils/metrics.py:197-207, :934-977 top-k accuracy and the confusion matrix).
//
//   classify_pool    Classify.conv (1x1 conv c1 -> cout, BatchNorm folded, SiLU) + AdaptiveAvgPool2d(1) in one launch: pooled (B, cout) fp32.  The
//                    (B, cout, h, w) map never reaches HBM.  Per image a GEMM M = h*w pixels, K = c1, N = cout on the matrix cores (16x16x32 bf16 /
//                    16x16x4 f32).  A workgroup owns (image, NB = 16 / 32 / 64 output channels): it stages its NB x K weight slice in LDS once; its
//                    four waves split into NB / 16 channel tiles x 4 / (NB / 16) pixel phases; a wave walks its 16-pixel tiles (pixels = A operand,
//                    read from global memory in 16-byte pieces; weights = B operand from LDS), so the accumulator holds channel lane & 15 at pixels
//                    4 * (lane >> 4) + 0..3.  Epilogue in registers: + shift, SiLU, rows past h*w masked (SiLU(shift) != 0: an unmasked padding row
//                    would bias the mean), summed per lane; then two lane exchanges, an LDS slot per wave, and a fixed-order sum over the pixel
//                    phases.  No floating-point atomics: the summation order depends on the shape alone (bit-reproducible).
//   classify_linear  logits = pooled @ W^T + b (one wave per output, fp32 accumulation, W in the compute dtype) [+ the row softmax, second launch].
//   cls_softmax      row softmax of fp32 logits (maximum subtracted).
//   cls_loss         cross_entropy(logits, cls, reduction='sum') / 64 and its gradient (softmax - onehot) / 64 * gscale.  A label outside [0, nc):
//                    NaN loss, zero gradient row, nothing read out of bounds.
//   cls_topk         indices of the min(nc, 5) largest values per row, descending, equal values by lower index first [+ confusion counts
//                    matrix[top1][target] += 1, int32, integer atomics].
#include "common.h"

#define CLS_DIV 64.0f              // loss.py:399: the constant 64, not the batch size
#define CLS_TOPK 5

typedef __attribute__((ext_vector_type(4))) unsigned int cls_u32x4;

struct ClsPoolArgs {
  const void* x; const void* w; const float* bias; float* pooled;
  long sn, sh, sw;
  int W, HW, K, cout, NB, ldw;
};

template <typename T>
__global__ __launch_bounds__(256) void classify_pool_kernel(const ClsPoolArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cls_smem[];
  T* Ws = (T*)cls_smem;                                                        // [NB][ldw]: the weight slice, rows padded by 16 bytes
  float* part = (float*)(cls_smem + (size_t)a.NB * a.ldw * sizeof(T));         // [4 waves][16 channels]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, n0 = blockIdx.x * a.NB;
  constexpr int PV = 16 / (int)sizeof(T);                                      // elements of a 16-byte piece
  const int pieces = a.K / PV;
  for (int i = tid; i < a.NB * pieces; i += 256) {
    const int r = i / pieces, q = i - r * pieces;
    *(cls_u32x4*)(Ws + (long)r * a.ldw + q * PV) = *(const cls_u32x4*)((const T*)a.w + (long)(n0 + r) * a.K + q * PV);
  }
  __syncthreads();
  const int NT = a.NB >> 4, MS = 4 / NT;                                       // channel tiles (1, 2, 4) x pixel phases (4, 2, 1)
  const int nt = wave % NT, ms = wave / NT;
  const int j = lane & 15, g = lane >> 4;
  const T* wrow = Ws + (long)(nt * 16 + j) * a.ldw;                            // B operand: channel j of the tile, k = 8g .. 8g + 7
  const float shift = a.bias[n0 + nt * 16 + j];
  const T* X = (const T*)a.x + (long)b * a.sn;
  const int tiles = (a.HW + 15) >> 4;
  float sum = 0.f;
  for (int t = ms; t < tiles; t += MS) {
    const int p0 = t * 16, p = min(p0 + j, a.HW - 1);                          // A operand: pixel p0 + j (clamped: rows past h*w are masked below)
    const int py = p / a.W, px = p - py * a.W;
    const T* src = X + (long)py * a.sh + (long)px * a.sw;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int k0 = 0; k0 < a.K; k0 += 32) {
      const int k = k0 + 8 * g;
      const bool in = k < a.K;                                                 // K % 8 == 0: a lane's 8 values are all inside or all outside
      if constexpr (sizeof(T) == 2) {
        bf16x8 av, bv;
#pragma unroll
        for (int e = 0; e < 8; ++e) { av[e] = (bf16)0.f; bv[e] = (bf16)0.f; }
        if (in) { av = *(const bf16x8*)(src + k); bv = *(const bf16x8*)(wrow + k); }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
      } else {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, b0 = a0, b1 = a0;
        if (in) {
          a0 = *(const f32x4*)(src + k); a1 = *(const f32x4*)(src + k + 4);
          b0 = *(const f32x4*)(wrow + k); b1 = *(const f32x4*)(wrow + k + 4);
        }
        // step e multiplies k = 8g + e of both operands (the 16x16x4 form takes k = lane >> 4): the eight steps cover the 32 values
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b0[e], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b1[e], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = acc[e] + shift;
      const float sv = v * fast_sigmoid(v);
      if (p0 + 4 * g + e < a.HW) sum += sv;                                    // the mask of the last tile's padding rows
    }
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  if (lane < 16) part[wave * 16 + lane] = sum;
  __syncthreads();
  if (tid < a.NB) {
    const int t = tid >> 4, c = tid & 15;
    float s = 0.f;
    for (int m = 0; m < MS; ++m) s += part[(m * NT + t) * 16 + c];
    a.pooled[(long)b * a.cout + n0 + tid] = s / (float)a.HW;
  }
}

extern "C" int mgdt_classify_pool_fwd(const mgdt_view* x, const void* w, const float* bias, int cout, int k, int groups, int act, float* pooled, int dtype,
                                      mgdt_stream s) {
  if (!w || !bias || !pooled) MGDT_FAIL(MGDT_BAD_ARG, "classify_pool: null pointer");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "classify_pool: dtype %d", dtype);
  if (k != 1 || groups != 1) MGDT_FAIL(MGDT_BAD_ARG, "classify_pool: the fused head takes a 1x1 convolution with groups = 1 (k = %d, groups = %d): use the unfused chain", k, groups);
  if (act != MGDT_ACT_SILU) MGDT_FAIL(MGDT_BAD_ARG, "classify_pool: the fused head applies SiLU (act code %d): use the unfused chain", act);
  if (!view_ok(x) || !view_nhwc(x)) MGDT_FAIL(MGDT_BAD_SHAPE, "classify_pool: x must be a non-empty NHWC view");
  const int es = (int)dtype_size(dtype);
  if (x->c % 8 || cout < 16 || cout % 16 || x->n > 65535 || (long)x->h * x->w > (1L << 24))
    MGDT_FAIL(MGDT_BAD_SHAPE, "classify_pool: c1 = %d (a multiple of 8), cout = %d (a multiple of 16), n = %d (<= 65535), h*w = %ld (<= 2^24)", x->c, cout, x->n,
              (long)x->h * x->w);
  // the stride of a dimension of size 1 is never used (torch leaves it arbitrary)
  if ((x->n > 1 && x->sn % 8) || (x->h > 1 && x->sh % 8) || (x->w > 1 && x->sw % 8) || ((uintptr_t)x->p % 16) || ((uintptr_t)w % 16))
    MGDT_FAIL(MGDT_BAD_SHAPE, "classify_pool: pixel rows of x and the weights must be 16-byte aligned (strides %ld %ld %ld)", (long)x->sn, (long)x->sh, (long)x->sw);
  ClsPoolArgs a;
  a.x = x->p; a.w = w; a.bias = bias; a.pooled = pooled; a.sn = x->sn; a.sh = x->sh; a.sw = x->sw;
  a.W = x->w; a.HW = x->h * x->w; a.K = x->c; a.cout = cout;
  a.ldw = x->c + 16 / es;
  const size_t row = (size_t)a.ldw * es;
  a.NB = 16;
  for (int nb = 64; nb >= 32; nb >>= 1)
    if (cout % nb == 0 && nb * row <= 64 * 1024) { a.NB = nb; break; }
  const size_t lds = a.NB * row + 4 * 16 * sizeof(float);
  if (lds > 160 * 1024) MGDT_FAIL(MGDT_BAD_SHAPE, "classify_pool: c1 = %d needs %zu bytes of LDS for 16 output channels (<= 160 KiB)", x->c, lds);
  if (lds > 64 * 1024)
    if (int rc = lds_optin<classify_pool_kernel<float>, classify_pool_kernel<bf16>>("classify_pool")) return rc;
  const dim3 grid(cout / a.NB, x->n);
  MGDT_DISPATCH_DTYPE(dtype, (classify_pool_kernel<T><<<grid, 256, lds, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("classify_pool_fwd");
  return MGDT_OK;
}

// ================================================================================================ linear + softmax
// block-wide reductions in a fixed order (256 threads): lane exchanges inside a wave, then the four wave values through LDS
__device__ __forceinline__ float cls_block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float cls_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T>
__global__ __launch_bounds__(256) void classify_linear_kernel(const float* __restrict__ pooled, const T* __restrict__ w, const float* __restrict__ bias,
                                                              int K, int nc, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (n >= nc) return;
  const float* p = pooled + (long)b * K;
  const T* wr = w + (long)n * K;
  float acc = 0.f;
  for (int k = lane * 4; k < K; k += 256) {                                   // K % 4 == 0
    const f32x4 pv = *(const f32x4*)(p + k), wv = load4<T>(wr + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(pv[e], wv[e], acc);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) logits[(long)b * nc + n] = acc + (bias ? bias[n] : 0.f);
}

// one workgroup per row: maximum, sum of exp(v - max), normalise; `gmode` 0: the softmax; 1: (softmax - onehot(label)) * scale (zero row for a bad label)
__global__ __launch_bounds__(256) void cls_softmax_kernel(const float* __restrict__ logits, int nc, float* __restrict__ out, const int64_t* __restrict__ labels,
                                                          float scale, int gmode) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* r = logits + (long)b * nc;
  float* o = out + (long)b * nc;
  long lab = -1;
  if (gmode) {
    lab = labels[b];
    if (lab < 0 || lab >= nc) {
      for (int i = tid; i < nc; i += 256) o[i] = 0.f;
      return;                                                                  // uniform: the whole workgroup reads the same label
    }
  }
  float m = -INFINITY;
  for (int i = tid; i < nc; i += 256) m = fmaxf(m, r[i]);
  m = cls_block_max(m, red);
  float sum = 0.f;
  for (int i = tid; i < nc; i += 256) sum += expf(r[i] - m);
  sum = cls_block_sum(sum, red);
  for (int i = tid; i < nc; i += 256) {
    const float pr = expf(r[i] - m) / sum;
    o[i] = gmode ? (pr - (i == lab ? 1.f : 0.f)) * scale : pr;
  }
}

extern "C" int mgdt_cls_softmax_fwd(const float* logits, int n, int nc, float* probs, mgdt_stream s) {
  if (!logits || !probs) MGDT_FAIL(MGDT_BAD_ARG, "cls_softmax: null pointer");
  if (n < 1 || nc < 1) MGDT_FAIL(MGDT_BAD_SHAPE, "cls_softmax: n=%d nc=%d", n, nc);
  cls_softmax_kernel<<<n, 256, 0, (hipStream_t)s>>>(logits, nc, probs, nullptr, 1.f, 0);
  MGDT_CHECK_LAUNCH("cls_softmax_fwd");
  return MGDT_OK;
}

extern "C" int mgdt_classify_linear_fwd(const float* pooled, const void* w, const float* bias, int n, int k, int nc, float* logits, float* probs, int dtype,
                                        mgdt_stream s) {
  if (!pooled || !w || !logits) MGDT_FAIL(MGDT_BAD_ARG, "classify_linear: null pointer");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "classify_linear: dtype %d", dtype);
  if (n < 1 || n > 65535 || nc < 1 || k < 4 || k % 4) MGDT_FAIL(MGDT_BAD_SHAPE, "classify_linear: n=%d (<= 65535) nc=%d k=%d (a multiple of 4)", n, nc, k);
  if (((uintptr_t)pooled % 16) || ((uintptr_t)w % 16)) MGDT_FAIL(MGDT_BAD_SHAPE, "classify_linear: pooled and the weights must be 16-byte aligned");
  const dim3 grid(cdiv(nc, 4), n);
  MGDT_DISPATCH_DTYPE(dtype, (classify_linear_kernel<T><<<grid, 256, 0, (hipStream_t)s>>>(pooled, (const T*)w, bias, k, nc, logits)));
  MGDT_CHECK_LAUNCH("classify_linear_fwd");
  if (probs) {
    cls_softmax_kernel<<<n, 256, 0, (hipStream_t)s>>>(logits, nc, probs, nullptr, 1.f, 0);
    MGDT_CHECK_LAUNCH("classify_linear_fwd (softmax)");
  }
  return MGDT_OK;
}

// ================================================================================================ loss
__global__ __launch_bounds__(256) void cls_loss_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int nc, float* __restrict__ row_loss) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* r = logits + (long)b * nc;
  const long lab = labels[b];
  if (lab < 0 || lab >= nc) {                                                  // uniform
    if (tid == 0) row_loss[b] = __builtin_nanf("");
    return;
  }
  float m = -INFINITY;
  for (int i = tid; i < nc; i += 256) m = fmaxf(m, r[i]);
  m = cls_block_max(m, red);
  float sum = 0.f;
  for (int i = tid; i < nc; i += 256) sum += expf(r[i] - m);
  sum = cls_block_sum(sum, red);
  if (tid == 0) row_loss[b] = (logf(sum) + m) - r[lab];                        // -log_softmax(logits)[label]
}

__global__ __launch_bounds__(64) void cls_loss_sum_kernel(const float* __restrict__ row_loss, int n, float* __restrict__ loss) {
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) v += row_loss[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if (threadIdx.x == 0) *loss = v / CLS_DIV;
}

extern "C" int mgdt_cls_loss_fwd(const float* logits, const int64_t* labels, int n, int nc, float* row_loss, float* loss, mgdt_stream s) {
  if (!logits || !labels || !row_loss || !loss) MGDT_FAIL(MGDT_BAD_ARG, "cls_loss_fwd: null pointer");
  if (n < 1 || nc < 1) MGDT_FAIL(MGDT_BAD_SHAPE, "cls_loss_fwd: n=%d nc=%d", n, nc);
  cls_loss_row_kernel<<<n, 256, 0, (hipStream_t)s>>>(logits, labels, nc, row_loss);
  MGDT_CHECK_LAUNCH("cls_loss_fwd");
  cls_loss_sum_kernel<<<1, 64, 0, (hipStream_t)s>>>(row_loss, n, loss);
  MGDT_CHECK_LAUNCH("cls_loss_fwd (sum)");
  return MGDT_OK;
}

extern "C" int mgdt_cls_loss_bwd(const float* logits, const int64_t* labels, int n, int nc, float gscale, float* dlogits, mgdt_stream s) {
  if (!logits || !labels || !dlogits) MGDT_FAIL(MGDT_BAD_ARG, "cls_loss_bwd: null pointer");
  if (n < 1 || nc < 1) MGDT_FAIL(MGDT_BAD_SHAPE, "cls_loss_bwd: n=%d nc=%d", n, nc);
  cls_softmax_kernel<<<n, 256, 0, (hipStream_t)s>>>(logits, nc, dlogits, labels, gscale / CLS_DIV, 1);
  MGDT_CHECK_LAUNCH("cls_loss_bwd");
  return MGDT_OK;
}

// ================================================================================================ top-k + confusion matrix
struct ClsCand { float v; int i; };
__device__ __forceinline__ bool cls_better(ClsCand a, ClsCand b) { return a.v > b.v || (a.v == b.v && a.i < b.i); }

__global__ __launch_bounds__(256) void cls_topk_kernel(const float* __restrict__ probs, int nc, int n5, int64_t* __restrict__ topk, const int64_t* __restrict__ targets,
                                                       int32_t* __restrict__ matrix) {
  __shared__ float sv[256];
  __shared__ int si[256], so[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* r = probs + (long)b * nc;
  ClsCand loc[CLS_TOPK];                                                       // this thread's best, descending
#pragma unroll
  for (int q = 0; q < CLS_TOPK; ++q) loc[q] = ClsCand{-INFINITY, 0x7fffffff};
  for (int i = tid; i < nc; i += 256) {
    float v = r[i];
    if (v != v) v = -INFINITY;                                                 // NaN ranks last
    ClsCand c{v, i};
#pragma unroll
    for (int q = 0; q < CLS_TOPK; ++q)
      if (cls_better(c, loc[q])) { const ClsCand t = loc[q]; loc[q] = c; c = t; }
  }
  int head = 0;                                                                // next unused entry of loc
  for (int round = 0; round < n5; ++round) {
    ClsCand c{-INFINITY, 0x7fffffff};
#pragma unroll
    for (int q = 0; q < CLS_TOPK; ++q)
      if (q == head) c = loc[q];
    sv[tid] = c.v; si[tid] = c.i; so[tid] = tid;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
      if (tid < st && cls_better(ClsCand{sv[tid + st], si[tid + st]}, ClsCand{sv[tid], si[tid]})) {
        sv[tid] = sv[tid + st]; si[tid] = si[tid + st]; so[tid] = so[tid + st];
      }
      __syncthreads();
    }
    const int win = si[0], owner = so[0];
    if (tid == owner) ++head;
    if (tid == 0) {
      topk[(long)b * n5 + round] = win;
      if (round == 0 && matrix) {
        const long t = targets[b];
        if (win >= 0 && win < nc && t >= 0 && t < nc) atomicAdd(&matrix[(long)win * nc + t], 1);
      }
    }
    __syncthreads();
  }
}

extern "C" int mgdt_cls_topk_fwd(const float* probs, int n, int nc, int64_t* topk, const int64_t* targets, int32_t* matrix, mgdt_stream s) {
  if (!probs || !topk) MGDT_FAIL(MGDT_BAD_ARG, "cls_topk: null pointer");
  if (matrix && !targets) MGDT_FAIL(MGDT_BAD_ARG, "cls_topk: the confusion matrix needs the targets");
  if (n < 1 || nc < 1 || (matrix && (long)nc * nc > 0x7fffffffL)) MGDT_FAIL(MGDT_BAD_SHAPE, "cls_topk: n=%d nc=%d", n, nc);
  const int n5 = nc < CLS_TOPK ? nc : CLS_TOPK;
  cls_topk_kernel<<<n, 256, 0, (hipStream_t)s>>>(probs, nc, n5, topk, targets, matrix);
  MGDT_CHECK_LAUNCH("cls_topk_fwd");
  return MGDT_OK;
}
