// Max-pool layers of the YOLOv3 graphs: nn.MaxPool2d(2, 2) / nn.MaxPool2d(2, 1) forward and reverse (models/v3/yolov3-tiny.yaml), and the reverse
// pass of SPP's three direct windows (nn/modules/block.py:121-135).  ATen's semantics throughout, as pointwise.hip's SPPF pools and train_vec.hip's
// maxpool5_bwd follow them: a NaN in a window is the window's maximum (IEEE maximum, not fmaxf); in the reverse pass the gradient goes to the first
// maximum in (ky, kx) scan order and a NaN replaces what was found before it, so -0.0 and 0.0 tie and the first one wins; a window of -inf only keeps
// its first element.  Every reverse pass is a gather in a fixed order: no float atomics, the same bits on every run and under capture.
#include <algorithm>

#include "common.h"

__device__ __forceinline__ float pl_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
static inline int pl_grid(long total) { return (int)std::min<long>((total + 255) / 256, 65536); }

// V channels per lane: 16-byte accesses (8 bf16 / 4 fp32) or one element
template <typename T, int V>
__device__ __forceinline__ void pl_ld(const T* p, float* v) {
  if constexpr (V == 1) {
    v[0] = ldf<T>(p);
  } else if constexpr (sizeof(T) == 4) {
    const f32x4 t = *(const f32x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = t[j];
  } else {
    const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
  }
}
template <typename T, int V>
__device__ __forceinline__ void pl_st(T* p, const float* v) {
  if constexpr (V == 1) {
    stf<T>(p, v[0]);
  } else if constexpr (sizeof(T) == 4) {
    *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (bf16)v[j];
    *(bf16x8*)p = t;
  }
}
static bool pl_vec_ok(const mgdt_view* v, int V) {
  return v->c % V == 0 && v->sw % V == 0 && v->sh % V == 0 && v->sn % V == 0 && (uintptr_t)v->p % 16 == 0;
}

#define PL_DECODE(i, v, V, N_, H_, W_, C_) \
  const int Q_ = (v).c / V;                \
  const int C_ = (int)((i) % Q_) * V;      \
  long t_ = (i) / Q_;                      \
  const int W_ = (int)(t_ % (v).w);        \
  t_ /= (v).w;                             \
  const int H_ = (int)(t_ % (v).h);        \
  const long N_ = t_ / (v).h;

// y[oy][ox] = max of x[oy*s .. oy*s+1][ox*s .. ox*s+1]; the host checked y.h == (x.h - 2) / s + 1 (and w), so every tap is inside the map
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const mgdt_view x, const mgdt_view y, int s) {
  const long total = (long)y.n * y.h * y.w * (y.c / V);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    PL_DECODE(i, y, V, n, oy, ox, c)
    const T* xb = (const T*)x.p + n * x.sn + (long)(oy * s) * x.sh + (long)(ox * s) * x.sw + c;
    float a[V], b[V], d[V], e[V];
    pl_ld<T, V>(xb, a);
    pl_ld<T, V>(xb + x.sw, b);
    pl_ld<T, V>(xb + x.sh, d);
    pl_ld<T, V>(xb + x.sh + x.sw, e);
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = pl_max(pl_max(a[j], b[j]), pl_max(d[j], e[j]));
    pl_st<T, V>((T*)y.p + n * y.sn + (long)oy * y.sh + (long)ox * y.sw + c, a);
  }
}

// the window whose top-left corner is xb: adds g where the window's argmax (first maximum in scan order, a NaN replaces what came before) is tap `mine`
template <typename T, int V>
__device__ __forceinline__ void pl_window_bwd(const T* xb, long sh, long sw, const T* gp, int mine, float* acc) {
  float v[4][V], g[V];
  pl_ld<T, V>(xb, v[0]);
  pl_ld<T, V>(xb + sw, v[1]);
  pl_ld<T, V>(xb + sh, v[2]);
  pl_ld<T, V>(xb + sh + sw, v[3]);
  pl_ld<T, V>(gp, g);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float best = -INFINITY;
    int bt = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (v[t][j] > best || isnan(v[t][j])) { best = v[t][j]; bt = t; }
    acc[j] += bt == mine ? g[j] : 0.f;
  }
}

// One lane = V channels of one INPUT pixel: it sums gy over the windows that contain it (one for stride 2, up to four for stride 1, in (oy, ox)
// order) and whose argmax it is; a pixel no window reads (the odd trailing row / column at stride 2) gets 0.  gx is written in the activation type.
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const mgdt_view x, const mgdt_view gy, const mgdt_view gx, int s) {
  const long total = (long)x.n * x.h * x.w * (x.c / V);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    PL_DECODE(i, x, V, n, h, w, c)
    const T* xn = (const T*)x.p + n * x.sn + c;
    const T* gn = (const T*)gy.p + n * gy.sn + c;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (s == 2) {
      const int oy = h >> 1, ox = w >> 1;
      if (oy < gy.h && ox < gy.w)
        pl_window_bwd<T, V>(xn + (long)(2 * oy) * x.sh + (long)(2 * ox) * x.sw, x.sh, x.sw, gn + (long)oy * gy.sh + (long)ox * gy.sw, (h & 1) * 2 + (w & 1), acc);
    } else {
      for (int oy = h - 1; oy <= h; ++oy) {
        if ((unsigned)oy >= (unsigned)gy.h) continue;
        for (int ox = w - 1; ox <= w; ++ox) {
          if ((unsigned)ox >= (unsigned)gy.w) continue;
          pl_window_bwd<T, V>(xn + (long)oy * x.sh + (long)ox * x.sw, x.sh, x.sw, gn + (long)oy * gy.sh + (long)ox * gy.sw, (h - oy) * 2 + (w - ox), acc);
        }
      }
    }
    pl_st<T, V>((T*)gx.p + n * gx.sn + (long)h * gx.sh + (long)w * gx.sw + c, acc);
  }
}

static int maxpool2d_check(const char* what, const mgdt_view* x, const mgdt_view* y, int k, int stride) {
  if (!view_ok(x) || !view_ok(y)) MGDT_FAIL(MGDT_BAD_ARG, "%s: null/empty argument", what);
  if (k != 2 || (stride != 1 && stride != 2)) MGDT_FAIL(MGDT_BAD_ARG, "%s: kernel 2 with stride 1 or 2 is built, got kernel %d stride %d", what, k, stride);
  if (x->sc != 1 || y->sc != 1) MGDT_FAIL(MGDT_BAD_SHAPE, "%s: NHWC views", what);
  if (x->h < 2 || x->w < 2 || y->n != x->n || y->c != x->c || y->h != (x->h - 2) / stride + 1 || y->w != (x->w - 2) / stride + 1)
    MGDT_FAIL(MGDT_BAD_SHAPE, "%s: input %dx%dx%dx%d needs an output %dx%dx%dx%d, got %dx%dx%dx%d", what, x->n, x->h, x->w, x->c, x->n,
              x->h < 2 ? 0 : (x->h - 2) / stride + 1, x->w < 2 ? 0 : (x->w - 2) / stride + 1, x->c, y->n, y->h, y->w, y->c);
  return MGDT_OK;
}

#define PL_DISPATCH(dtype, vec, ...)                                                            \
  do {                                                                                          \
    if ((dtype) == MGDT_F32) { using T = float; if (vec) { constexpr int V = 4; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } }      \
    else if ((dtype) == MGDT_BF16) { using T = bf16; if (vec) { constexpr int V = 8; __VA_ARGS__; } else { constexpr int V = 1; __VA_ARGS__; } } \
    else MGDT_FAIL(MGDT_BAD_DTYPE, "unsupported dtype %d", (int)(dtype));                       \
  } while (0)

extern "C" int mgdt_maxpool2d_fwd(const mgdt_view* x, const mgdt_view* y, int k, int stride, int dtype, mgdt_stream s) {
  if (int e = maxpool2d_check("maxpool2d_fwd", x, y, k, stride)) return e;
  const int VN = dtype == MGDT_BF16 ? 8 : 4;
  const bool vec = pl_vec_ok(x, VN) && pl_vec_ok(y, VN);
  const long total = (long)y->n * y->h * y->w * (y->c / (vec ? VN : 1));
  PL_DISPATCH(dtype, vec, (maxpool2_fwd_kernel<T, V><<<pl_grid(total), 256, 0, (hipStream_t)s>>>(*x, *y, stride)));
  MGDT_CHECK_LAUNCH("maxpool2d_fwd");
  return MGDT_OK;
}

extern "C" int mgdt_maxpool2d_bwd(const mgdt_view* x, const mgdt_view* gy, const mgdt_view* gx, int k, int stride, int dtype, mgdt_stream s) {
  if (int e = maxpool2d_check("maxpool2d_bwd", x, gy, k, stride)) return e;
  if (!view_ok(gx)) MGDT_FAIL(MGDT_BAD_ARG, "maxpool2d_bwd: null/empty argument");
  if (gx->sc != 1 || gx->n != x->n || gx->h != x->h || gx->w != x->w || gx->c != x->c) MGDT_FAIL(MGDT_BAD_SHAPE, "maxpool2d_bwd: gx has the shape of x");
  const int VN = dtype == MGDT_BF16 ? 8 : 4;
  const bool vec = pl_vec_ok(x, VN) && pl_vec_ok(gy, VN) && pl_vec_ok(gx, VN);
  const long total = (long)x->n * x->h * x->w * (x->c / (vec ? VN : 1));
  PL_DISPATCH(dtype, vec, (maxpool2_bwd_kernel<T, V><<<pl_grid(total), 256, 0, (hipStream_t)s>>>(*x, *gy, *gx, stride)));
  MGDT_CHECK_LAUNCH("maxpool2d_bwd");
  return MGDT_OK;
}

// ------------------------------------------------------------------------------------------------ SPP reverse pass
// gx = sum over k in (5, 9, 13) of the adjoint of MaxPool2d(k, 1, k / 2) at x, applied to g_k.  The first maximum of a window in row-major scan
// order is separable: it lies in the first row whose row maximum equals the window's maximum (a NaN: the last row that holds one), at the first
// column of that row that holds the row maximum (the last NaN).  So per window size, with r = k / 2:
//   A  RM[y][ox], RC[y][ox] = maximum and its column over x[y][ox - r .. ox + r]                 (k taps)
//   B  AR[oy][ox]           = the row of the maximum over RM[oy - r .. oy + r][ox]               (k taps): window (oy, ox) has its argmax at (AR, RC[AR][ox])
//   C  TT[h][ox]            = sum over oy of g[oy][ox] where AR[oy][ox] == h, oy ascending       (k taps)
//   D  gx[h][w]            += sum over ox of TT[h][ox] where RC[h][ox] == w, ox ascending         (k taps)
// 4 k taps per pixel instead of the k^2 of a direct gather.  The order of the sums is fixed (per window size: ox ascending, within it oy ascending;
// then 5, 9, 13), and the global-memory route below adds in the same order, so both give the same bits.
// LDS route: workgroup = (image, CB channels; CB = 16 / 8 / 4, the largest whose planes stay within 16 KB, else 4), the whole plane in LDS, 10 bytes per pixel and channel: x and RM / TT in fp32, RC and AR as byte
// offsets from the window's first column / row (<= 12).  The windows are clipped by their loop bounds, so no halo is stored.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void spp_bwd_lds_kernel(const mgdt_view x, const mgdt_view g5, const mgdt_view g9, const mgdt_view g13, float* __restrict__ gx, int CB) {
  extern __shared__ __attribute__((aligned(16))) float spp_sm[];
  const int H = x.h, W = x.w, HW = H * W, n = blockIdx.x, c0 = blockIdx.y * CB;
  const int cb = min(CB, x.c - c0);                     // channels of this block that exist
  const int N = HW * CB;
  float* X = spp_sm;
  float* RM = spp_sm + N;                               // phase C onwards: TT
  unsigned char* RC = (unsigned char*)(RM + N);
  unsigned char* AR = RC + N;
  if (VEC) {                                            // x.c % 4 == 0: a quad of channels exists as a whole or not at all
    const int QB = CB >> 2;
    for (int i = threadIdx.x; i < HW * QB; i += 256) {
      const int p = i / QB, q = i - p * QB;
      const int y = p / W, xx = p - y * W;
      *(f32x4*)(X + p * CB + 4 * q) = 4 * q < cb ? load4<T>((const T*)x.p + (long)n * x.sn + (long)y * x.sh + (long)xx * x.sw + c0 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  } else {
    for (int i = threadIdx.x; i < N; i += 256) {
      const int p = i / CB, c = i - p * CB;
      const int y = p / W, xx = p - y * W;
      X[i] = c < cb ? ldf<T>((const T*)x.p + (long)n * x.sn + (long)y * x.sh + (long)xx * x.sw + c0 + c) : 0.f;
    }
  }
  __syncthreads();
  for (int kk = 0; kk < 3; ++kk) {
    const int r = 2 + 2 * kk;
    const mgdt_view& g = kk == 0 ? g5 : kk == 1 ? g9 : g13;
    for (int i = threadIdx.x; i < N; i += 256) {        // A
      const int p = i / CB, c = i - p * CB;
      const int y = p / W, ox = p - y * W;
      const int lo = max(ox - r, 0), hi = min(ox + r, W - 1);
      float best = -INFINITY;
      int bc = lo;
      for (int xx = lo; xx <= hi; ++xx) {
        const float v = X[(y * W + xx) * CB + c];
        if (v > best || isnan(v)) { best = v; bc = xx; }
      }
      RM[i] = best;
      RC[i] = (unsigned char)(bc - (ox - r));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {        // B
      const int p = i / CB, c = i - p * CB;
      const int oy = p / W, ox = p - oy * W;
      const int lo = max(oy - r, 0), hi = min(oy + r, H - 1);
      float best = -INFINITY;
      int br = lo;
      for (int yy = lo; yy <= hi; ++yy) {
        const float v = RM[(yy * W + ox) * CB + c];
        if (v > best || isnan(v)) { best = v; br = yy; }
      }
      AR[i] = (unsigned char)(br - (oy - r));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {        // C (RM is dead: it becomes TT)
      const int p = i / CB, c = i - p * CB;
      const int h = p / W, ox = p - h * W;
      float acc = 0.f;
      if (c < cb) {
        const int lo = max(h - r, 0), hi = min(h + r, H - 1);
        const T* gp = (const T*)g.p + (long)n * g.sn + (long)ox * g.sw + c0 + c;
        for (int oy = lo; oy <= hi; ++oy)
          if ((int)AR[(oy * W + ox) * CB + c] + oy - r == h) acc += ldf<T>(gp + (long)oy * g.sh);
      }
      RM[i] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {        // D: element i belongs to the same lane for all three window sizes
      const int p = i / CB, c = i - p * CB;
      if (c >= cb) continue;
      const int h = p / W, w = p - h * W;
      const int lo = max(w - r, 0), hi = min(w + r, W - 1);
      float acc = 0.f;
      for (int ox = lo; ox <= hi; ++ox)
        if ((int)RC[(h * W + ox) * CB + c] + ox - r == w) acc += RM[(h * W + ox) * CB + c];
      float* o = gx + ((long)n * HW + p) * x.c + c0 + c;
      *o = kk == 0 ? acc : *o + acc;
    }
    __syncthreads();
  }
}

// maximum of x[y][ox - r .. ox + r] (clipped) and its column, in scan order
template <typename T>
__device__ __forceinline__ float spp_row_max(const T* xb, long sh, long sw, int W, int y, int ox, int r, int& col) {
  const int lo = max(ox - r, 0), hi = min(ox + r, W - 1);
  float best = -INFINITY;
  col = lo;
  for (int xx = lo; xx <= hi; ++xx) {
    const float v = ldf<T>(xb + (long)y * sh + (long)xx * sw);
    if (v > best || isnan(v)) { best = v; col = xx; }
  }
  return best;
}

// Any plane size, straight from global memory, one lane per element: the same tests and the same order of the sums as the LDS route.
template <typename T>
__global__ __launch_bounds__(256) void spp_bwd_scalar_kernel(const mgdt_view x, const mgdt_view g5, const mgdt_view g9, const mgdt_view g13, float* __restrict__ gx) {
  const long total = (long)x.n * x.h * x.w * x.c;
  const int H = x.h, W = x.w;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    PL_DECODE(i, x, 1, n, h, w, c)
    const T* xb = (const T*)x.p + n * x.sn + c;
    float sum = 0.f;
    for (int kk = 0; kk < 3; ++kk) {
      const int r = 2 + 2 * kk;
      const mgdt_view& g = kk == 0 ? g5 : kk == 1 ? g9 : g13;
      const T* gb = (const T*)g.p + n * g.sn + c;
      float acc = 0.f;
      for (int ox = max(w - r, 0); ox <= min(w + r, W - 1); ++ox) {
        int col;
        spp_row_max<T>(xb, x.sh, x.sw, W, h, ox, r, col);
        if (col != w) continue;
        float tt = 0.f;
        for (int oy = max(h - r, 0); oy <= min(h + r, H - 1); ++oy) {
          float best = -INFINITY;
          int br = max(oy - r, 0), dummy;
          for (int yy = max(oy - r, 0); yy <= min(oy + r, H - 1); ++yy) {
            const float v = spp_row_max<T>(xb, x.sh, x.sw, W, yy, ox, r, dummy);
            if (v > best || isnan(v)) { best = v; br = yy; }
          }
          if (br == h) tt += ldf<T>(gb + (long)oy * g.sh + (long)ox * g.sw);
        }
        acc += tt;
      }
      sum = kk == 0 ? acc : sum + acc;
    }
    gx[((n * H + h) * W + w) * x.c + c] = sum;
  }
}

static bool spp_v4_ok(const mgdt_view* v, int dtype) {
  return v->c % 4 == 0 && v->sw % 4 == 0 && v->sh % 4 == 0 && v->sn % 4 == 0 && (uintptr_t)v->p % (4 * dtype_size(dtype)) == 0;
}

// gx_f32: dense fp32 [n][h][w][c], every element written (no need to zero it).
extern "C" int mgdt_spp_pool_bwd(const mgdt_view* x, const mgdt_view* g5, const mgdt_view* g9, const mgdt_view* g13, float* gx_f32, int dtype, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(g5) || !view_ok(g9) || !view_ok(g13) || !gx_f32) MGDT_FAIL(MGDT_BAD_ARG, "spp_pool_bwd: null/empty argument");
  for (const mgdt_view* g : {g5, g9, g13})
    if (x->sc != 1 || g->sc != 1 || x->n != g->n || x->h != g->h || x->w != g->w || x->c != g->c) MGDT_FAIL(MGDT_BAD_SHAPE, "spp_pool_bwd: matching NHWC views");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "unsupported dtype %d", dtype);
  const long HW = (long)x->h * x->w;
  if (HW * 4 * 10 <= 64 * 1024) {
    int CB = 16;                // small channel blocks: the phases are chains of dependent LDS reads, so what hides their latency is waves per CU (<= 16 KB: 8+ workgroups)
    while (CB > 4 && (HW * CB * 10 > 16 * 1024 || CB >= 2 * x->c)) CB >>= 1;
    const size_t lds = (size_t)HW * CB * 10;
    const dim3 grid(x->n, (x->c + CB - 1) / CB);
    if (spp_v4_ok(x, dtype))
      MGDT_DISPATCH_DTYPE(dtype, (spp_bwd_lds_kernel<T, true><<<grid, 256, lds, (hipStream_t)s>>>(*x, *g5, *g9, *g13, gx_f32, CB)));
    else
      MGDT_DISPATCH_DTYPE(dtype, (spp_bwd_lds_kernel<T, false><<<grid, 256, lds, (hipStream_t)s>>>(*x, *g5, *g9, *g13, gx_f32, CB)));
  } else {
    const long total = (long)x->n * HW * x->c;
    MGDT_DISPATCH_DTYPE(dtype, (spp_bwd_scalar_kernel<T><<<pl_grid(total), 256, 0, (hipStream_t)s>>>(*x, *g5, *g9, *g13, gx_f32)));
  }
  MGDT_CHECK_LAUNCH("spp_pool_bwd");
  return MGDT_OK;
}
