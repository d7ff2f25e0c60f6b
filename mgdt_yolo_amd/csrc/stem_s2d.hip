// The 6x6 / stride 2 / padding 2 stem of the YOLOv5 graphs (models/v5/yolov5.yaml row 0) as space-to-depth + a 3x3 / stride 1 / padding 1 convolution:
//   S[b, (dy*2+dx)*C + ci, i, j] = x[b, ci, 2i+dy, 2j+dx]        W3[co, (dy*2+dx)*C + ci, a, b] = W6[co, ci, 2a+dy, 2b+dx]
//   conv2d(x, W6, stride 2, pad 2) == conv2d(S, W3, stride 1, pad 1)
// This file holds the two data movements around the existing kernels: the image -> S rearrangement in front of the MFMA implicit GEMM (forward) and of
// the 3x3 weight-gradient kernel (reverse), and the inverse permutation that turns that kernel's 3x3 result into the gradient of the 6x6 weight.
#include <algorithm>
#include <type_traits>

#include "common.h"

template <typename TX> __device__ __forceinline__ float img_val(TX v) {
  if constexpr (std::is_same<TX, uint8_t>::value) return (float)v / 255.0f;      // the preprocess division, exact (as conv2d_direct / stem2 / image_pad4)
  else return (float)v;
}

// One thread per output pixel: for every input channel two rows x two adjacent pixels (one 2-element load per row where the view allows it, so a wave
// reads whole contiguous runs of each input row, and every input row is read by one row of threads only), then CP / 4 (fp32) or CP / 8 (bf16) 16-byte stores
// of the pixel's channels, the pad channels zero.
template <typename TX, typename TY, int C>
__global__ __launch_bounds__(256) void space_to_depth2_kernel(const TX* __restrict__ x, long xsn, long xsc, long xsh, long xsw, int pair, TY* __restrict__ y,
                                                              long ysn, long ysh, long ysw, int N, int Ho, int Wo) {
  constexpr int VEC = std::is_same<TY, bf16>::value ? 8 : 4;
  constexpr int CP = (4 * C + VEC - 1) / VEC * VEC;
  typedef TX __attribute__((ext_vector_type(2))) TX2;
  const long total = (long)N * Ho * Wo;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int j = (int)(i % Wo);
    const long t = i / Wo;
    const int r = (int)(t % Ho);
    const long n = t / Ho;
    float v[CP];
#pragma unroll
    for (int k = 0; k < CP; ++k) v[k] = 0.f;
#pragma unroll
    for (int ci = 0; ci < C; ++ci) {
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const TX* p = x + n * xsn + ci * xsc + (2L * r + dy) * xsh + 2L * j * xsw;
        TX a, b;
        if (pair) {
          const TX2 ab = *(const TX2*)p;
          a = ab[0];
          b = ab[1];
        } else {
          a = p[0];
          b = p[xsw];
        }
        v[(dy * 2 + 0) * C + ci] = img_val<TX>(a);
        v[(dy * 2 + 1) * C + ci] = img_val<TX>(b);
      }
    }
    TY* q = y + n * ysn + r * ysh + j * ysw;
    if constexpr (std::is_same<TY, bf16>::value) {
#pragma unroll
      for (int k = 0; k < CP; k += 8) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)v[k + e];
        *(bf16x8*)(q + k) = o;
      }
    } else {
#pragma unroll
      for (int k = 0; k < CP; k += 4) *(f32x4*)(q + k) = f32x4{v[k], v[k + 1], v[k + 2], v[k + 3]};
    }
  }
}

extern "C" int mgdt_space_to_depth2_channels(int c, int y_dtype) {
  const int vec = y_dtype == MGDT_BF16 ? 8 : 4;
  return (4 * c + vec - 1) / vec * vec;
}

extern "C" int mgdt_space_to_depth2_fwd(const mgdt_view* x, int xdt, const mgdt_view* y, int ydt, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(y)) MGDT_FAIL(MGDT_BAD_ARG, "space_to_depth2: null/empty view");
  if (ydt != MGDT_F32 && ydt != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "space_to_depth2: y dtype %d", ydt);
  if (x->c < 1 || x->c > 4 || (x->h & 1) || (x->w & 1)) MGDT_FAIL(MGDT_BAD_SHAPE, "space_to_depth2: x with 1-4 channels and even h, w (got %d x %d x %d)", x->c, x->h, x->w);
  const int vec = ydt == MGDT_BF16 ? 8 : 4;
  if (y->c != mgdt_space_to_depth2_channels(x->c, ydt) || y->n != x->n || 2 * y->h != x->h || 2 * y->w != x->w || y->sc != 1 || y->sw % vec || y->sh % vec ||
      y->sn % vec || (uintptr_t)y->p % 16)
    MGDT_FAIL(MGDT_BAD_SHAPE, "space_to_depth2: y is the N x H/2 x W/2 x %d NHWC map, 16-byte aligned", mgdt_space_to_depth2_channels(x->c, ydt));
  const size_t xe = xdt == MGDT_U8 ? 1 : dtype_size(xdt);
  const int pair = x->sw == 1 && x->sh % 2 == 0 && x->sc % 2 == 0 && x->sn % 2 == 0 && (uintptr_t)x->p % (2 * xe) == 0;
  const long total = (long)y->n * y->h * y->w;
  const int g = (int)std::min<long>((total + 255) / 256, 16384);
  hipStream_t st = (hipStream_t)s;
#define LC(TX, TY, C) space_to_depth2_kernel<TX, TY, C><<<g, 256, 0, st>>>((const TX*)x->p, x->sn, x->sc, x->sh, x->sw, pair, (TY*)y->p, y->sn, y->sh, y->sw, y->n, y->h, y->w)
#define LP(TX, TY)                                                              \
  do {                                                                          \
    if (x->c == 3) LC(TX, TY, 3); else if (x->c == 4) LC(TX, TY, 4);            \
    else if (x->c == 1) LC(TX, TY, 1); else LC(TX, TY, 2);                      \
  } while (0)
  if (xdt == MGDT_U8 && ydt == MGDT_BF16) LP(uint8_t, bf16);
  else if (xdt == MGDT_U8 && ydt == MGDT_F32) LP(uint8_t, float);
  else if (xdt == MGDT_F32 && ydt == MGDT_F32) LP(float, float);
  else if (xdt == MGDT_F32 && ydt == MGDT_BF16) LP(float, bf16);
  else if (xdt == MGDT_BF16 && ydt == MGDT_BF16) LP(bf16, bf16);
  else MGDT_FAIL(MGDT_BAD_DTYPE, "space_to_depth2: dtypes %d -> %d", xdt, ydt);
#undef LP
#undef LC
  MGDT_CHECK_LAUNCH("space_to_depth2_fwd");
  return MGDT_OK;
}

// dw6[co][ci][2a+dy][2b+dx] = dw3[co][(dy*2+dx)*cin + ci][a][b]: the gradient of the 6x6 weight from the 3x3 weight-gradient kernel's FINAL sums over S
// (dw3: fp32 [cout][cp][3][3], cp >= 4*cin; its rows past 4*cin - the zero pad channels of S - are not read).  Overwrites dw6 (fp32 [cout][cin][6][6]).
__global__ __launch_bounds__(256) void stem6_wgrad_unpack_kernel(const float* __restrict__ dw3, float* __restrict__ dw6, int cout, int cin, int cp) {
  const int total = cout * cin * 36;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int c = i % 6, r = (i / 6) % 6;
    const int ci = (i / 36) % cin, co = i / (36 * cin);
    const int q = (r & 1) * 2 + (c & 1);
    dw6[i] = dw3[(((long)co * cp + q * cin + ci) * 3 + (r >> 1)) * 3 + (c >> 1)];
  }
}

extern "C" int mgdt_stem6_wgrad_unpack(const float* dw3, int cout, int cin, int cp, float* dw6, mgdt_stream s) {
  if (!dw3 || !dw6) MGDT_FAIL(MGDT_BAD_ARG, "stem6_wgrad_unpack: null pointer");
  if (cout < 1 || cin < 1 || cin > 4 || cp < 4 * cin || cout > (1 << 16)) MGDT_FAIL(MGDT_BAD_SHAPE, "stem6_wgrad_unpack: cout %d cin %d cp %d", cout, cin, cp);
  const int total = cout * cin * 36;
  stem6_wgrad_unpack_kernel<<<std::min((total + 255) / 256, 4096), 256, 0, (hipStream_t)s>>>(dw3, dw6, cout, cin, cp);
  MGDT_CHECK_LAUNCH("stem6_wgrad_unpack");
  return MGDT_OK;
}
