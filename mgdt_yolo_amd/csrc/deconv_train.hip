// Reverse pass of nn.ConvTranspose2d(cin, cout, 2, 2, 0) (models/v6/yolov6.yaml rows 11 and 16; forward: mgdt_deconv2x2_fwd in segment.hip).
// Kernel size == stride, so output pixel (2y + ky, 2x + kx) depends on input pixel (y, x) alone and both gradients are plain GEMMs over a
// 2x2 gather of dy (N x 2H x 2W x cout NHWC), with the weight read in the parameter's own layout w[cin][cout][2][2] fp32:
//
//   deconv2x2_dgrad   dx[b, y, x, ci] = sum_{ky, kx, co} w[ci][co][ky][kx] * dy[b, 2y+ky, 2x+kx, co]  [+ r1] [+ r2]
//                     One GEMM with M = pixels of dx, N = cin, K = 4 cout.  A workgroup keeps w for its NT input channels in LDS as
//                     Ws[phase][ci][co] (zero rows / columns for the padding), each of its 4 waves owns 16 pixels of a 64-pixel tile and
//                     walks K in the fixed order (phase, co); workgroups are persistent over the pixel tiles.  The A operand is loaded straight
//                     from dy (16 bytes fp32 / 8 bytes bf16 per lane: 4 consecutive channels of the lane's pixel).
//   deconv2x2_wgrad   dw[ci][co][ky][kx] = sum_{b, y, x} x[b, y, x, ci] * dy[b, 2y+ky, 2x+kx, co]
//                     One GEMM with M = cin, N = 4 cout (column = phase * coutP + co), K = pixels.  The reduction index is the slow index of
//                     both NHWC tensors; with the fp32 16x16x4 MFMA a lane supplies ONE element per operand (row i, k = g), so chunks of 32
//                     pixels staged in LDS as [pixel][channel] rows are read without any transpose.  Workgroups split the pixels (grid.x) and the
//                     (cin, column) tiles (grid.y); split s leaves its sums in partial[s][cin][cout][2][2] - the parameter's layout - and
//                     mgdt_wgrad_final_batch (train.hip) adds the splits in its fixed order: no unpack launch, and the layer takes part in
//                     ops.defer_wgrad() like every convolution.
//
// Both kernels multiply on the fp32 matrix cores whatever the tensors' dtype (bf16 values are widened exactly; accumulation is fp32): the layer
// is two rows of the graph and bound by its memory traffic.  Every sum has one fixed association: results are bit-equal from run to run.
#include "common.h"

#include <algorithm>

#define DC_LDS_MAX (64 * 1024)
#define DC_NBMAX 4            // 16-channel blocks of dx per workgroup (deconv2x2_dgrad)

struct DcDxArgs {
  const void* dy; long dsn, dsh, dsw;
  const float* w;
  void* dx; long xsn, xsh, xsw;
  const void* r1; long r1sn, r1sh, r1sw;
  const void* r2; long r2sn, r2sh, r2sw;
  int H, W, Cin, Cout, CoutP, NB, pitch, mtiles;
  long M;
};

template <typename T>
__global__ __launch_bounds__(256) void deconv2x2_dgrad_kernel(const DcDxArgs a) {
  extern __shared__ __attribute__((aligned(16))) float dc_ws[];                 // [4][NT][pitch]
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
  const int NT = a.NB * 16, n0 = blockIdx.y * NT;
  {                                                                                // the weights of this workgroup's input channels, once
    const int total = NT * a.CoutP * 4;
    for (int e = tid; e < total; e += 256) {
      const int ph = e & 3, q = e >> 2, n = q / a.CoutP, co = q - n * a.CoutP, ci = n0 + n;
      dc_ws[(ph * NT + n) * a.pitch + co] = (ci < a.Cin && co < a.Cout) ? a.w[((long)ci * a.Cout + co) * 4 + ph] : 0.f;
    }
  }
  __syncthreads();
  const long HW = (long)a.H * a.W;
  const T* dyp = (const T*)a.dy;
  for (int tile = blockIdx.x; tile < a.mtiles; tile += gridDim.x) {
    const long m0 = (long)tile * 64 + wave * 16;
    const long m = m0 + i;
    const bool valid = m < a.M;
    long base = 0;
    if (valid) {
      const long b = m / HW, r = m - b * HW;
      const long y = r / a.W, x = r - y * a.W;
      base = b * a.dsn + 2 * y * a.dsh + 2 * x * a.dsw;
    }
    f32x4 acc[DC_NBMAX];
#pragma unroll
    for (int nb = 0; nb < DC_NBMAX; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ph = 0; ph < 4; ++ph) {
      const T* p = dyp + base + (ph >> 1) * a.dsh + (ph & 1) * a.dsw;
      const float* wsp = dc_ws + (long)(ph * NT + i) * a.pitch;
      for (int co0 = 0; co0 < a.CoutP; co0 += 16) {
        const int c = co0 + 4 * g;                                                 // Cout % 4 == 0: the four channels are in range together
        const f32x4 av = (valid && c < a.Cout) ? load4<T>(p + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nb = 0; nb < DC_NBMAX; ++nb) {
          if (nb < a.NB) {
            const f32x4 bv = *(const f32x4*)(wsp + nb * 16 * a.pitch + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc[nb], 0, 0, 0);
          }
        }
      }
    }
    // D layout: lane (i, g) holds pixels 4g .. 4g+3 of the wave's 16 (rows), input channel i of block nb (column)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long mr = m0 + 4 * g + r;
      if (mr >= a.M) continue;
      const long b = mr / HW, q = mr - b * HW;
      const long y = q / a.W, x = q - y * a.W;
#pragma unroll
      for (int nb = 0; nb < DC_NBMAX; ++nb) {
        const int ci = n0 + nb * 16 + i;
        if (nb >= a.NB || ci >= a.Cin) continue;
        float v = acc[nb][r];
        if (a.r1) v += ldf<T>((const T*)a.r1 + b * a.r1sn + y * a.r1sh + x * a.r1sw + ci);
        if (a.r2) v += ldf<T>((const T*)a.r2 + b * a.r2sn + y * a.r2sh + x * a.r2sw + ci);
        stf<T>((T*)a.dx + b * a.xsn + y * a.xsh + x * a.xsw + ci, v);
      }
    }
  }
}

static bool dc_vec_view(const mgdt_view* v, int dtype) {        // 4-channel vector loads: NHWC, channels / strides in fours, aligned base
  return v->sc == 1 && v->c % 4 == 0 && v->sn % 4 == 0 && v->sh % 4 == 0 && v->sw % 4 == 0 && (uintptr_t)v->p % (4 * dtype_size(dtype)) == 0;
}

extern "C" int mgdt_deconv2x2_dgrad(const mgdt_view* dy, const float* w, const mgdt_view* r1, const mgdt_view* r2, const mgdt_view* dx, int dtype,
                                    mgdt_stream s) {
  if (!view_ok(dy) || !view_ok(dx) || !w) MGDT_FAIL(MGDT_BAD_ARG, "deconv2x2_dgrad: null/empty argument");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "deconv2x2_dgrad: dtype %d", dtype);
  if (dy->n != dx->n || dy->h != 2 * dx->h || dy->w != 2 * dx->w)
    MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_dgrad: dy is %dx%dx%d, expected %dx%dx%d (kernel 2, stride 2, padding 0)", dy->n, dy->h, dy->w, dx->n, 2 * dx->h, 2 * dx->w);
  if (!dc_vec_view(dy, dtype) || dx->sc != 1 || dx->c % 4)
    MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_dgrad: NHWC views with channels %% 4 == 0; dy with strides %% 4 == 0 and a base aligned to 4 elements");
  for (const mgdt_view* r : {r1, r2})
    if (r && r->p && (r->sc != 1 || r->n != dx->n || r->h != dx->h || r->w != dx->w || r->c != dx->c))
      MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_dgrad: an addend must be an NHWC view shaped like dx");
  DcDxArgs a;
  memset(&a, 0, sizeof(a));
  a.M = (long)dx->n * dx->h * dx->w;
  if (a.M >= 0x7fffffffL / 64) MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_dgrad: too many pixels");
  a.dy = dy->p; a.dsn = dy->sn; a.dsh = dy->sh; a.dsw = dy->sw;
  a.w = w;
  a.dx = dx->p; a.xsn = dx->sn; a.xsh = dx->sh; a.xsw = dx->sw;
  if (r1 && r1->p) { a.r1 = r1->p; a.r1sn = r1->sn; a.r1sh = r1->sh; a.r1sw = r1->sw; }
  if (r2 && r2->p) { a.r2 = r2->p; a.r2sn = r2->sn; a.r2sh = r2->sh; a.r2sw = r2->sw; }
  a.H = dx->h; a.W = dx->w; a.Cin = dx->c; a.Cout = dy->c;
  a.CoutP = (a.Cout + 15) / 16 * 16;
  a.pitch = a.CoutP + 4;
  a.NB = std::min(DC_NBMAX, cdiv(a.Cin, 16));
  while (a.NB > 1 && (size_t)4 * a.NB * 16 * a.pitch * sizeof(float) > DC_LDS_MAX) --a.NB;
  const size_t lds = (size_t)4 * a.NB * 16 * a.pitch * sizeof(float);
  if (lds > DC_LDS_MAX) MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_dgrad: cout %d exceeds the LDS weight tile (compose the four phases instead)", a.Cout);
  a.mtiles = cdiv(a.M, 64);
  dim3 grid(std::min(a.mtiles, 512), cdiv(a.Cin, a.NB * 16));
  MGDT_DISPATCH_DTYPE(dtype, (deconv2x2_dgrad_kernel<T><<<grid, 256, lds, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("deconv2x2_dgrad");
  return MGDT_OK;
}

// ================================================================================================ weight gradient
#define DW_KP 32              // pixels per staged chunk
#define DW_CT 64              // input channels per workgroup (4 blocks of 16)
#define DW_NT 256             // (phase, cout) columns per workgroup (4 waves x 4 blocks of 16)
#define DW_XP (DW_CT + 16)    // LDS row pitches (floats): the four pixel rows a wave reads together start 16 banks apart
#define DW_DP (DW_NT + 16)
#define DW_MAX_SPLITS 256

struct DcDwArgs {
  const void* x; long xsn, xsh, xsw;
  const void* dy; long dsn, dsh, dsw;
  float* partial;
  int H, W, Cin, Cout, CoutP, NCOL, ncolg, nsplit;
  long M;
};

template <typename T>
__global__ __launch_bounds__(256) void deconv2x2_wgrad_kernel(const DcDwArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[DW_KP * DW_XP];
  __shared__ __attribute__((aligned(16))) float ds[DW_KP * DW_DP];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4, wave = tid >> 6;
  const int split = blockIdx.x, cig = blockIdx.y / a.ncolg, colg = blockIdx.y - cig * a.ncolg;
  const int ci0 = cig * DW_CT, col0 = colg * DW_NT;
  const long HW = (long)a.H * a.W;
  const long q0 = (long)split * a.M / a.nsplit, q1 = (long)(split + 1) * a.M / a.nsplit;
  const T* xp = (const T*)a.x;
  const T* dp = (const T*)a.dy;
  f32x4 acc[4][4];
#pragma unroll
  for (int ma = 0; ma < 4; ++ma)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[ma][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long p0 = q0; p0 < q1; p0 += DW_KP) {
    __syncthreads();                                                              // the previous chunk's fragments have been read
    for (int it = tid; it < DW_KP * (DW_CT / 4); it += 256) {
      const int pix = it / (DW_CT / 4), v4 = it - pix * (DW_CT / 4), ci = ci0 + v4 * 4;
      const long m = p0 + pix;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < q1 && ci < a.Cin) {
        const long b = m / HW, r = m - b * HW;
        const long y = r / a.W, x = r - y * a.W;
        v = load4<T>(xp + b * a.xsn + y * a.xsh + x * a.xsw + ci);
      }
      *(f32x4*)&xs[pix * DW_XP + v4 * 4] = v;
    }
    for (int it = tid; it < DW_KP * (DW_NT / 4); it += 256) {
      const int pix = it / (DW_NT / 4), v4 = it - pix * (DW_NT / 4), col = col0 + v4 * 4;
      const int ph = col / a.CoutP, co = col - ph * a.CoutP;
      const long m = p0 + pix;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < q1 && col < a.NCOL && co < a.Cout) {
        const long b = m / HW, r = m - b * HW;
        const long y = r / a.W, x = r - y * a.W;
        v = load4<T>(dp + b * a.dsn + (2 * y + (ph >> 1)) * a.dsh + (2 * x + (ph & 1)) * a.dsw + co);
      }
      *(f32x4*)&ds[pix * DW_DP + v4 * 4] = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < DW_KP / 4; ++ks) {
      const int row = ks * 4 + g;                                                 // A[ci i][pixel g], B[pixel g][column i]
      float av[4], bv[4];
#pragma unroll
      for (int ma = 0; ma < 4; ++ma) av[ma] = xs[row * DW_XP + ma * 16 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = ds[row * DW_DP + (wave * 4 + j) * 16 + i];
#pragma unroll
      for (int ma = 0; ma < 4; ++ma)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ma][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ma], bv[j], acc[ma][j], 0, 0, 0);
    }
  }
  // D layout: lane (i, g) holds input channels 4g .. 4g+3 of block ma (rows), column i of the wave's block j
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = col0 + (wave * 4 + j) * 16 + i;
    const int ph = col / a.CoutP, co = col - ph * a.CoutP;
    if (col >= a.NCOL || co >= a.Cout) continue;
#pragma unroll
    for (int ma = 0; ma < 4; ++ma)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = ci0 + ma * 16 + 4 * g + r;
        if (ci < a.Cin) a.partial[(((long)split * a.Cin + ci) * a.Cout + co) * 4 + ph] = acc[ma][j][r];
      }
  }
}

static inline int dw_groups(int cin, int cout) { return cdiv(cin, DW_CT) * cdiv(4 * ((cout + 15) / 16 * 16), DW_NT); }

// pixel splits: enough workgroups for the chip whatever the channel tiles; a function of the channel counts alone, so a layer's partial rows
// (and the order of their final sum) never depend on the batch
extern "C" int mgdt_deconv2x2_wgrad_splits(int cin, int cout) {
  if (cin < 1 || cout < 1) return 0;
  const long cap = (32L << 20) / ((long)cin * cout * 16);            // the partial rows stay under 32 MB (one split, whatever its size, past 1448 x 1448 channels)
  return (int)std::max(1L, std::min<long>({DW_MAX_SPLITS, 1024 / dw_groups(cin, cout), cap}));
}

extern "C" size_t mgdt_deconv2x2_wgrad_workspace_bytes(int cin, int cout) {
  if (cin < 1 || cout < 1) return 0;
  return (size_t)mgdt_deconv2x2_wgrad_splits(cin, cout) * cin * cout * 4 * sizeof(float);
}

extern "C" int mgdt_deconv2x2_wgrad(const mgdt_view* x, const mgdt_view* dy, float* dw, int accumulate, void* ws, int dtype, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(dy) || !ws) MGDT_FAIL(MGDT_BAD_ARG, "deconv2x2_wgrad: null/empty argument");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "deconv2x2_wgrad: dtype %d", dtype);
  if (dy->n != x->n || dy->h != 2 * x->h || dy->w != 2 * x->w)
    MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_wgrad: dy is %dx%dx%d, expected %dx%dx%d (kernel 2, stride 2, padding 0)", dy->n, dy->h, dy->w, x->n, 2 * x->h, 2 * x->w);
  if (!dc_vec_view(x, dtype) || !dc_vec_view(dy, dtype))
    MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_wgrad: NHWC views with channels and strides %% 4 == 0 and bases aligned to 4 elements");
  DcDwArgs a;
  memset(&a, 0, sizeof(a));
  a.M = (long)x->n * x->h * x->w;
  if (a.M >= 0x7fffffffL / DW_MAX_SPLITS) MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2_wgrad: too many pixels");
  a.x = x->p; a.xsn = x->sn; a.xsh = x->sh; a.xsw = x->sw;
  a.dy = dy->p; a.dsn = dy->sn; a.dsh = dy->sh; a.dsw = dy->sw;
  a.partial = (float*)ws;
  a.H = x->h; a.W = x->w; a.Cin = x->c; a.Cout = dy->c;
  a.CoutP = (a.Cout + 15) / 16 * 16;
  a.NCOL = 4 * a.CoutP;
  a.ncolg = cdiv(a.NCOL, DW_NT);
  a.nsplit = mgdt_deconv2x2_wgrad_splits(a.Cin, a.Cout);
  dim3 grid(a.nsplit, cdiv(a.Cin, DW_CT) * a.ncolg);
  MGDT_DISPATCH_DTYPE(dtype, (deconv2x2_wgrad_kernel<T><<<grid, 256, 0, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("deconv2x2_wgrad");
  if (dw) {                                            // dw == NULL: partial sums only, added up later by mgdt_wgrad_final_batch with the others'
    mgdt_wgrad_final_desc d;
    d.partial = (const float*)ws; d.dw = dw; d.n = (long)a.Cin * a.Cout * 4; d.nsplit = a.nsplit; d.accumulate = accumulate;
    return mgdt_wgrad_final_batch(&d, 1, s);
  }
  return MGDT_OK;
}
