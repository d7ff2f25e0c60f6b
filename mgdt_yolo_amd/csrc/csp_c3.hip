// Mode 2 (CSP_C3) of the csp_block family: one launch per C3 block (reference nn/modules/block.py:434-447) of the bf16 inference path, behind the same
// entry points (mgdt_csp_block_supported / _tiles / _fwd in csp_block.hip dispatch here for mode == 2; the kernels of modes 0 / 1 are untouched).
//
//   front   x = [a | b] = [cv1 | cv2](input) comes from ONE ordinary 1x1 launch over the concatenated weights; the front copies a (tile + halo) and
//           b (tile) into LDS
//   middle  n bottlenecks on a: T = silu(1x1(P)), P' = silu(3x3(T)) (+ P).  The 1x1 needs no neighbours, so it runs over the region the following 3x3
//           reads; the halo is n pixels (one ring per bottleneck), recomputed per tile
//   back    y = silu(cv3([P_n | b])), K = 2 wd, written to HBM.  No pooled sums.
//
// A workgroup (4 waves) owns a TH x TW tile of one image.  LDS: three NHWC maps over the (TH + 2n) x (TW + 2n) region (P, T, P'; pixel stride wd * 2 bytes,
// unswizzled) and b over the tile.  GEMM orientation and panels as conv_igemm / csp_block: weights = A operand (ordinary mgdt_conv_pack panels read from
// L2), 16 pixels = B operand (one 16-byte LDS read per lane and K chunk), a lane ends with 4 consecutive channels of one pixel.  Every map is bf16 where
// it is stored (the rounding points of ref_csp_block); pixels outside the image are zeros in P and T (the convolutions' zero padding).  A ring of the
// region that a step cannot compute holds values nobody consumes: after bottleneck j the map is valid at distance >= j + 1 from the region's border.
// Plain and untuned next to modes 0 / 1 (no swizzle, weights re-read per pixel group): whether a shape takes it is decided by measurement.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "conv_igemm_kernel.h"

struct C3Args {
  const char* x; long xsn, xsh, xsw;
  char* y; long ysn, ysh, ysw;
  const char* mid[4]; const float* mid_bias[4];
  const char* back; const float* back_bias;
  int N, H, W, Cout, nbtl, shortcut;
  int TH, TW, RH, RW, RPA, TPA, tiles_x, tiles_y, nbo;
};

constexpr int C3_THREADS = 256;
constexpr int C3_NW = C3_THREADS / 64;

__device__ __forceinline__ void c3_store4(char* p, f32x4 v) {
  bf16x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (bf16)v[i];
  *(bf16x4*)p = o;
}

template <int WD>
__global__ __launch_bounds__(C3_THREADS) void csp_c3_kernel(const C3Args a) {
  constexpr int CP = WD / 8;                       // 16-byte pieces of a wd-channel pixel
  constexpr int NB = WD / 16;                      // cout blocks of a wd -> wd conv
  constexpr int NCH1 = (CP + 3) / 4;               // K chunks: 1x1 wd -> wd
  constexpr int NCH3 = (9 * CP + 3) / 4;           //           3x3 wd -> wd
  constexpr int NCHB = (2 * CP + 3) / 4;           //           1x1 over [P_n | b]
  constexpr int PS = 2 * WD;                       // pixel stride (bytes)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* M0 = smem;
  char* Tb = M0 + (size_t)a.RPA * PS;
  char* M1 = Tb + (size_t)a.RPA * PS;
  char* Bt = M1 + (size_t)a.RPA * PS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int tpi = a.tiles_x * a.tiles_y;
  const int n = blockIdx.x / tpi, trem = blockIdx.x - n * tpi;
  const int tyi = trem / a.tiles_x;
  const int ty0 = tyi * a.TH, tx0 = (trem - tyi * a.tiles_x) * a.TW;
  const int halo = a.nbtl, RP = a.RH * a.RW, TP = a.TH * a.TW;
  const bf16x8 zero8 = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};

  // ---- front: a over the region (zeros outside the image), b over the tile
  for (int i = tid; i < RP * CP; i += C3_THREADS) {
    const int q = i / CP, cp = i - q * CP;
    const int ry = q / a.RW, rx = q - ry * a.RW;
    const int iy = ty0 - halo + ry, ix = tx0 - halo + rx;
    const bool in = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
    const char* src = a.x + n * a.xsn + iy * a.xsh + ix * a.xsw + cp * 16;
    bf16x8 va = zero8;
    if (in) va = *(const bf16x8*)src;
    *(bf16x8*)(M0 + (size_t)q * PS + cp * 16) = va;
    const int cy = ry - halo, cx = rx - halo;
    if ((unsigned)cy < (unsigned)a.TH && (unsigned)cx < (unsigned)a.TW) *(bf16x8*)(Bt + (size_t)(cy * a.TW + cx) * PS + cp * 16) = *(const bf16x8*)(src + PS);
  }
  __syncthreads();

  const int ngr = (RP + 15) >> 4;
  char* src = M0;
  char* dst = M1;
  for (int j = 0; j < a.nbtl; ++j) {
    // ---- 1x1 over every region pixel: T = silu(cv1(src)), zero outside the image
    for (int gi = wave; gi < ngr; gi += C3_NW) {
      const int q = gi * 16 + r;
      const bool live = q < RP;
      const int ry = q / a.RW, rx = q - ry * a.RW;
      const int iy = ty0 - halo + ry, ix = tx0 - halo + rx;
      const bool in = live && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      bf16x8 Bf[NCH1];
#pragma unroll
      for (int kc = 0; kc < NCH1; ++kc) {
        const int p = kc * 4 + g;
        Bf[kc] = (live && p < CP) ? *(const bf16x8*)(src + (size_t)q * PS + p * 16) : zero8;
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        f32x4 acc = *(const f32x4*)(a.mid_bias[2 * j] + nb * 16 + 4 * g);
#pragma unroll
        for (int kc = 0; kc < NCH1; ++kc) acc = mma(*(const bf16x8*)(a.mid[2 * j] + ((size_t)(kc * NB + nb) * 64 + lane) * 16), Bf[kc], acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = in ? acc[e] * fast_sigmoid(acc[e]) : 0.f;
        if (live) c3_store4(Tb + (size_t)q * PS + (nb * 16 + 4 * g) * 2, acc);
      }
    }
    __syncthreads();
    // ---- 3x3 over the region's interior: dst = silu(cv2(T)) (+ src)
    for (int gi = wave; gi < ngr; gi += C3_NW) {
      const int q = gi * 16 + r;
      const int ry = q / a.RW, rx = q - ry * a.RW;
      const bool live = q < RP && ry >= 1 && ry < a.RH - 1 && rx >= 1 && rx < a.RW - 1;
      f32x4 acc[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = *(const f32x4*)(a.mid_bias[2 * j + 1] + nb * 16 + 4 * g);
#pragma unroll
      for (int kc = 0; kc < NCH3; ++kc) {
        const int p = kc * 4 + g;
        const int tap = p / CP, cp = p - tap * CP;
        bf16x8 Bf = zero8;
        if (live && tap < 9) Bf = *(const bf16x8*)(Tb + (size_t)(q + (tap / 3 - 1) * a.RW + (tap % 3 - 1)) * PS + cp * 16);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = mma(*(const bf16x8*)(a.mid[2 * j + 1] + ((size_t)(kc * NB + nb) * 64 + lane) * 16), Bf, acc[nb]);
      }
      if (live) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int c = nb * 16 + 4 * g;
          f32x4 v = acc[nb];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] * fast_sigmoid(v[e]);
          if (a.shortcut) {
            const bf16x4 s = *(const bf16x4*)(src + (size_t)q * PS + c * 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)s[e];
          }
          c3_store4(dst + (size_t)q * PS + c * 2, v);
        }
      }
    }
    __syncthreads();
    char* t = src; src = dst; dst = t;
  }

  // ---- back: y = silu(cv3([src | b])) over the tile's pixels
  const int ngt = (TP + 15) >> 4;
  for (int gi = wave; gi < ngt; gi += C3_NW) {
    const int t = gi * 16 + r;
    const bool live = t < TP;
    const int cy = t / a.TW, cx = t - cy * a.TW;
    const int q = (cy + halo) * a.RW + cx + halo;
    bf16x8 Bf[NCHB];
#pragma unroll
    for (int kc = 0; kc < NCHB; ++kc) {
      const int p = kc * 4 + g;
      bf16x8 v = zero8;
      if (live && p < CP) v = *(const bf16x8*)(src + (size_t)q * PS + p * 16);
      else if (live && p < 2 * CP) v = *(const bf16x8*)(Bt + (size_t)t * PS + (p - CP) * 16);
      Bf[kc] = v;
    }
    char* yp = a.y + n * a.ysn + (ty0 + cy) * a.ysh + (tx0 + cx) * a.ysw;
    for (int nb = 0; nb < a.nbo; ++nb) {
      f32x4 acc = *(const f32x4*)(a.back_bias + nb * 16 + 4 * g);
#pragma unroll
      for (int kc = 0; kc < NCHB; ++kc) acc = mma(*(const bf16x8*)(a.back + ((size_t)(kc * a.nbo + nb) * 64 + lane) * 16), Bf[kc], acc);
      const int c = nb * 16 + 4 * g;
      if (live && c < a.Cout) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] * fast_sigmoid(acc[e]);
        c3_store4(yp + c * 2, acc);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct C3Geom { int TH, TW, RH, RW, RPA, TPA, tiles_x, tiles_y; size_t lds; };
constexpr size_t C3_LDS_MAX = 80 * 1024;          // two workgroups per CU (160 KB)

int csp_c3_supported(int cin, int cout, int wd, int nbtl, int h, int w, int dtype) {
  if (dtype != MGDT_BF16 || (wd != 16 && wd != 32 && wd != 64) || nbtl < 1 || nbtl > 2) return 0;
  if (cin != 2 * wd || cout < 4 || cout % 4 || cout > 512 || h < 2 || w < 2) return 0;
  return 1;
}

static bool c3_pick_tile(int H, int W, int N, int wd, int nbtl, C3Geom* best) {
  int fth = 0, ftw = 0;
  knob_pair("MGDT_CSP_TILE", &fth, &ftw);       // experiment knob "th,tw" shared with modes 0 / 1, read per call (not part of the ABI)
  double best_cost = 1e30;
  bool found = false;
  for (int th = 2; th <= std::min(H, 32); ++th) {
    if (H % th) continue;
    for (int tw = 2; tw <= std::min(W, 32); ++tw) {
      if (W % tw) continue;
      if (fth && (th != fth || tw != ftw)) continue;
      C3Geom g;
      g.TH = th; g.TW = tw; g.RH = th + 2 * nbtl; g.RW = tw + 2 * nbtl;
      g.RPA = ((g.RH * g.RW + 15) / 16) * 16;
      g.TPA = ((th * tw + 15) / 16) * 16;
      g.tiles_x = W / tw; g.tiles_y = H / th;
      g.lds = (size_t)(3 * g.RPA + g.TPA) * wd * 2;
      if (g.lds > C3_LDS_MAX) continue;
      const double wgs = (double)N * g.tiles_x * g.tiles_y;
      double cost = (double)g.RPA / (th * tw);                 // recomputed halo and idle lanes of the last pixel group
      if (wgs < 512) cost *= 512.0 / wgs;                      // fewer workgroups than two per CU: the chip is not filled
      if (cost < best_cost) { best_cost = cost; *best = g; found = true; }
    }
  }
  return found;
}

int csp_c3_tiles(int n, int cin, int cout, int wd, int nbtl, int h, int w, int* geom8) {
  if (!csp_c3_supported(cin, cout, wd, nbtl, h, w, MGDT_BF16)) return 0;
  C3Geom g;
  if (!c3_pick_tile(h, w, n, wd, nbtl, &g)) return 0;
  if (geom8) {
    geom8[0] = g.TH; geom8[1] = g.TW; geom8[2] = g.RH; geom8[3] = g.RW; geom8[4] = (int)g.lds; geom8[5] = n * g.tiles_x * g.tiles_y;
    geom8[6] = g.tiles_x; geom8[7] = g.tiles_y;
  }
  return g.tiles_x * g.tiles_y;
}

int csp_c3_fwd(const mgdt_view* x, const void* const* mid, const float* const* mid_bias, int nbtl, int shortcut, const void* back, const float* back_bias,
               int wd, const mgdt_view* y, mgdt_stream s) {
  C3Args a;
  memset(&a, 0, sizeof(a));
  // the kernel keeps 64-bit strides; x: 16-byte loads, y: 8-byte stores
  if (!view_fits(x, 2, {8, true, 0, 0, false}) || !view_fits(y, 2, {4, true, 0, 0, false})) MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block (C3): views must be NHWC (sc == 1), x in 16-byte and y in 8-byte aligned pixels, span < 2 GiB");
  C3Geom g;
  if (!c3_pick_tile(x->h, x->w, x->n, wd, nbtl, &g)) MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block (C3): no tile fits %dx%d wd=%d n=%d", x->h, x->w, wd, nbtl);
  a.x = (const char*)x->p; a.xsn = x->sn * 2; a.xsh = x->sh * 2; a.xsw = x->sw * 2;
  a.y = (char*)y->p; a.ysn = y->sn * 2; a.ysh = y->sh * 2; a.ysw = y->sw * 2;
  for (int j = 0; j < 2 * nbtl; ++j) { a.mid[j] = (const char*)mid[j]; a.mid_bias[j] = mid_bias[j]; }
  a.back = (const char*)back; a.back_bias = back_bias;
  a.N = x->n; a.H = x->h; a.W = x->w; a.Cout = y->c; a.nbtl = nbtl; a.shortcut = shortcut;
  a.TH = g.TH; a.TW = g.TW; a.RH = g.RH; a.RW = g.RW; a.RPA = g.RPA; a.TPA = g.TPA; a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y;
  a.nbo = (a.Cout + 15) / 16;
  const long grid = (long)a.N * g.tiles_x * g.tiles_y;
  if (grid > 0x7fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block (C3): too many tiles");
  hipStream_t st = (hipStream_t)s;
#define C3_LAUNCH(WD_)                                                                                                                    \
  do {                                                                                                                                     \
    if (int rc_ = lds_optin<csp_c3_kernel<WD_>>("csp_block (C3)", (int)C3_LDS_MAX)) return rc_;                                            \
    csp_c3_kernel<WD_><<<(int)grid, C3_THREADS, g.lds, st>>>(a);                                                                           \
  } while (0)
  switch (wd) { case 16: C3_LAUNCH(16); break; case 32: C3_LAUNCH(32); break; default: C3_LAUNCH(64); break; }
#undef C3_LAUNCH
  MGDT_CHECK_LAUNCH("csp_block_fwd (C3)");
  return MGDT_OK;
}
