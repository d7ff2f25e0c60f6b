// Test-time augmentation input resampling: the optional left-right flip, the bilinear resize and the right / bottom padding of one augmented
// pass in one launch.  Reference: yolo/utils/torch_utils.py:261-270 (scale_img), nn/tasks.py:256-287 (_predict_augment: x.flip(3) first).
//
// The kernel is HBM-bound (B = 32, 640^2 uint8 -> 544^2 bf16: ~39 MB read, ~57 MB written).  A wave owns a band of SI_BAND output rows of one
// (image, channel) plane; the two source rows an output row interpolates between are staged in LDS as fp32 (read coalesced, converted - and
// divided by 255 - once per source pixel, kept across output rows that share them), the row weights are wave-uniform, and the lanes write
// 16-byte runs of V consecutive pixels along W.  Index / weight arithmetic is PyTorch's CPU upsample_bilinear2d with align_corners=False
// and the output size given: scale = (float)in / out, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = (int)src (clamped), the +1 neighbour
// clamped at the edge, lambda = src - i0; out = (x00 w0 + x01 w1) h0 + (x10 w0 + x11 w1) h1.
#include "common.h"

template <typename TX> __device__ __forceinline__ float img_ld(const TX* p);
template <> __device__ __forceinline__ float img_ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float img_ld<bf16>(const bf16* p) { return (float)*p; }
template <> __device__ __forceinline__ float img_ld<uint8_t>(const uint8_t* p) { return __fdiv_rn((float)*p, 255.f); }     // `img /= 255`, exact

struct SiArgs {
  const void* x; long xsn, xsc, xsh, xsw;     // N x 3 x H x W image, element strides
  void* y; long ysn, ysc, ysh, ysw;           // N x 3 x Hp x Wp output, element strides
  int N, H, W, Hs, Ws, Hp, Wp, flip, rows;   // rows: wave units = planes x bands of output rows
  float sy, sx, pad;
};

constexpr int SI_BAND = 4;         // output rows per wave unit (more units = more waves in flight: the row fetches are latency-bound)
constexpr int SI_MAX_W = 2048;     // 4 waves x 2 source rows x W fp32 of LDS <= 64 KiB

template <typename TX, typename TY>
__global__ __launch_bounds__(256) void scale_img_kernel(const SiArgs a) {
  extern __shared__ float srows[];                           // [4 waves][2][W]
  constexpr int V = 16 / sizeof(TY);                         // pixels per lane: one 16-byte store
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool vec = a.ysw == 1 && (a.Wp % V) == 0 && (a.ysh % V) == 0 && (a.ysc % V) == 0 && (a.ysn % V) == 0 && ((uintptr_t)a.y & 15) == 0;
  auto wave_sync = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const int bands = (a.Hp + SI_BAND - 1) / SI_BAND;
  for (int unit = blockIdx.x * 4 + wave; unit < a.rows; unit += gridDim.x * 4) {   // a.rows = planes x bands
    const int nc = unit / bands, oy0 = (unit - nc * bands) * SI_BAND;
    const int n = nc / 3, c = nc - n * 3;
    const TX* plane = (const TX*)a.x + n * a.xsn + c * a.xsc;
    float* s0 = srows + (size_t)wave * 2 * a.W;
    float* s1 = s0 + a.W;
    int k0 = -1, k1 = -1;                                    // source rows held in s0 / s1
    auto fetch = [&](float* dst, int yy) __attribute__((always_inline)) {
      wave_sync();                                           // every lane is done reading the row this one replaces
      const TX* r = plane + yy * a.xsh;
#pragma unroll 4
      for (int i = lane; i < a.W; i += 64) dst[i] = img_ld<TX>(r + (long)(a.flip ? a.W - 1 - i : i) * a.xsw);   // stored flipped
    };
    for (int oy = oy0; oy < min(oy0 + SI_BAND, a.Hp); ++oy) {
      TY* yr = (TY*)a.y + n * a.ysn + c * a.ysc + oy * a.ysh;
      const bool in_row = oy < a.Hs;
      float h0 = 0.f, h1 = 0.f;
      if (in_row) {
        const float sy = fmaxf(a.sy * ((float)oy + 0.5f) - 0.5f, 0.f);
        const int y0 = min((int)sy, a.H - 1), y1 = y0 + (y0 < a.H - 1 ? 1 : 0);
        h1 = fminf(fmaxf(sy - (float)y0, 0.f), 1.f); h0 = 1.f - h1;
        if (k0 != y0) {
          if (k1 == y0) { float* t = s0; s0 = s1; s1 = t; k1 = k0; k0 = y0; }
          else { fetch(s0, y0); k0 = y0; }
        }
        if (k1 != y1) { fetch(s1, y1); k1 = y1; }
        wave_sync();                                         // the staged rows are visible to every lane
      }
      for (int ox0 = lane * V; ox0 < a.Wp; ox0 += 64 * V) {
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int ox = ox0 + k;
          if (!in_row || ox >= a.Ws) { o[k] = a.pad; continue; }
          const float sx = fmaxf(a.sx * ((float)ox + 0.5f) - 0.5f, 0.f);
          const int x0 = min((int)sx, a.W - 1), x1 = x0 + (x0 < a.W - 1 ? 1 : 0);
          const float w1 = fminf(fmaxf(sx - (float)x0, 0.f), 1.f), w0 = 1.f - w1;
          const float t0 = s0[x0] * w0 + s0[x1] * w1;
          const float t1 = s1[x0] * w0 + s1[x1] * w1;
          o[k] = t0 * h0 + t1 * h1;
        }
        if (vec) {
          if constexpr (sizeof(TY) == 4) {
            *(f32x4*)(yr + ox0) = f32x4{o[0], o[1], o[2], o[3]};
          } else {
            bf16x8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (bf16)o[k];        // round to nearest even
            *(bf16x8*)(yr + ox0) = v;
          }
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (ox0 + k < a.Wp) yr[(long)(ox0 + k) * a.ysw] = (TY)o[k];
        }
      }
    }
  }
}

extern "C" int mgdt_scale_img_fwd(const mgdt_view* x, int x_dtype, int flip, int hs, int ws, float pad, const mgdt_view* y, int y_dtype, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(y)) MGDT_FAIL(MGDT_BAD_ARG, "scale_img: null/empty argument");
  if (x->c != 3 || y->c != 3 || y->n != x->n || hs < 1 || ws < 1 || hs > y->h || ws > y->w)
    MGDT_FAIL(MGDT_BAD_SHAPE, "scale_img: x %dx%dx%dx%d, y %dx%dx%dx%d, resized %dx%d", x->n, x->c, x->h, x->w, y->n, y->c, y->h, y->w, hs, ws);
  if ((long)y->n * 3 * y->h >= 0x7fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "scale_img: too many rows");
  if (x->w > SI_MAX_W) MGDT_FAIL(MGDT_BAD_SHAPE, "scale_img: images wider than %d px are not covered (got %d)", SI_MAX_W, x->w);
  SiArgs a;
  a.x = x->p; a.xsn = x->sn; a.xsc = x->sc; a.xsh = x->sh; a.xsw = x->sw;
  a.y = y->p; a.ysn = y->sn; a.ysc = y->sc; a.ysh = y->sh; a.ysw = y->sw;
  a.N = x->n; a.H = x->h; a.W = x->w; a.Hs = hs; a.Ws = ws; a.Hp = y->h; a.Wp = y->w; a.flip = flip ? 1 : 0;
  a.rows = y->n * 3 * ((y->h + SI_BAND - 1) / SI_BAND);
  a.sy = (float)x->h / (float)hs; a.sx = (float)x->w / (float)ws; a.pad = pad;
  const int grid = std::min(cdiv(a.rows, 4), 4096);
  const size_t lds = (size_t)4 * 2 * x->w * sizeof(float);
#define SI_LAUNCH(TX, TY) scale_img_kernel<TX, TY><<<grid, 256, lds, (hipStream_t)s>>>(a)
  if (y_dtype != MGDT_F32 && y_dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "scale_img: output dtype %d", y_dtype);
  const bool yf = y_dtype == MGDT_F32;
  if (x_dtype == MGDT_F32) { if (yf) SI_LAUNCH(float, float); else SI_LAUNCH(float, bf16); }
  else if (x_dtype == MGDT_BF16) { if (yf) SI_LAUNCH(bf16, float); else SI_LAUNCH(bf16, bf16); }
  else if (x_dtype == MGDT_U8) { if (yf) SI_LAUNCH(uint8_t, float); else SI_LAUNCH(uint8_t, bf16); }
  else MGDT_FAIL(MGDT_BAD_DTYPE, "scale_img: input dtype %d", x_dtype);
#undef SI_LAUNCH
  MGDT_CHECK_LAUNCH("scale_img_fwd");
  return MGDT_OK;
}
