// SimFusion_3in / LAF (reference nn/modules/block.py:309-329) with cv2 = cv3 = Identity, eval, bf16, in ONE launch:
//   out = act2(cv_fuse([act1(cv1(p0)) | x1 | bilinear(x2)]))        p0 = the avg-pooled first input, x1 the second, x2 the third
// The separate form runs cv1 into concat slot 0, the bilinear into slot 2 and cv_fuse over the 3 * oc channel buffer: two oc-channel maps written to
// HBM and read straight back.  Every output pixel needs its own pixel of p0 and x1 and four taps of x2, so here both maps stay on the chip.
//
// Bit for bit the separate launches: stage 1 is conv_igemm_kernel's chain for cv1 (bias-initialised accumulators, mma(weights, pixels, acc), K chunks
// ascending, activation, rounding to bf16); its values go through a per-wave LDS tile [pixel][channel] and come back as B fragments in natural channel
// order; stage 2 runs cv_fuse's K chunks in concat order [cv1 output | x1 | bilinear(x2)]; the interpolation is resample.h's, rounded to bf16 as the
// stored map is.
//
// A wave owns 16 consecutive output pixels (the MFMA N dimension) per step and all output channels; waves share nothing but the two weight panels,
// staged in LDS once per persistent workgroup, so the loop has no workgroup barrier.  Everything a step reads from memory - one chunk of p0 per 32
// input channels, oc / 32 chunks of x1 and 4 taps x oc / 32 chunks of x2 - is requested one step ahead and lands under the current step's MFMAs
// (p0 / x1 at the top of the step, the taps as soon as the current ones are interpolated: they reuse those registers).
#include <algorithm>

#include "conv_igemm_kernel.h"
#include "resample.h"

struct LafArgs {   // strides in BYTES, extents < 2 GiB (bind_view): the kernel addresses through buffer descriptors
  const char* p0; int p0sn, p0sh, p0sw; uint32_t p0_bytes;
  const char* x1; int x1sn, x1sh, x1sw; uint32_t x1_bytes;
  const char* x2; int x2sn, x2sh, x2sw; uint32_t x2_bytes;
  const char* y; int ysn, ysh, ysw; uint32_t y_bytes;
  const char* w1; const float* b1; const char* w2; const float* b2;
  int H, W, H2, W2, C0, M, HW, numTiles, T8, act1, act2;
  FastDiv fd_hw, fd_w;
  float ry, rx;                                            // (float)H2 / (float)H, (float)W2 / (float)W: the ratio lerp_of divides out, once on the host
};

constexpr int LAF_WAVES = 4, LAF_THREADS = 64 * LAF_WAVES, LAF_CPAD = 8;   // channel padding of a tile pixel (bank spread)
constexpr int LAF_MAX_WGS = 1024;                                         // persistent grid: at most four workgroups on each of the 256 compute units

typedef __attribute__((ext_vector_type(2))) float laf_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 laf_bf16x2;
typedef __attribute__((ext_vector_type(4))) unsigned int laf_u32x4;
__device__ __forceinline__ uint32_t laf_pk_bf16(float lo, float hi) {      // two floats -> two bf16, round to nearest even
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(laf_f32x2{lo, hi}, laf_bf16x2));
}
__device__ __forceinline__ float laf_act(float v, int act) {               // the epilogue forms of conv_igemm_kernel
  return act == MGDT_ACT_RELU ? fmaxf(v, 0.f) : act == MGDT_ACT_SILU ? v * fast_sigmoid(v) : v;
}

// the interpolation weights of the lane's pixel (resample.h's Lerp without the tap indices)
struct LafWeights { float ly0, ly1, lx0, lx1; };

// KC1 = K chunks of cv1 (c0 <= 32 * KC1), NB = oc / 16 cout blocks of both convolutions (cv_fuse: 3 * oc -> oc)
template <int KC1, int NB>
__global__ __launch_bounds__(LAF_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void laf_fuse_kernel(const LafArgs a) {
  typedef bf16x8 frag;
  constexpr int KCM = NB / 2;                               // K chunks of one concat slot
  constexpr int RS = (NB * 16 + LAF_CPAD) * 2;              // bytes per tile pixel
  constexpr int W1V = KC1 * NB * 64, W2V = 3 * KCM * NB * 64;   // 16-byte vectors of the two panels
  __shared__ __attribute__((aligned(16))) char w1l[W1V * 16];          // [KC1][NB][64 lanes][16 B]
  __shared__ __attribute__((aligned(16))) char w2l[W2V * 16];          // [3 * KCM][NB][64][16 B]
  __shared__ __attribute__((aligned(16))) float bl[2][NB * 16];
  __shared__ __attribute__((aligned(16))) char tiles[LAF_WAVES][16 * RS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;

  const __amdgpu_buffer_rsrc_t p0rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.p0, 0, a.p0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x1rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x1, 0, a.x1_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t x2rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x2, 0, a.x2_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.y_bytes, 0x00020000);

  // v = position in the launch-wide round-robin; workgroups land on XCD (id % 8), so XCD k is given the contiguous tile range [k*T8, (k+1)*T8):
  // the x2 rows that neighbouring output rows share are then served by that XCD's own L2 (conv_igemm_kernel's arrangement).
  auto pixel = [&](int v, int& n, int& oy, int& ox) __attribute__((always_inline)) {
    const int tile = (v & 7) * a.T8 + (v >> 3);
    const bool tv = (v >> 3) < a.T8 && tile < a.numTiles;
    const int m = (tile * LAF_WAVES + wave) * 16 + r;
    const bool pv = tv && m < a.M;                          // pixels past the end: every address out of range (loads give 0, stores are dropped)
    const uint32_t mm = pv ? (uint32_t)m : 0u;
    n = (int)fdiv(mm, a.fd_hw);
    const int rem = (int)mm - n * a.HW;
    oy = (int)fdiv((uint32_t)rem, a.fd_w); ox = rem - oy * a.W;
    return pv;
  };
  // the lane's own pixel of p0 and x1, and where its output goes
  auto request_px = [&](int v, frag(&P)[KC1], frag(&X)[KCM], int& yo) __attribute__((always_inline)) {
    int n, oy, ox;
    const bool pv = pixel(v, n, oy, ox);
    const int po = pv ? n * a.p0sn + oy * a.p0sh + ox * a.p0sw : MGDT_OOB;
    const int xo = pv ? n * a.x1sn + oy * a.x1sh + ox * a.x1sw : MGDT_OOB;
    yo = pv ? n * a.ysn + oy * a.ysh + ox * a.ysw : MGDT_OOB;
#pragma unroll
    for (int kc = 0; kc < KC1; ++kc) {
      const int cb = (kc * 4 + g) * 16;
      P[kc] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(p0rs, (cb < a.C0 * 2) ? (uint32_t)(po + cb) : (uint32_t)MGDT_OOB, 0, 0));
    }
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc)
      X[kc] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(x1rs, (uint32_t)(xo + (kc * 4 + g) * 16), 0, 0));
  };
  // its four taps of x2 and their weights
  auto request_taps = [&](int v, frag(&T)[4][KCM], LafWeights& q) __attribute__((always_inline)) {
    int n, oy, ox;
    const bool pv = pixel(v, n, oy, ox);
    const Lerp ly = lerp_of_r(oy, a.ry, a.H2), lx = lerp_of_r(ox, a.rx, a.W2);
    q.ly0 = ly.l0; q.ly1 = ly.l1; q.lx0 = lx.l0; q.lx1 = lx.l1;
    const int base = n * a.x2sn, r0 = ly.i0 * a.x2sh, r1 = ly.i1 * a.x2sh, c0 = lx.i0 * a.x2sw, c1 = lx.i1 * a.x2sw;
    const int to[4] = {base + r0 + c0, base + r0 + c1, base + r1 + c0, base + r1 + c1};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int kc = 0; kc < KCM; ++kc)
        T[t][kc] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(x2rs, pv ? (uint32_t)(to[t] + (kc * 4 + g) * 16) : (uint32_t)MGDT_OOB, 0, 0));
  };

  // p0 / x1 are double-buffered; the taps (the bulk of the registers) are not: a step turns them into its bilinear B fragments first and requests
  // the next step's taps into the same registers, so those too are in flight under this step's MFMAs
  frag P[KC1], X[KCM], Pn[KC1], Xn[KCM], T[4][KCM];
  LafWeights q;
  int yo, yon;
  request_px((int)blockIdx.x, P, X, yo);                    // the first step's reads fly while the panels are staged
  request_taps((int)blockIdx.x, T, q);
  {
    // both weight panels: every 16-byte request is issued before the first LDS store
    constexpr int N1 = (W1V + LAF_THREADS - 1) / LAF_THREADS, N2 = (W2V + LAF_THREADS - 1) / LAF_THREADS;
    uint4 t1[N1], t2[N2];
#pragma unroll
    for (int u = 0; u < N1; ++u) t1[u] = ((const uint4*)a.w1)[min(tid + u * LAF_THREADS, W1V - 1)];
#pragma unroll
    for (int u = 0; u < N2; ++u) t2[u] = ((const uint4*)a.w2)[min(tid + u * LAF_THREADS, W2V - 1)];
#pragma unroll
    for (int u = 0; u < N1; ++u) if (tid + u * LAF_THREADS < W1V) ((uint4*)w1l)[tid + u * LAF_THREADS] = t1[u];
#pragma unroll
    for (int u = 0; u < N2; ++u) if (tid + u * LAF_THREADS < W2V) ((uint4*)w2l)[tid + u * LAF_THREADS] = t2[u];
    if (tid < NB * 16) { bl[0][tid] = a.b1[tid]; bl[1][tid] = a.b2[tid]; }
  }
  __syncthreads();
  const char* const w1lane = w1l + lane * 16;
  const char* const w2lane = w2l + lane * 16;
  char* const tile = tiles[wave];
  char* const twr = tile + r * RS + 8 * g;                  // the accumulator layout's slot: channels nb*16 + 4g .. +3 of pixel r
  const char* const trd = tile + r * RS + 16 * g;           // the B fragment's slot: channels kc*32 + 8g .. +7 of pixel r
  // the store leaves through the tile as well: 16 bytes per lane, the NB * 2 lanes of a pixel cover its whole line
  constexpr int LPP = NB * 2, PPP = 64 / LPP;               // lanes per pixel, pixels per pass (KCM passes)
  const int spx = lane / LPP, spc = (lane % LPP) * 16;

#pragma unroll 1
  for (int v = blockIdx.x; v < 8 * a.T8; v += gridDim.x) {
    request_px(v + (int)gridDim.x, Pn, Xn, yon);            // the next step's reads fly under this step's MFMAs
    // ---- bilinear(x2) of my 16 pixels as stage 2's last B fragments, rounded to bf16 as the stored map is ----
    frag BW[KCM];
    {
      const Lerp ly = {0, 0, q.ly0, q.ly1}, lx = {0, 0, q.lx0, q.lx1};
#pragma unroll
      for (int kc = 0; kc < KCM; ++kc) {
        const laf_u32x4 t00 = __builtin_bit_cast(laf_u32x4, T[0][kc]), t01 = __builtin_bit_cast(laf_u32x4, T[1][kc]);
        const laf_u32x4 t10 = __builtin_bit_cast(laf_u32x4, T[2][kc]), t11 = __builtin_bit_cast(laf_u32x4, T[3][kc]);
        laf_u32x4 bw;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = bilerp_mix_fma(__uint_as_float(t00[j] << 16), __uint_as_float(t01[j] << 16), __uint_as_float(t10[j] << 16), __uint_as_float(t11[j] << 16), ly, lx);
          const float hi = bilerp_mix_fma(__uint_as_float(t00[j] & 0xffff0000u), __uint_as_float(t01[j] & 0xffff0000u), __uint_as_float(t10[j] & 0xffff0000u),
                                      __uint_as_float(t11[j] & 0xffff0000u), ly, lx);
          bw[j] = laf_pk_bf16(lo, hi);
        }
        BW[kc] = __builtin_bit_cast(frag, bw);
      }
    }
    request_taps(v + (int)gridDim.x, T, q);

    // ---- stage 1: cv1 on my 16 pixels, into the tile as bf16 ----
    {
      f32x4 acc[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = *(const f32x4*)(&bl[0][nb * 16 + 4 * g]);
#pragma unroll
      for (int kc = 0; kc < KC1; ++kc)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = mma(*(const frag*)(w1lane + (kc * NB + nb) * 1024), P[kc], acc[nb]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const f32x4 c = acc[nb];
        *(uint2*)(twr + nb * 32) = make_uint2(laf_pk_bf16(laf_act(c[0], a.act1), laf_act(c[1], a.act1)), laf_pk_bf16(laf_act(c[2], a.act1), laf_act(c[3], a.act1)));
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- stage 2: cv_fuse over [cv1 output | x1 | bilinear(x2)], K chunks ascending ----
    f32x4 acc2[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc2[nb] = *(const f32x4*)(&bl[1][nb * 16 + 4 * g]);
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc) {
      const frag B = *(const frag*)(trd + kc * 64);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc2[nb] = mma(*(const frag*)(w2lane + (kc * NB + nb) * 1024), B, acc2[nb]);
    }
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc2[nb] = mma(*(const frag*)(w2lane + ((KCM + kc) * NB + nb) * 1024), X[kc], acc2[nb]);
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc2[nb] = mma(*(const frag*)(w2lane + ((2 * KCM + kc) * NB + nb) * 1024), BW[kc], acc2[nb]);

    // ---- epilogue: activation, rounding, whole lines out through the tile ----
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                         // every lane has read its stage-1 fragments
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const f32x4 c = acc2[nb];
      *(uint2*)(twr + nb * 32) = make_uint2(laf_pk_bf16(laf_act(c[0], a.act2), laf_act(c[1], a.act2)), laf_pk_bf16(laf_act(c[2], a.act2), laf_act(c[3], a.act2)));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int ps = 0; ps < KCM; ++ps) {
      const int px = ps * PPP + spx;                         // lanes 0..15 hold pixels 0..15 (g = 0)
      const int yp = __shfl(yo, px);
      const laf_u32x4 o = *(const laf_u32x4*)(tile + px * RS + spc);
      __builtin_amdgcn_raw_buffer_store_b128(o, yrs, (uint32_t)yp + (uint32_t)spc, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                         // the tile is free for the next step's stage 1

#pragma unroll
    for (int kc = 0; kc < KC1; ++kc) P[kc] = Pn[kc];
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc) X[kc] = Xn[kc];
    yo = yon;
  }
}

static bool laf_act_ok(int act) { return act == MGDT_ACT_NONE || act == MGDT_ACT_SILU || act == MGDT_ACT_RELU; }

/* 1 when mgdt_laf_fuse_fwd covers the shapes: bf16, c0 % 8 == 0 and <= 64, oc in {32, 64}, cv_fuse 3 * oc -> oc2 == oc, activations none / SiLU / ReLU */
extern "C" int mgdt_laf_fuse_supported(int c0, int oc, int oc2, int h, int w, int h2, int w2, int act1, int act2, int dtype) {
  if (dtype != MGDT_BF16 || c0 < 8 || c0 % 8 || c0 > 64 || (oc != 32 && oc != 64) || oc2 != oc) return 0;
  if (h < 1 || w < 1 || h2 < 1 || w2 < 1 || !laf_act_ok(act1) || !laf_act_ok(act2)) return 0;
  return 1;
}

template <int KC1, int NB>
static int laf_launch(const LafArgs& a, hipStream_t st) {
  // persistent grid = what is resident at once (registers decide: 4 workgroups per CU at c0 <= 32, 3 above), in whole rounds of the 8 XCDs
  static std::atomic<int> resident{0};
  int cap = resident;
  if (!cap) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t pr;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, laf_fuse_kernel<KC1, NB>, LAF_THREADS, 0) != hipSuccess || per_cu < 1 ||
        hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess || pr.multiProcessorCount < 8)
      MGDT_FAIL(MGDT_LAUNCH_FAIL, "laf_fuse: occupancy query failed");
    resident = cap = std::min(per_cu * pr.multiProcessorCount / 8 * 8, LAF_MAX_WGS);
  }
  laf_fuse_kernel<KC1, NB><<<std::min(8 * a.T8, cap), LAF_THREADS, 0, st>>>(a);
  MGDT_CHECK_LAUNCH("laf_fuse_fwd");
  return MGDT_OK;
}

extern "C" int mgdt_laf_fuse_fwd(const mgdt_view* p0, const mgdt_view* x1, const mgdt_view* x2, const void* packed_w1, const float* bias1, int act1,
                                 const void* packed_w2, const float* bias2, int act2, const mgdt_view* y, int dtype, mgdt_stream s) {
  if (!view_ok(p0) || !view_ok(x1) || !view_ok(x2) || !view_ok(y) || !packed_w1 || !bias1 || !packed_w2 || !bias2)
    MGDT_FAIL(MGDT_BAD_ARG, "laf_fuse: null/empty argument");
  if (!mgdt_laf_fuse_supported(p0->c, x1->c, y->c, y->h, y->w, x2->h, x2->w, act1, act2, dtype))
    MGDT_FAIL(MGDT_BAD_SHAPE, "laf_fuse: shapes/dtype/activations not covered (see mgdt_laf_fuse_supported)");
  if (p0->n != y->n || x1->n != y->n || x2->n != y->n || p0->h != y->h || p0->w != y->w || x1->h != y->h || x1->w != y->w || x2->c != x1->c)
    MGDT_FAIL(MGDT_BAD_SHAPE, "laf_fuse: p0 / x1 / y must share n, h, w; x2 shares n and x1's channels");
  const long M = (long)y->n * y->h * y->w;
  if (M >= 0x7fffffffL - 64 * LAF_MAX_WGS) MGDT_FAIL(MGDT_BAD_SHAPE, "laf_fuse: too many pixels");
  LafArgs a;
  memset(&a, 0, sizeof(a));
  const int sz = 2;
  const ViewPolicy v16 = {8, true, 0, 0, false};            // 16-byte pieces of a pixel's channels
  if (!bind_view(p0, sz, v16, &a.p0, &a.p0sn, &a.p0sh, &a.p0sw, &a.p0_bytes) || !bind_view(x1, sz, v16, &a.x1, &a.x1sn, &a.x1sh, &a.x1sw, &a.x1_bytes) ||
      !bind_view(x2, sz, v16, &a.x2, &a.x2sn, &a.x2sh, &a.x2sw, &a.x2_bytes) || !bind_view(y, sz, v16, &a.y, &a.ysn, &a.ysh, &a.ysw, &a.y_bytes))
    MGDT_FAIL(MGDT_BAD_SHAPE, "laf_fuse: views must be NHWC (sc == 1), 16-byte aligned and < 2 GiB");
  a.w1 = (const char*)packed_w1; a.b1 = bias1; a.w2 = (const char*)packed_w2; a.b2 = bias2; a.act1 = act1; a.act2 = act2;
  a.H = y->h; a.W = y->w; a.H2 = x2->h; a.W2 = x2->w; a.C0 = p0->c; a.M = (int)M; a.HW = y->h * y->w;
  a.numTiles = cdiv(M, 16 * LAF_WAVES); a.T8 = cdiv(a.numTiles, 8);
  a.fd_hw = make_fastdiv((uint32_t)a.HW); a.fd_w = make_fastdiv((uint32_t)a.W);
  a.ry = (float)a.H2 / (float)a.H; a.rx = (float)a.W2 / (float)a.W;
  const int kc1 = cdiv(a.C0, 32), nb = x1->c / 16;
  hipStream_t st = (hipStream_t)s;
#define LAF_CASE(K, B) if (kc1 == K && nb == B) return laf_launch<K, B>(a, st);
  LAF_CASE(1, 2) LAF_CASE(2, 2) LAF_CASE(1, 4) LAF_CASE(2, 4)
#undef LAF_CASE
  MGDT_FAIL(MGDT_BAD_SHAPE, "laf_fuse: no kernel for kc1=%d nb=%d", kc1, nb);
}
