// SPPF / SPP (reference nn/modules/block.py:121-153), eval, bf16, in ONE launch:
//   y = act2(cv2([x0 | y1 | y2 | y3]))      x0 = act1(cv1(x)), y1 / y2 / y3 = the 5x5 / 9x9 / 13x13 stride-1 maxima of x0 (three chained MaxPool2d(5, 1, 2))
// The separate form runs cv1 into concat slot 0, the pools into slots 1..3 and cv2 over the 4 * c_ channel buffer: a 4 * c_ channel map written by two
// launches and read back by a third.  cv2 of a pixel needs that pixel's x0, y1, y2, y3 only, and those need cv1 on its 13x13 neighbourhood, so here
// nothing but x and y touches memory.
//
// Bit for bit the three launches: cv1 and cv2 are conv_igemm_kernel's chain (bias-initialised accumulators, mma(weights, pixels, acc), K chunks
// ascending - cv2's in concat order [x0 | y1 | y2 | y3] -, the activation, rounding to bf16); a maximum is exact, so how the windows are put together
// does not show in the result.
//
// A workgroup (8 waves) owns a tile of up to 10x10 output pixels of one image:
//   1. cv1 on the tile and its 6-pixel halo, clipped to the map, into LDS plane A as [pixel][channel]; cv1's weight panel is staged in plane B first.
//   2. cv2's x0 chunks for the tile's pixels (accumulators stay in registers from here on); T = 5-wide row maxima of A -> B.
//   3. Y1 = 5-high column maxima of T, on the tile + 4 pixels -> A (x0 is no longer needed).
//   4. cv2's y1 chunks; Y2 = max of Y1 at the four (+-2, +-2) neighbours, on the tile + 2 pixels -> B: the union of four 5x5 windows is the 9x9 one.
//   5. cv2's y2 chunks; y3 = max of Y2 at the four (+-2, +-2) neighbours, on the tile -> A; cv2's y3 chunks; activation, rounding, store.
// Window positions outside the map behave as -inf: every tap index is clamped to the map instead, which names an element the clipped window already
// holds (a maximum does not mind duplicates), so there is no halo to fill and no bounds test around the LDS reads.
// In LDS a bf16 value is kept as the 16-bit integer that orders the same way (sign-magnitude -> two's complement: negative values have their low 15
// bits inverted, the transform is its own inverse; -0 < +0 as in IEEE maximum; a NaN is stored as the positive quiet NaN, the largest key, so it
// propagates as pool_max does), and two values are compared per instruction (v_pk_max_i16).  The keys are turned back when a B fragment is read.
// cv2's panel (256 KB at c2 = 256) is streamed from L2 into registers: a wave owns a quarter (half) of the output channels for half (a quarter) of the
// tile's pixel groups and requests its weight fragments a whole concat slot at a time, a pooling phase ahead of the MFMAs.  Workgroups share nothing.
#include <algorithm>

#include "conv_igemm_kernel.h"

struct SppfArgs {   // strides in BYTES, extents < 2 GiB (bind_view): the kernel addresses through buffer descriptors
  const char* x; int xsn, xsh, xsw; uint32_t x_bytes;
  const char* y; int ysn, ysh, ysw; uint32_t y_bytes;
  const char* w1; const float* b1; const char* w2; const float* b2;
  int H, W, T, tiles_x, tiles_img, act1, act2;
  int a_bytes;                                               // size of plane A = offset of plane B in the dynamic LDS
  unsigned long long* dbg;                                   // MGDT_SPPF_DBG: 8 stamps per workgroup (10 ns ticks), null otherwise
};

constexpr int SPPF_THREADS = 512, SPPF_CPAD = 8;             // channel padding of an LDS pixel (bank spread)
constexpr int SPPF_TILES[] = {10, 8, 6, 5, 4, 3, 2, 1};      // tile edge candidates: the largest whose planes fit LDS (sppf_plan)
constexpr int SPPF_STATIC = 2048;                            // room for the two static bias vectors (asserted in the kernel)
constexpr int SPPF_LDS = 160 * 1024 - SPPF_STATIC;           // dynamic LDS budget

typedef __attribute__((ext_vector_type(2))) float sppf_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 sppf_bf16x2;
typedef __attribute__((ext_vector_type(8))) short sppf_i16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int sppf_u32x4;
typedef __attribute__((__vector_size__(2 * sizeof(unsigned int)))) unsigned int sppf_u32x2v;
__device__ __forceinline__ uint32_t sppf_pk_bf16(float lo, float hi) {      // two floats -> two bf16, round to nearest even
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(sppf_f32x2{lo, hi}, sppf_bf16x2));
}
// two bf16 <-> two ordered int16 keys (an involution: the sign bits stay)
__device__ __forceinline__ uint32_t sppf_key(uint32_t v) { return v ^ (((v >> 15) & 0x00010001u) * 0x7fffu); }
__device__ __forceinline__ sppf_u32x4 sppf_key4(sppf_u32x4 v) { return sppf_u32x4{sppf_key(v[0]), sppf_key(v[1]), sppf_key(v[2]), sppf_key(v[3])}; }
__device__ __forceinline__ sppf_u32x4 sppf_kmax(sppf_u32x4 p, sppf_u32x4 q) {   // 8 keys
  return __builtin_bit_cast(sppf_u32x4, __builtin_elementwise_max(__builtin_bit_cast(sppf_i16x8, p), __builtin_bit_cast(sppf_i16x8, q)));
}
__device__ __forceinline__ float sppf_nan_pos(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v; }
__device__ __forceinline__ int sppf_clamp(int v, int hi) { return min(max(v, 0), hi); }

// KC1 = K chunks of cv1 (c1 = 32 * KC1, even); c_ = c1 / 2 = 16 * KC1: KC1 cout blocks of cv1, KC1 / 2 K chunks per concat slot; NB2 = c2 / 16
template <int KC1, int NB2>
__global__ __launch_bounds__(SPPF_THREADS) void sppf_fuse_kernel(const SppfArgs a) {
  typedef bf16x8 frag;
  constexpr int NB1 = KC1, KCM = KC1 / 2, CQ = 2 * KC1;       // CQ = 16-byte pieces of a pixel's c_ channels
  constexpr int RS = (NB1 * 16 + SPPF_CPAD) * 2;            // bytes per LDS pixel
  constexpr int W1V = KC1 * NB1 * 64;                       // 16-byte vectors of cv1's panel
  constexpr int CW = NB2 % 4 == 0 ? 4 : 2, NBW = NB2 / CW;  // cv2: waves across the output channels, cout blocks of a wave
  constexpr int PW = 8 / CW, MT2 = (7 + PW - 1) / PW;       // ... waves across the tile's (at most 7) pixel groups, groups of a wave
  static_assert((NB1 + NB2) * 16 * sizeof(float) <= SPPF_STATIC, "the bias vectors outgrow their share of the 160 KiB");
  static_assert(KC1 % 2 == 0 && MT2 * PW >= 7, "whole K chunks per concat slot; seven pixel groups of a 10 x 10 tile");
  extern __shared__ __attribute__((aligned(16))) char sppf_sm[];
  __shared__ __attribute__((aligned(16))) float bl1[NB1 * 16];
  __shared__ __attribute__((aligned(16))) float bl2[NB2 * 16];
  char* const A = sppf_sm;
  char* const B = sppf_sm + a.a_bytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  unsigned long long* const dbgw = (a.dbg && tid == 0) ? a.dbg + (size_t)blockIdx.x * 8 : nullptr;
  if (dbgw) dbgw[0] = wall_clock64();

  // ---- the tile, its region (tile + 6, clipped to the map) and the sub-regions of the pooling planes: all uniform ----
  const int n = (int)blockIdx.x / a.tiles_img, tile = (int)blockIdx.x - n * a.tiles_img;
  const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
  const int H = a.H, W = a.W;
  const int y0 = tyi * a.T, x0 = txi * a.T, th = min(a.T, H - y0), tw = min(a.T, W - x0);
  const int ry0 = max(y0 - 6, 0), ry1 = min(y0 + th + 6, H), rx0 = max(x0 - 6, 0), rx1 = min(x0 + tw + 6, W);
  const int RH = ry1 - ry0, RW = rx1 - rx0, RP = RH * RW, NG1 = (RP + 15) >> 4;
  const int uy0 = max(y0 - 4, 0), uy1 = min(y0 + th + 4, H), ux0 = max(x0 - 4, 0), ux1 = min(x0 + tw + 4, W), UW = ux1 - ux0;   // Y1 (and T's columns)
  const int vy0 = max(y0 - 2, 0), vy1 = min(y0 + th + 2, H), vx0 = max(x0 - 2, 0), vx1 = min(x0 + tw + 2, W), VW = vx1 - vx0;   // Y2

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.y_bytes, 0x00020000);

  // ---- cv1's input: a wave takes the region's pixel groups (16 pixels) in pairs 2p, 2p + 1, p = wave, wave + 8, ... ----
  auto request = [&](int p, frag(&P)[2][KC1]) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int rp = (2 * p + mt) * 16 + r;
      const bool pv = rp < RP;                              // pixels past the region: the address is out of range, the loads give 0
      const int rr = pv ? rp / RW : 0, rc = pv ? rp - rr * RW : 0;
      const int off = pv ? n * a.xsn + (ry0 + rr) * a.xsh + (rx0 + rc) * a.xsw : MGDT_OOB;
#pragma unroll
      for (int kc = 0; kc < KC1; ++kc)
        P[mt][kc] = __builtin_bit_cast(frag, __builtin_amdgcn_raw_buffer_load_b128(xrs, (uint32_t)(off + (kc * 4 + g) * 16), 0, 0));
    }
  };
  frag P[2][KC1];
  int p = wave;
  request(p, P);                                            // the first reads fly while cv1's panel is staged

  // ---- cv2's weights: my NBW cout blocks of a whole concat slot (KCM chunks) per request, issued a pooling phase ahead of its MFMAs
  // (slot 0 under cv1): a request may be a trip to memory.
  const int cw = wave % CW, pw = wave / CW;
  const char* const w2lane = a.w2 + ((size_t)(cw * NBW) * 64 + lane) * 16;
  frag Wc[KCM][NBW];
  auto request_w2 = [&](int s) __attribute__((always_inline)) {
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc)
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb) Wc[kc][nb] = *(const frag*)(w2lane + (size_t)((s * KCM + kc) * NB2 + nb) * 1024);
  };

  {
    // cv1's panel into plane B: a straight copy, the scheduler puts the 16-byte requests in front of the LDS stores
    constexpr int N1 = (W1V + SPPF_THREADS - 1) / SPPF_THREADS;
#pragma unroll
    for (int u = 0; u < N1; ++u) {
      const int i = tid + u * SPPF_THREADS;
      if (W1V % SPPF_THREADS == 0 || i < W1V) ((uint4*)B)[i] = ((const uint4*)a.w1)[i];
    }
    if (tid < NB1 * 16) bl1[tid] = a.b1[tid];
    if (tid < NB2 * 16) bl2[tid] = a.b2[tid];
  }
  __syncthreads();
  if (dbgw) dbgw[1] = wall_clock64();
  request_w2(0);                                            // lands under cv1 (behind the barrier: in front of the staging it raised the register count)

  // The code below is kept short - rolled loops over cv1's cout blocks and cv2's concat slots: a workgroup runs it once, on a cold instruction cache
  // (DESIGN.md section 8, Round 10).

  // ---- 1. cv1 on the region, into plane A as keys: one cout block per iteration, its K chain over the resident pixel fragments ----
  auto cv1_blocks = [&](auto actf) __attribute__((always_inline)) {
    const char* const w1lane = B + lane * 16;
    while (2 * p < NG1) {
      char* const dst = A + (2 * p * 16 + r) * RS + 8 * g;  // the accumulator layout's slot: channels nb*16 + 4g .. +3 of pixel r
      const bool second = 2 * p + 1 < NG1;                  // plane A holds NG1 * 16 pixels
#pragma unroll 1
      for (int nb = 0; nb < NB1; ++nb) {
        f32x4 acc0 = *(const f32x4*)(&bl1[nb * 16 + 4 * g]), acc1 = acc0;
#pragma unroll
        for (int kc = 0; kc < KC1; ++kc) {
          const frag Wf = *(const frag*)(w1lane + (kc * NB1 + nb) * 1024);
          acc0 = mma(Wf, P[0][kc], acc0);
          acc1 = mma(Wf, P[1][kc], acc1);
        }
        *(uint2*)(dst + nb * 32) = make_uint2(sppf_key(sppf_pk_bf16(sppf_nan_pos(actf(acc0[0])), sppf_nan_pos(actf(acc0[1])))),
                                              sppf_key(sppf_pk_bf16(sppf_nan_pos(actf(acc0[2])), sppf_nan_pos(actf(acc0[3])))));
        if (second)
          *(uint2*)(dst + 16 * RS + nb * 32) = make_uint2(sppf_key(sppf_pk_bf16(sppf_nan_pos(actf(acc1[0])), sppf_nan_pos(actf(acc1[1])))),
                                                          sppf_key(sppf_pk_bf16(sppf_nan_pos(actf(acc1[2])), sppf_nan_pos(actf(acc1[3])))));
      }
      p += 8;
      if (2 * p < NG1) request(p, P);
    }
  };
  switch (a.act1) {                                         // the epilogue forms of conv_igemm_kernel
    case MGDT_ACT_SILU: cv1_blocks([](float v) { return v * fast_sigmoid(v); }); break;
    case MGDT_ACT_RELU: cv1_blocks([](float v) { return fmaxf(v, 0.f); }); break;
    default: cv1_blocks([](float v) { return v; }); break;
  }
  __syncthreads();                                          // plane A is complete, the panel in plane B is dead
  if (dbgw) dbgw[2] = wall_clock64();

  // ---- my pixels of the tile for cv2: group pw + PW * mt, lane r's pixel of it ----
  int aoff[MT2], voff[MT2], yo[MT2];
#pragma unroll
  for (int mt = 0; mt < MT2; ++mt) {
    const int t = (pw + PW * mt) * 16 + r;
    const bool pv = t < th * tw;                            // pixels past the tile compute on pixel 0 and store nowhere
    const int tt = pv ? t : 0, tr = tt / tw, tc = tt - tr * tw;
    const int row = y0 + tr, col = x0 + tc;
    aoff[mt] = ((row - ry0) * RW + (col - rx0)) * RS + 16 * g;      // the B fragment's slot: channels kc*32 + 8g .. +7 of the pixel
    voff[mt] = ((row - vy0) * VW + (col - vx0)) * RS + 16 * g;
    yo[mt] = pv ? n * a.ysn + row * a.ysh + col * a.ysw + 8 * g : MGDT_OOB;
  }
  f32x4 acc2[NBW][MT2];
#pragma unroll
  for (int nb = 0; nb < NBW; ++nb) {
    const f32x4 b = *(const f32x4*)(&bl2[(cw * NBW + nb) * 16 + 4 * g]);
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt) acc2[nb][mt] = b;
  }

  // max of the four (+-2, +-2) neighbours (clamped to the map) of pixel (rw, c): src indexed [row - sy0][col - sx0] with row length SW
  auto max4 = [&](const char* src, int sy0, int sx0, int SW, int rw, int c, int cq) __attribute__((always_inline)) {
    const int ra = (sppf_clamp(rw - 2, H - 1) - sy0) * SW - sx0, rb = (sppf_clamp(rw + 2, H - 1) - sy0) * SW - sx0;
    const int ca = sppf_clamp(c - 2, W - 1), cb = sppf_clamp(c + 2, W - 1);
    const char* const base = src + cq * 16;
    return sppf_kmax(sppf_kmax(*(const sppf_u32x4*)(base + (ra + ca) * RS), *(const sppf_u32x4*)(base + (ra + cb) * RS)),
                     sppf_kmax(*(const sppf_u32x4*)(base + (rb + ca) * RS), *(const sppf_u32x4*)(base + (rb + cb) * RS)));
  };

  // ---- 2..5. cv2, one concat slot per iteration: its MFMAs on the plane that holds the slot, the request of the next slot's weights, then the
  // pooling pass that makes the next slot's plane ----
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    const char* const plane = s == 2 ? B : A;               // x0, Y1 and y3 live in A (the region's indexing), Y2 in B
#pragma unroll
    for (int kc = 0; kc < KCM; ++kc) {
      frag Bf[MT2];
#pragma unroll
      for (int mt = 0; mt < MT2; ++mt) Bf[mt] = __builtin_bit_cast(frag, sppf_key4(*(const sppf_u32x4*)(plane + (s == 2 ? voff[mt] : aoff[mt]) + kc * 64)));
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb)
#pragma unroll
        for (int mt = 0; mt < MT2; ++mt) acc2[nb][mt] = mma(Wc[kc][nb], Bf[mt], acc2[nb][mt]);
      __builtin_amdgcn_sched_barrier(0);                    // one chunk's B fragments live at a time
    }
    if (s == 3) break;
    request_w2(s + 1);                                      // into the registers the MFMAs above have just read (behind the last sched_barrier)
    __builtin_amdgcn_sched_barrier(0);
    if (s == 0) {
      // T = 5-wide row maxima of A on the region's rows x Y1's columns -> B
      for (int i = tid; i < RH * UW * CQ; i += SPPF_THREADS) {
        const int cq = i % CQ, px = i / CQ, rr = px / UW, cc = px - rr * UW, c = ux0 + cc;
        const int rowi = rr * RW - rx0;                     // + column = the region's pixel index
        const char* const base = A + cq * 16;
        sppf_u32x4 m = *(const sppf_u32x4*)(base + (rowi + c) * RS);
#pragma unroll
        for (int d = -2; d <= 2; ++d)
          if (d) m = sppf_kmax(m, *(const sppf_u32x4*)(base + (rowi + sppf_clamp(c + d, W - 1)) * RS));
        *(sppf_u32x4*)(B + px * RS + cq * 16) = m;
      }
      __syncthreads();
      if (dbgw) dbgw[3] = wall_clock64();
      // Y1 = 5-high column maxima of T -> A, at the region's own indexing (every wave is past its x0 chunks)
      for (int i = tid; i < (uy1 - uy0) * UW * CQ; i += SPPF_THREADS) {
        const int cq = i % CQ, px = i / CQ, rr = px / UW, cc = px - rr * UW, rw = uy0 + rr;
        const char* const base = B + cq * 16;
        sppf_u32x4 m = *(const sppf_u32x4*)(base + (px + (uy0 - ry0) * UW) * RS);
#pragma unroll
        for (int d = -2; d <= 2; ++d)
          if (d) m = sppf_kmax(m, *(const sppf_u32x4*)(base + ((sppf_clamp(rw + d, H - 1) - ry0) * UW + cc) * RS));
        *(sppf_u32x4*)(A + ((rw - ry0) * RW + (ux0 + cc - rx0)) * RS + cq * 16) = m;
      }
    } else if (s == 1) {
      // Y2 = max of Y1 at (+-2, +-2), on the tile + 2 -> B (T is dead)
      for (int i = tid; i < (vy1 - vy0) * VW * CQ; i += SPPF_THREADS) {
        const int cq = i % CQ, px = i / CQ, rr = px / VW, cc = px - rr * VW;
        *(sppf_u32x4*)(B + px * RS + cq * 16) = max4(A, ry0, rx0, RW, vy0 + rr, vx0 + cc, cq);
      }
    } else {
      // y3 = max of Y2 at (+-2, +-2), on the tile -> A (Y1 is dead: every wave is past its y1 chunks and the Y2 pass)
      for (int i = tid; i < th * tw * CQ; i += SPPF_THREADS) {
        const int cq = i % CQ, px = i / CQ, rr = px / tw, cc = px - rr * tw;
        *(sppf_u32x4*)(A + ((y0 + rr - ry0) * RW + (x0 + cc - rx0)) * RS + cq * 16) = max4(B, vy0, vx0, VW, y0 + rr, x0 + cc, cq);
      }
    }
    __syncthreads();
    if (dbgw) dbgw[4 + s] = wall_clock64();
  }

  // ---- epilogue: lane holds couts (cw * NBW + nb) * 16 + 4g .. +3 of its pixels; out-of-tile pixels are dropped by the descriptor ----
  auto epilogue = [&](auto actf) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt)
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb) {
        const f32x4 c = acc2[nb][mt];
        const sppf_u32x2v o = {sppf_pk_bf16(actf(c[0]), actf(c[1])), sppf_pk_bf16(actf(c[2]), actf(c[3]))};
        __builtin_amdgcn_raw_buffer_store_b64(o, yrs, (uint32_t)(yo[mt] + (cw * NBW + nb) * 32), 0, 0);
      }
  };
  switch (a.act2) {
    case MGDT_ACT_SILU: epilogue([](float v) { return v * fast_sigmoid(v); }); break;
    case MGDT_ACT_RELU: epilogue([](float v) { return fmaxf(v, 0.f); }); break;
    default: epilogue([](float v) { return v; }); break;
  }
  if (dbgw) dbgw[7] = wall_clock64();
}

static bool sppf_act_ok(int act) { return act == MGDT_ACT_NONE || act == MGDT_ACT_SILU || act == MGDT_ACT_RELU; }

// The largest tile edge whose two LDS planes fit: A = the largest region (tile + 6 on each side, clipped to the map) in whole pixel groups, B = the
// larger of cv1's panel and the T plane (region rows x tile + 4 on each side; Y2, tile + 2, is smaller).  On a 20 x 20 map a 10 x 10 tile always
// touches a border, so its region is 16 x 16, not 22 x 22.
static int sppf_extent(int size, int t, int halo) {         // the longest clipped [o - halo, o + t + halo) over the tiles o = 0, t, 2t, ...
  int m = 0;
  for (int o = 0; o < size; o += t) m = std::max(m, std::min(o + std::min(t, size - o) + halo, size) - std::max(o - halo, 0));
  return m;
}
static bool sppf_plan(int cm, int h, int w, int* T, int* a_bytes, int* lds) {
  const int RS = (cm + SPPF_CPAD) * 2, panel = (2 * cm / 32) * (cm / 16) * 1024;
  for (int t : SPPF_TILES) {
    const int rh = sppf_extent(h, t, 6), rw = sppf_extent(w, t, 6), uw = sppf_extent(w, t, 4);
    const long ab = (long)cdiv((long)rh * rw, 16) * 16 * RS, bb = std::max((long)panel, (long)rh * uw * RS);
    if (ab + bb > SPPF_LDS) continue;
    *T = t; *a_bytes = (int)ab; *lds = (int)(ab + bb);
    return true;
  }
  return false;
}

/* 1 when mgdt_sppf_fuse_fwd covers the shapes: bf16, cv1 c1 -> cm = c1 / 2, cv2 4 * cm -> c2 with (c1, c2) in {(64, 64), (64, 96), (256, 256)},
 * activations none / SiLU / ReLU */
extern "C" int mgdt_sppf_fuse_supported(int c1, int cm, int c2, int h, int w, int act1, int act2, int dtype) {
  if (dtype != MGDT_BF16 || c1 != 2 * cm || h < 1 || w < 1 || h > 4096 || w > 4096 || !sppf_act_ok(act1) || !sppf_act_ok(act2)) return 0;
  if (!((c1 == 64 && (c2 == 64 || c2 == 96)) || (c1 == 256 && c2 == 256))) return 0;
  int T, ab, lds;
  return sppf_plan(cm, h, w, &T, &ab, &lds) ? 1 : 0;
}

template <int KC1, int NB2>
static int sppf_launch(const SppfArgs& a, int grid, int lds, hipStream_t st) {
  if (int rc = lds_optin<sppf_fuse_kernel<KC1, NB2>>("sppf_fuse", SPPF_LDS)) return rc;   // the static bias vectors take part of the 160 KiB
  static StampBuf stamps;      // MGDT_SPPF_DBG: 8 words per workgroup
  SppfArgs b = a;
  const bool dbg = knob_set("MGDT_SPPF_DBG");
  if (dbg && !stamps.ensure((size_t)grid * 8)) MGDT_FAIL(MGDT_WORKSPACE, "sppf_fuse: no memory for the MGDT_SPPF_DBG stamps");
  b.dbg = dbg ? stamps.p : nullptr;
  sppf_fuse_kernel<KC1, NB2><<<grid, SPPF_THREADS, lds, st>>>(b);
  MGDT_CHECK_LAUNCH("sppf_fuse_fwd");
  if (dbg) {
    const std::vector<unsigned long long> h = stamps.read((size_t)grid * 8, st);
    unsigned long long t0 = ~0ull, t7 = 0; double ph[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < grid; ++i) { t0 = std::min(t0, h[i * 8]); t7 = std::max(t7, h[i * 8 + 7]); for (int j = 0; j < 7; ++j) ph[j] += (double)(h[i * 8 + j + 1] - h[i * 8 + j]); }
    fprintf(stderr, "sppf_fuse x10ns: %d WGs, span %llu; avg per WG: load+stage %.0f cv1 %.0f x0+rowmax %.0f colmax %.0f y1+Y2 %.0f y2+y3 %.0f y3+store %.0f\n", grid, t7 - t0,
            ph[0] / grid, ph[1] / grid, ph[2] / grid, ph[3] / grid, ph[4] / grid, ph[5] / grid, ph[6] / grid);
  }
  return MGDT_OK;
}

extern "C" int mgdt_sppf_fuse_fwd(const mgdt_view* x, const void* packed_w1, const float* bias1, int act1, const void* packed_w2, const float* bias2,
                                  int act2, const mgdt_view* y, int dtype, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(y) || !packed_w1 || !bias1 || !packed_w2 || !bias2) MGDT_FAIL(MGDT_BAD_ARG, "sppf_fuse: null/empty argument");
  if (!mgdt_sppf_fuse_supported(x->c, x->c / 2, y->c, y->h, y->w, act1, act2, dtype))
    MGDT_FAIL(MGDT_BAD_SHAPE, "sppf_fuse: shapes/dtype/activations not covered (see mgdt_sppf_fuse_supported)");
  if (x->n != y->n || x->h != y->h || x->w != y->w) MGDT_FAIL(MGDT_BAD_SHAPE, "sppf_fuse: x and y must share n, h, w");
  SppfArgs a;
  memset(&a, 0, sizeof(a));
  const ViewPolicy vx = {8, true, 0, 0, false}, vy = {4, true, 0, 0, false};   // 16-byte pieces of x's pixels, 8-byte pieces of y's
  if (!bind_view(x, 2, vx, &a.x, &a.xsn, &a.xsh, &a.xsw, &a.x_bytes) || !bind_view(y, 2, vy, &a.y, &a.ysn, &a.ysh, &a.ysw, &a.y_bytes))
    MGDT_FAIL(MGDT_BAD_SHAPE, "sppf_fuse: views must be NHWC (sc == 1), x 16-byte and y 8-byte aligned, and < 2 GiB");
  int lds = 0;
  if (!sppf_plan(x->c / 2, y->h, y->w, &a.T, &a.a_bytes, &lds)) MGDT_FAIL(MGDT_BAD_SHAPE, "sppf_fuse: no tile fits LDS");
  a.w1 = (const char*)packed_w1; a.b1 = bias1; a.w2 = (const char*)packed_w2; a.b2 = bias2; a.act1 = act1; a.act2 = act2;
  a.H = y->h; a.W = y->w; a.tiles_x = cdiv(a.W, a.T); a.tiles_img = a.tiles_x * cdiv(a.H, a.T);
  const long grid = (long)y->n * a.tiles_img;
  if (grid >= 0x7fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "sppf_fuse: too many tiles");
  hipStream_t st = (hipStream_t)s;
  const int kc1 = x->c / 32, nb2 = y->c / 16;
#define SPPF_CASE(K, N) if (kc1 == K && nb2 == N) return sppf_launch<K, N>(a, (int)grid, lds, st);
  SPPF_CASE(2, 4) SPPF_CASE(2, 6) SPPF_CASE(8, 16)
#undef SPPF_CASE
  MGDT_FAIL(MGDT_BAD_SHAPE, "sppf_fuse: no kernel for kc1=%d nb2=%d", kc1, nb2);
}
