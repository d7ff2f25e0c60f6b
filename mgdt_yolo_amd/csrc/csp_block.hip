// One launch per CSP block (MSPA_C2f / C2f) of the bf16 inference path: the whole block for one spatial tile of one image stays on the
// CU.  Reference: nn/modules/block.py:209-287 (MSPA_C2f), :187-207 (C2f), :514-526 (Bottleneck).
//
//   front   MSPA: sp0 = cv0(x0), sp1 = cv1(sp0 + x1), sp2 = cv2(sp1 + x2)   (register-chained MFMAs, as mgdt_pw_chain3_fwd)
//           C2f : [y0 | y1] = cv1(x) comes from the ordinary 1x1 conv launch; the front copies it into the tile buffers
//   middle  n bottlenecks, each two 3x3 convs wd -> wd (+ shortcut), on LDS-resident maps of the tile + halo
//   back    1x1 conv over the concat [front outputs | bottleneck outputs] -> Cout, written to HBM; MSPA: per-tile channel sums for
//           the SPR pooling attention (the block output is never re-read for pooling)
//
// Why: at 20x20 .. 80x80 the unfused block is 7-8 dependent launches of 10-40 us with < 5 us of work each (grids far below 256 CUs,
// one fill/drain each).  Here a workgroup (8 waves) owns a TH x TW tile of one image; the bottleneck chain needs a halo of 2n pixels,
// which is recomputed per tile (the recomputed part is cheap: K <= 576, and it is MFMA work that replaces HBM round trips).
//
// Layout on the CU: two NHWC maps P (bottleneck input / output) and T (its hidden map) over the (TH+2h) x (TW+2h) region, pixel stride
// wd*2 bytes, and the concat buffer of the tile's own pixels without the last bottleneck's output (the back conv reads that one from P).
// No padding: the 16-byte slots of a pixel row are XOR-swizzled by the pixel index (csp_psw, cat_at) so that every ds_read_b128 lane
// group of the 3x3 convs and of the back conv hits 16 different slots of the 256-byte bank row.
// Pixel walk of the 3x3 convs: conv j (0 .. 2n - 1) needs the rectangle of rows / columns j + 1 .. RH - j - 2 / RW - j - 2 of the region.
// Its pixels are numbered row-major and taken in groups of 16 (compact walk: one FastDiv per conv turns the number into the region
// pixel); lanes past the end of the last group are clamped to the last pixel and store nothing.  Nothing outside the rectangle is
// written: conv j + 1 reads the rectangle one ring wider than its own, which is conv j's; the shortcut reads `out` at the pixel it
// writes; the concat copy and the back conv read tile pixels only, the last conv's rectangle.  For wd <= 16 (no swizzle) a tap is a
// per-lane constant byte offset: B operand = one ds_read_b128 at (pixel * stride + boff[tap]); for wd 32 / 64 the slot XOR is formed
// from the tap pixel's byte offset once per group and tap (bsw).  MGDT_CSP_COMPACT=0 selects the earlier linear walk (the range
// [lo, hi) of region pixels from the rectangle's first to its last pixel, wrap-around columns computed and never consumed; there the
// swizzle depends on the pixel index mod 16 only and is baked into boff): same MFMAs and rounding per needed pixel, same bits.
// Pixel coordinates (image offset, tile index) are computed from the pixel index where they are needed, not stored in LDS tables.
// GEMM orientation as conv_igemm: weights = A operand (rows = 16 output channels), pixels = B operand, so a lane ends with 4 consecutive
// channels of one pixel = one 8-byte LDS / HBM store.  Each wave keeps the weight fragments of ONE cout block of the running conv in
// registers (weights-stationary: 12..72 VGPRs) and streams pixel groups through them; the packed panels are the ordinary
// mgdt_conv_pack layout, read straight from L2.  Pixels outside the image are written as zeros (the next conv's zero padding).
#include <algorithm>
#include <type_traits>
#include <vector>

#include "conv_igemm_kernel.h"

struct CspArgs {
  const char* x; int xsn, xsh, xsw; uint32_t x_bytes;
  char* y; int ysn, ysh, ysw; uint32_t y_bytes;
  const char* front; const float* front_bias;
  const char* mid[4]; const float* mid_bias[4];
  const char* back; const float* back_bias;
  float* pool;
  int N, H, W, Cin, Cout, wd, nbtl, shortcut, act;
  int TH, TW, halo, RH, RW, tiles_x, tiles_y, total_tiles, per_xcd;
  int catC, nchb, nbo;                 // concat channels, K chunks / cout blocks of the back conv
  int RPA, TPA, CS;                    // allocated region / tile pixels, pixel stride (bytes) of the concat buffer (P/T: 2 * wd)
  int catS, cmsk, csh;                 // concat channels held in the concat buffer (catC - wd), its slot swizzle (t >> csh) & cmsk
  int chain_words;                     // MSPA: 16-byte words of the chain blob's weight part
  unsigned long long* dbg;             // MGDT_CSP_DBG: 8 wall-clock stamps (10 ns units) per workgroup
  int pool_gst;                        // back phase: waves per cout block = pool slots per tile (1 when there are >= 8 cout blocks)
  FastDiv fd_rw, fd_tw, fd_tx, fd_tpi; // pixel coordinates: division by region width / tile width / tiles per row / tiles per image without the ~40-instruction sequence
  FastDiv fd_cw[4];                    // compact walk: division by the width RW - 2j - 2 of 3x3 conv j's output rectangle
};

constexpr int CSP_THREADS = 512;
constexpr int CSP_NW = CSP_THREADS / 64;
constexpr int CSP_NCHB_MAX = 8;        // back conv: K <= 256 concat channels (host-side bound)
// workgroups per CU that the registers allow: the paired wd 8 form fits 80 VGPRs without scratch = three (its tile takes 41 KB of LDS),
// wd 16 / 32 and the unpaired wd 8 form <= 128 = two, wd 64 one
constexpr int csp_waves_per_simd(int wd, bool pair) { return wd == 8 && pair ? 6 : (wd <= 32 ? 4 : 2); }

// SiLU only, branch-free (the host refuses anything else): a run-time activation switch here turned every epilogue into four serial
// branchy exp -> rcp chains; as straight-line code the four values' transcendentals interleave
__device__ __forceinline__ float csp_act(float v, int) { return v * fast_sigmoid(v); }

typedef __attribute__((__vector_size__(2 * sizeof(unsigned int)))) unsigned int csp_raw2;

__device__ __forceinline__ void lds_store4(char* p, f32x4 v) {
  bf16x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (bf16)v[i];
  *(bf16x4*)p = o;
}
// XOR applied to the 16-byte slot index of a P/T pixel (wd * 2 bytes): with it the 3x3 convs' ds_read_b128 lane groups are conflict-free
// for wd = 32 / 64; for wd <= 16 the unswizzled rows are already within 10 % of conflict-free.  A function of pix mod 16 only.
template <int WD> __device__ __forceinline__ int csp_psw(int pix) { return WD == 64 ? (pix & 7) : (WD == 32 ? ((pix >> 1) & 3) : 0); }

__device__ __forceinline__ f32x4 lds_load4(const char* p) {
  const bf16x4 o = *(const bf16x4*)p;
  return f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
}

// v_permlane32_swap: lanes 32-63 of `lo` trade places with lanes 0-31 of `hi`.  Returned: [0] = lo's lower half | hi's lower half,
// [1] = lo's upper half | hi's upper half.
__device__ __forceinline__ csp_raw2 csp_swap32(unsigned int lo, unsigned int hi) { return __builtin_amdgcn_permlane32_swap(lo, hi, false, false); }
// two accumulators that are live in lanes 0-31 only -> one: a's live half in lanes 0-31, b's in lanes 32-63
__device__ __forceinline__ f32x4 csp_merge(f32x4 va, f32x4 vb) {
  f32x4 m;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float fa = va[j], fb = vb[j];                            // scalars first: a bit cast of a vector ELEMENT reads element 0 for every j
    m[j] = __uint_as_float(csp_swap32(__float_as_uint(fa), __float_as_uint(fb))[0]);
  }
  return m;
}

// MODE 0 = MSPA_C2f, 1 = C2f.  WD = bottleneck width (8, 16, 32, 64).
// PAIR (WD = 8 only): a 16-row MFMA block carries 8 real output channels there, so lanes 32-63 (g = 2, 3) of every accumulator hold padding.
// The paired form keeps every MFMA as it is and merges the accumulators of two pixel groups into one register set (group a in lanes 0-31,
// group b in lanes 32-63; a lane's channels are 4 * (g & 1) ..) before the SiLU / round / store epilogue, which then runs once for both.
// The front also loads a pair with all 64 lanes live and splits the rounded operand back into two B operands whose upper halves are real
// zeros (0 * Inf of the neighbouring group must not reach this one).  Same arithmetic in the same order: the outputs are bit-identical.
// COMPACT: the 3x3 convs form their 16-pixel groups over the pixels of the output rectangle only (see the header); false = the linear walk.
template <int WD, int MODE, bool PAIR = false, bool COMPACT = true>
__global__ __launch_bounds__(CSP_THREADS, csp_waves_per_simd(WD, PAIR)) void csp_block_kernel(const CspArgs a) {
  static_assert(!PAIR || (WD == 8 && MODE == 0), "the paired epilogue is the wd = 8 MSPA form");
  constexpr int CP = WD / 8;                         // 16-byte pieces per tap
  constexpr int NCHB = WD == 8 ? 2 : (WD == 16 ? 3 : (WD == 32 ? 5 : 8));   // K chunks of the back conv at n = 2 (concat <= 256 channels)
  constexpr int NB = WD >= 16 ? WD / 16 : 1;         // cout blocks of a wd -> wd conv
  constexpr int NCH = (9 * CP + 3) / 4;              // K chunks of a 3x3 conv
  constexpr int NBK = NB, KC = (NBK + 1) / 2;        // pw chain geometry (mlp_chain.hip)
  constexpr int PS = 2 * WD;                         // P/T pixel stride (bytes)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Pb = smem;                                               // RPA, TPA are multiples of 16: every array below starts 16-byte aligned
  char* Tb = Pb + (size_t)a.RPA * PS;
  char* catb = Tb + (size_t)a.RPA * PS;                          // [TPA][catS] concat of the tile's pixels (the last bottleneck output stays in P)
  char* wl = catb + (size_t)a.TPA * a.CS;                        // MSPA: staged chain weights + bias

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;

  // XCD k (workgroup id % 8) takes the contiguous tile range [k*per_xcd, (k+1)*per_xcd): neighbouring tiles share their halo in that XCD's L2
  const int v = blockIdx.x;
  const int tlin = (v & 7) * a.per_xcd + (v >> 3);
  if ((v >> 3) >= a.per_xcd || tlin >= a.total_tiles) return;    // uniform per workgroup: no barrier is skipped by a part of it
  const int tpi = a.tiles_x * a.tiles_y;
  const int n = (int)fdiv((uint32_t)tlin, a.fd_tpi), trem = tlin - n * tpi;
  const int tyi = (int)fdiv((uint32_t)trem, a.fd_tx);
  const int ty0 = tyi * a.TH, tx0 = (trem - tyi * a.tiles_x) * a.TW;
  const int RP = a.RH * a.RW, TP = a.TH * a.TW;
  const bool inner = ty0 >= a.halo && tx0 >= a.halo && ty0 + a.TH + a.halo <= a.H && tx0 + a.TW + a.halo <= a.W;   // region inside the image
  auto stamp = [&](int k) __attribute__((always_inline)) { if (a.dbg && tid == 0) a.dbg[(size_t)tlin * 8 + k] = __builtin_amdgcn_s_memrealtime(); };
  // region pixel q -> byte offset in the x view (MGDT_OOB outside the image) and index in the tile (-1 outside it)
  auto region_px = [&](int q, int& go, int& ct) __attribute__((always_inline)) {
    const int ry = (int)fdiv((uint32_t)q, a.fd_rw), rx = q - ry * a.RW;
    const int iy = ty0 - a.halo + ry, ix = tx0 - a.halo + rx;
    go = (q < RP && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? n * a.xsn + iy * a.xsh + ix * a.xsw : MGDT_OOB;
    const int cy = ry - a.halo, cx = rx - a.halo;
    ct = (q < RP && (unsigned)cy < (unsigned)a.TH && (unsigned)cx < (unsigned)a.TW) ? cy * a.TW + cx : -1;
  };
  // byte offsets of channel c (a multiple of 4) of P/T pixel q and of concat pixel t
  auto pt_at = [&](int q, int c) __attribute__((always_inline)) { return q * PS + ((((c >> 3) ^ csp_psw<WD>(q)) << 4) | ((c & 7) << 1)); };
  auto cat_at = [&](int t, int c) __attribute__((always_inline)) { return t * a.CS + ((((c >> 3) ^ ((t >> a.csh) & a.cmsk)) << 4) | ((c & 7) << 1)); };
  stamp(0);

  // weights-stationary: this wave's cout block of the running 3x3 conv lives in registers.  Every conv's fragments are requested one
  // phase AHEAD (the first ones right here, before the zero fill and the front), so no phase starts by waiting on L2.
  const int nbv = wave % NB, gvm = wave / NB, gstm = CSP_NW / NB;
  bf16x8 A[NCH];
  f32x4 bias;
  auto load_a0 = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int kc = 0; kc < NCH; ++kc) A[kc] = *(const bf16x8*)(a.mid[0] + ((size_t)(kc * NB + nbv) * 64 + lane) * 16);
    bias = *(const f32x4*)(a.mid_bias[0] + nbv * 16 + 4 * g);
  };
  if (WD != 32 || MODE != 0) load_a0();

  // ---- zero fill, chain weights
  {
    const int words = (int)(((size_t)2 * a.RPA * PS) >> 4);
    uint4* z = (uint4*)Pb;
    for (int i = tid; i < words; i += CSP_THREADS) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (MODE == 0) {
    for (int i = tid; i < a.chain_words; i += CSP_THREADS) ((uint4*)wl)[i] = ((const uint4*)a.front)[i];
    float* bl = (float*)(wl + (size_t)a.chain_words * 16);
    for (int i = tid; i < 3 * NBK * 16; i += CSP_THREADS) bl[i] = ((const float*)(a.front + (size_t)a.chain_words * 16))[i];
  }
  __syncthreads();
  stamp(1);

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.y_bytes, 0x00020000);
  const int ngr = (RP + 15) >> 4;                                // 16-pixel groups of the region

  // ================================================================ front
  if (MODE == 0) {
    // each wave takes a contiguous run of pixel groups and requests the inputs of U groups before it touches the first one: the phase is
    // bound by HBM/L2 latency, not by work (a wave that waits for one group at a time leaves the CU with 16 requests in flight)
    constexpr int U = WD == 64 ? 2 : (WD == 32 ? 3 : 5);
    const char* const wlane = wl + lane * 16;
    const float* bl = (const float*)(wl + (size_t)a.chain_words * 16);
    const int per = ngr / CSP_NW, rem = ngr - per * CSP_NW;   // balanced: the first `rem` waves take one group more
    const int gbeg = wave * per + min(wave, rem), gend = gbeg + per + (wave < rem ? 1 : 0);
    if constexpr (PAIR) {
      // groups in pairs: lane (r, g) holds channels 4 (g & 1) .. of pixel r of group g >> 1, so every load, SiLU and store lane is live
      constexpr int UP = 3;                                      // pairs in flight (the unpaired form has 5 groups)
      const int hb = lane >> 5, cl = 4 * (g & 1);
      for (int g0 = gbeg; g0 < gend; g0 += 2 * UP) {
        int go[UP], ct[UP];
        csp_raw2 XR[UP][4];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          const int grp = g0 + 2 * u + hb;
          region_px(grp * 16 + r, go[u], ct[u]);
          if (grp >= gend) go[u] = MGDT_OOB, ct[u] = -1;         // an odd run's last group is unpaired: its upper lanes load zeros and store nothing
#pragma unroll
          for (int i = 0; i < 4; ++i) XR[u][i] = __builtin_amdgcn_raw_buffer_load_b64(xrs, (uint32_t)go[u] + (uint32_t)((i * WD + cl) * 2), 0, 0);
        }
#pragma unroll
        for (int u = 0; u < UP; ++u) {
          if (g0 + 2 * u >= gend) break;                         // wave-uniform
          const bool hasb = g0 + 2 * u + 1 < gend;               // wave-uniform
          const int q = (g0 + 2 * u + hb) * 16 + r;
          f32x4 X[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bf16x4 o = __builtin_bit_cast(bf16x4, XR[u][i]);
            X[i] = f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
          }
          f32x4 prev;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            bf16x4 vb;
#pragma unroll
            for (int e = 0; e < 4; ++e) vb[e] = (bf16)(X[i][e] + (i ? prev[e] : 0.f));
            const csp_raw2 vw = __builtin_bit_cast(csp_raw2, vb);
            // one swap per word against a zero register: [0] = group a's operand, [1] = group b's moved to lanes 0-31, both with lanes 32-63 zero
            const csp_raw2 s0 = csp_swap32(vw[0], 0u), s1 = csp_swap32(vw[1], 0u);
            typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int raw4;
            const bf16x8 Ba = __builtin_bit_cast(bf16x8, (raw4){s0[0], s1[0], 0u, 0u});
            const bf16x8 Bb = __builtin_bit_cast(bf16x8, (raw4){s0[1], s1[1], 0u, 0u});
            const f32x4 bi = *(const f32x4*)(bl + i * 16 + 4 * g);
            const bf16x8 Wf = *(const bf16x8*)(wlane + i * 1024);
            const f32x4 acca = mma(Wf, Ba, bi);
            f32x4 accb = bi;
            if (hasb) accb = mma(Wf, Bb, bi);
            f32x4 acc = csp_merge(acca, accb);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (float)(bf16)csp_act(acc[j], a.act);
            prev = acc;
            if (ct[u] >= 0) lds_store4(catb + cat_at(ct[u], i * WD + cl), acc);
          }
          // bottleneck input = sp2 + x3 (the pending add of block.py:259), zero outside the image
          f32x4 p0 = prev + X[3];
          if (go[u] == MGDT_OOB) p0 = f32x4{0.f, 0.f, 0.f, 0.f};
          if (hb == 0 || hasb) lds_store4(Pb + pt_at(q, cl), p0);
        }
      }
    } else
    for (int g0 = gbeg; g0 < gend; g0 += U) {
      int go[U], ct[U];
      csp_raw2 XR[U][4][NBK];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool gv_ = g0 + u < gend;
        const int q = (g0 + u) * 16 + r;
        region_px(q, go[u], ct[u]);
        if (!gv_) go[u] = MGDT_OOB, ct[u] = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int blk = 0; blk < NBK; ++blk) {
            const int c = blk * 16 + 4 * g;
            const int dead = c >= WD ? MGDT_OOB : 0;
            XR[u][i][blk] = __builtin_amdgcn_raw_buffer_load_b64(xrs, (uint32_t)(go[u] | dead) + (uint32_t)((i * WD + c) * 2), 0, 0);
          }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (g0 + u >= gend) break;                               // wave-uniform
        const int q = (g0 + u) * 16 + r;
        f32x4 X[4][NBK];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int blk = 0; blk < NBK; ++blk) {
            const bf16x4 o = __builtin_bit_cast(bf16x4, XR[u][i][blk]);
            X[i][blk] = f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
          }
        f32x4 prev[NBK];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          bf16x8 Bf[KC];
#pragma unroll
          for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int blk = kc * 2 + e / 4;
              float vv = 0.f;
              if (blk < NBK) vv = X[i][blk][e % 4] + (i ? prev[blk][e % 4] : 0.f);
              Bf[kc][e] = (bf16)vv;
            }
#pragma unroll
          for (int ob = 0; ob < NBK; ++ob) {
            f32x4 acc = *(const f32x4*)(bl + (i * NBK + ob) * 16 + 4 * g);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) acc = mma(*(const bf16x8*)(wlane + ((i * KC + kc) * NBK + ob) * 1024), Bf[kc], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (float)(bf16)csp_act(acc[j], a.act);
            prev[ob] = acc;
            const int c = ob * 16 + 4 * g;
            if (c < WD && ct[u] >= 0) lds_store4(catb + cat_at(ct[u], i * WD + c), acc);
          }
        }
        // bottleneck input = sp2 + x3 (the pending add of block.py:259), zero outside the image
#pragma unroll
        for (int ob = 0; ob < NBK; ++ob) {
          const int c = ob * 16 + 4 * g;
          f32x4 p0 = prev[ob] + X[3][ob];
          if (go[u] == MGDT_OOB) p0 = f32x4{0.f, 0.f, 0.f, 0.f};
          if (c < WD) lds_store4(Pb + pt_at(q, c), p0);
        }
      }
    }
  } else {
    // C2f: x is cv1's output [y0 | y1] (2*WD channels, written by the 1x1 conv launch in front of this one: a wide streaming GEMM that
    // gains nothing from living here); the front copies the tile's own pixels into the concat buffer and y1 (+ halo) into P
    constexpr int NB2 = 2 * WD / 16;
    constexpr int U = WD == 64 ? 2 : 4;
    const int per = ngr / CSP_NW, rem = ngr - per * CSP_NW;
    const int gbeg = wave * per + min(wave, rem), gend = gbeg + per + (wave < rem ? 1 : 0);
    for (int g0 = gbeg; g0 < gend; g0 += U) {
      int go[U], ct[U];
      csp_raw2 XR[U][NB2];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool gv_ = g0 + u < gend;
        const int q = (g0 + u) * 16 + r;
        region_px(q, go[u], ct[u]);
        if (!gv_) go[u] = MGDT_OOB, ct[u] = -1;
#pragma unroll
        for (int blk = 0; blk < NB2; ++blk)
          XR[u][blk] = __builtin_amdgcn_raw_buffer_load_b64(xrs, (uint32_t)go[u] + (uint32_t)((blk * 16 + 4 * g) * 2), 0, 0);   // zeros outside the image
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (g0 + u >= gend) break;                               // wave-uniform
        const int q = (g0 + u) * 16 + r;
#pragma unroll
        for (int blk = 0; blk < NB2; ++blk) {
          const int cc = blk * 16 + 4 * g;
          if (ct[u] >= 0) *(csp_raw2*)(catb + cat_at(ct[u], cc)) = XR[u][blk];
          if (cc >= WD) *(csp_raw2*)(Pb + pt_at(q, cc - WD)) = XR[u][blk];      // second half = the bottleneck chain's input (block.py:201-203)
        }
      }
    }
  }
  if (WD == 32 && MODE == 0) load_a0();
  stamp(2);
  __syncthreads();
  stamp(3);

  // ================================================================ middle: 2 * nbtl 3x3 convs, P -> T -> P ...
  constexpr bool PREB = WD <= 16;                                // narrow: all of the back conv's first fragments are requested during the last 3x3 conv
  // narrow convs request all of the next conv's fragments (the last conv: of the back conv's first cout block) while the running conv
  // computes.  Wide convs request them when the wave has finished its own groups, in front of the barrier that ends the conv instead
  // of behind it (A is dead there: no register cost, and the wave waits at the barrier anyway).  Requesting a part of them earlier
  // (6 of 9 chunks at wd 32, 9 or 18 of 18 at wd 64) fits the registers but measured slower: see DESIGN.md section 8 item 1.
  constexpr int NPRE = WD <= 16 ? NCH : 0;                       // chunks requested at the start of the running conv
  constexpr int NPREB = PREB ? NCHB : 0;
  constexpr bool RESW = COMPACT && WD >= 32;                     // compact walk of a swizzled map: the XOR term is re-formed per group
  constexpr int CPL = CP >= 4 ? CP / 4 : 1;                      // wide: K chunks per tap (a chunk lies inside one tap, the lane's piece is 4 h + g)
  constexpr int SWM = WD == 64 ? 0x70 : 0x30;                    // csp_psw(pix) << 4 = (pix * PS >> 3) & SWM
  bf16x8 AB[NCHB];
  f32x4 biasB = f32x4{0.f, 0.f, 0.f, 0.f};
  const int bgst = a.pool_gst, bgv = wave / (CSP_NW / bgst), obst = CSP_NW / bgst, ob0 = wave % obst;
  {
    const int gv = gvm, gst = gstm;
    const int cch = nbv * 16 + 4 * g;                            // this lane's first output channel
    const int slot0 = (MODE == 0 ? 3 : 2) * WD;                  // concat offset of the first bottleneck output
    // one 3x3 conv.  The last one is a copy of its own (LAST is a type, not a flag): what it requests for the back conv is then defined
    // after the loop over the others, not carried through it in registers that the wide convs do not have
    auto conv3 = [&](const int j, auto LAST) __attribute__((always_inline)) {
      const char* in = (j & 1) ? Tb : Pb;
      char* out = (j & 1) ? Pb : Tb;
      // narrow convs: the next conv's fragments are requested now and land while this conv computes
      bf16x8 An[NPRE > 0 ? NPRE : 1];
      f32x4 biasn = bias;
      constexpr bool more = !decltype(LAST)::value;
      if constexpr (more) {
#pragma unroll
        for (int kc = 0; kc < NPRE; ++kc) An[kc] = *(const bf16x8*)(a.mid[j + 1] + ((size_t)(kc * NB + nbv) * 64 + lane) * 16);
        biasn = *(const f32x4*)(a.mid_bias[j + 1] + nbv * 16 + 4 * g);
      } else if (ob0 < a.nbo) {
#pragma unroll
        for (int kc = 0; kc < NPREB; ++kc)
          if (kc < a.nchb) AB[kc] = *(const bf16x8*)(a.back + ((size_t)(kc * a.nbo + ob0) * 64 + lane) * 16);
        biasB = *(const f32x4*)(a.back_bias + ob0 * 16 + 4 * g);
      }
      const int lo = (j + 1) * a.RW + (j + 1), hi = (a.RH - j - 2) * a.RW + (a.RW - j - 1);
      const int wj = a.RW - 2 * j - 2, npx = (a.RH - 2 * j - 2) * wj;   // the output rectangle: rows / columns j + 1 .. of the region
      const int ng = COMPACT ? (npx + 15) >> 4 : (hi - lo + 15) >> 4;
      const FastDiv fdw = a.fd_cw[j];
      // pixel group -> this lane's region pixel.  Compact: the group's pixels are idx = 16 grp + r of the rectangle, row-major; lanes past
      // the end of the last group take the last pixel (their LDS reads stay inside the rectangle) and store nothing.  Linear: lo + idx,
      // liveness is finish's q < hi.
      auto gpx = [&](int grp, bool& lv) __attribute__((always_inline)) {
        const int idx = grp * 16 + r;
        lv = true;
        if constexpr (!COMPACT) return lo + idx;
        lv = idx < npx;
        const int ic = min(idx, npx - 1);
        const int row = (int)fdiv((uint32_t)ic, fdw);
        return lo + row * a.RW + (ic - row * wj);
      };
      const bool second = j & 1;
      const bool tocat = second && (j >> 1) + 1 < a.nbtl;       // the last bottleneck's output is read from P by the back conv
      // zero outside the image: only where a later conv reads it as padding, and only on tiles whose region crosses the image border
      // (the last conv's rectangle is the tile itself, inside the image; the linear walk's outside pixels there are wrap-around columns)
      const bool zchk = !inner && more;
      int boff[NCH];                                             // this lane's byte offset of chunk kc's piece relative to its pixel's row
#pragma unroll
      for (int kc = 0; kc < NCH; ++kc) {
        const int p = kc * 4 + g;
        int tap = p / CP, cp = p - tap * CP;
        if (tap >= 9) { tap = 4; cp = 0; }                       // padded piece: weights are zero, read something finite
        const int toff = (tap / 3 - 1) * a.RW + (tap % 3 - 1);
        // linear walk: pixel = lo + 16 k + r, its swizzle is known here.  Compact walk: q mod 16 differs from group to group, so a swizzled
        // map (wd 32 / 64) gets the XOR term per group (bsw below); wd <= 16 has none and boff stays the whole offset
        boff[kc] = toff * PS + ((RESW ? cp : cp ^ csp_psw<WD>(lo + r + toff)) << 4);
      }
      // RESW: byte offset of chunk tap * CPL + h of pixel q.  X = (q + toff) * PS + 16 g has the tap pixel's index above bit 6 (wd 64) /
      // bit 5 (wd 32), so its swizzle is a shift and a mask of X: 3 VALU per tap and one per further chunk, once per group
      auto bsw = [&](int q, int tap) __attribute__((always_inline)) {
        const int X = q * PS + boff[tap * CPL];
        return X ^ ((X >> 3) & SWM);
      };
      // cc = the lane's first output channel, live = false: a lane that holds no pixel of its own (paired form without a second group)
      auto finish = [&](int q, f32x4 acc, int cc, bool live) __attribute__((always_inline)) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[jj] = csp_act(acc[jj], a.act);
        if (live && q < hi && cc < WD) {
          char* po = out + pt_at(q, cc);
          if (second && a.shortcut) acc += lds_load4(po);       // x + cv2(cv1(x)): `out` still holds the bottleneck's input at this pixel
          int go = 0, ct = -1;
          if (zchk || tocat) region_px(q, go, ct);
          if (zchk && go == MGDT_OOB) acc = f32x4{0.f, 0.f, 0.f, 0.f};
          lds_store4(po, acc);
          if (tocat && ct >= 0) lds_store4(catb + cat_at(ct, slot0 + (j >> 1) * WD + cc), acc);
        }
      };
      for (int grp = gv; grp < ng; grp += 2 * gst) {             // two pixel groups per step: two independent accumulator chains
        const bool hasb = grp + gst < ng;                        // wave-uniform
        bool lva, lvb;
        const int qa = gpx(grp, lva);
        const int qb = gpx(hasb ? grp + gst : grp, lvb);
        f32x4 acca = bias, accb = bias;
        if constexpr (RESW) {
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const int oa = bsw(qa, tap), ob = bsw(qb, tap);
#pragma unroll
            for (int h = 0; h < CPL; ++h) {
              acca = mma(A[tap * CPL + h], *(const bf16x8*)(in + (oa ^ (h << 6))), acca);
              accb = mma(A[tap * CPL + h], *(const bf16x8*)(in + (ob ^ (h << 6))), accb);
            }
          }
        } else {
          const char* pa = in + qa * PS;
          const char* pb = in + qb * PS;
#pragma unroll
          for (int kc = 0; kc < NCH; ++kc) {
            acca = mma(A[kc], *(const bf16x8*)(pa + boff[kc]), acca);
            accb = mma(A[kc], *(const bf16x8*)(pb + boff[kc]), accb);
          }
        }
        if constexpr (PAIR) {
          finish(lane < 32 ? qa : qb, csp_merge(acca, accb), 4 * (g & 1), lane < 32 ? lva : hasb && lvb);   // one epilogue for both groups, every lane live
        } else {
          finish(qa, acca, cch, lva);
          if (hasb) finish(qb, accb, cch, lvb);
        }
      }
      // this wave's groups are done and A is dead: what was not requested ahead is requested here and lands while the wave waits for the
      // others at the barrier
      if constexpr (more) {
#pragma unroll
        for (int kc = 0; kc < NPRE; ++kc) A[kc] = An[kc];
#pragma unroll
        for (int kc = NPRE; kc < NCH; ++kc) A[kc] = *(const bf16x8*)(a.mid[j + 1] + ((size_t)(kc * NB + nbv) * 64 + lane) * 16);
        bias = biasn;
      } else if (ob0 < a.nbo) {
#pragma unroll
        for (int kc = NPREB; kc < NCHB; ++kc)
          if (kc < a.nchb) AB[kc] = *(const bf16x8*)(a.back + ((size_t)(kc * a.nbo + ob0) * 64 + lane) * 16);
      }
      __syncthreads();
      if (j == 0) stamp(4);
    };
    for (int j = 0; j + 1 < 2 * a.nbtl; ++j) conv3(j, std::false_type{});
    conv3(2 * a.nbtl - 1, std::true_type{});
  }
  stamp(5);

  // ================================================================ back: 1x1 conv over the concat, store, per-tile channel sums
  {
    const int tg = (TP + 15) >> 4;
    // K pieces [0, nsl) come from the concat buffer, [nsl, nsl + CP) (the last bottleneck's output) from P at the tile pixel's region
    // index; a lane's pixel is t = 16 grp + r, so its concat swizzle (t >> csh) & cmsk = (r >> csh) & cmsk is fixed
    const int nsl = a.catS >> 3, csw = (r >> a.csh) & a.cmsk;
    int koff[NCHB];
    bool kinp[NCHB];
#pragma unroll
    for (int kc = 0; kc < NCHB; ++kc) {
      const int p = kc * 4 + g;
      kinp[kc] = p >= nsl && p < nsl + CP;
      koff[kc] = kinp[kc] ? p - nsl : ((p < nsl ? p : 0) ^ csw) << 4;   // padded piece (p * 8 >= catC): zero weights, finite data
    }
    // few cout blocks (< 8): the waves that share a block split the tile's pixel groups; their partial sums go to separate pool slots
    const int gst = bgst, gv = bgv;
    bf16x8 ABn[PREB ? 1 : NCHB];                                 // wide blocks: the next cout block's fragments land during this one's MFMAs
    f32x4 biasBn = biasB;                                        // AB / biasB of cout block ob0: requested in the last 3x3 conv
    for (int ob = ob0; ob < a.nbo; ob += obst) {
      if (PREB && ob != ob0) {
#pragma unroll
        for (int kc = 0; kc < NCHB; ++kc)
          if (kc < a.nchb) AB[kc] = *(const bf16x8*)(a.back + ((size_t)(kc * a.nbo + ob) * 64 + lane) * 16);
        biasB = *(const f32x4*)(a.back_bias + ob * 16 + 4 * g);
      }
      if (!PREB && ob + obst < a.nbo) {
#pragma unroll
        for (int kc = 0; kc < NCHB; ++kc)
          if (kc < a.nchb) ABn[kc] = *(const bf16x8*)(a.back + ((size_t)(kc * a.nbo + ob + obst) * 64 + lane) * 16);
        biasBn = *(const f32x4*)(a.back_bias + (ob + obst) * 16 + 4 * g);
      }
      const int co = ob * 16 + 4 * g;
      const int dead = co >= a.Cout ? MGDT_OOB : 0;
      f32x4 psum = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int grp = gv; grp < tg; grp += gst) {
        const int t = grp * 16 + r;
        const int tc = min(t, TP - 1);                           // lanes past the tile: any in-tile pixel (their output is dropped)
        const int cy = (int)fdiv((uint32_t)tc, a.fd_tw), cx = tc - cy * a.TW;
        const int tq = (cy + a.halo) * a.RW + cx + a.halo;       // the pixel's index in the region (P)
        const int yo = t < TP ? n * a.ysn + (ty0 + cy) * a.ysh + (tx0 + cx) * a.ysw : MGDT_OOB;
        const char* pc = catb + t * a.CS;
        const char* pp = Pb + tq * PS;
        const int psw = csp_psw<WD>(tq);
        f32x4 acc = biasB;
#pragma unroll
        for (int kc = 0; kc < NCHB; ++kc)
          if (kc < a.nchb) acc = mma(AB[kc], *(const bf16x8*)(kinp[kc] ? pp + ((koff[kc] ^ psw) << 4) : pc + koff[kc]), acc);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[jj] = (float)(bf16)csp_act(acc[jj], a.act);
        bstore4<bf16>(yrs, (uint32_t)(yo | dead) + (uint32_t)(co * 2), acc);
        if (t < TP) psum += acc;
      }
      if (a.pool) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) psum[jj] += __shfl_xor(psum[jj], m, 64);
        if (r == 0 && co < a.Cout) {
          *(f32x4*)(a.pool + (((size_t)n * tpi + trem) * gst + gv) * a.Cout + co) = psum;
        }
      }
      if (!PREB && ob + obst < a.nbo) {
#pragma unroll
        for (int kc = 0; kc < NCHB; ++kc) AB[kc] = ABn[kc];
        biasB = biasBn;
      }
    }
  }
  stamp(6);
}

// ------------------------------------------------------------------------------------------------ host side
struct CspGeom { int TH, TW, halo, RH, RW, RPA, TPA, CS, tiles_x, tiles_y; size_t lds; };

// concat buffer: catC - wd channels per pixel (the last bottleneck output is read from P), no padding; the 16-byte slot index is XORed
// with (t >> csh) & cmsk, the form that leaves the back conv's ds_read_b128 lane groups conflict-free for the row's slot count
static void csp_cat_swizzle(int slots, int* cmsk, int* csh) {
  if (slots % 16 == 0) { *cmsk = 15; *csh = 0; }
  else if (slots % 8 == 0) { *cmsk = 7; *csh = 0; }
  else if (slots % 4 == 0) { *cmsk = 3; *csh = 1; }
  else { *cmsk = 0; *csh = 0; }                                           // odd (or 2 mod 4) slot counts: within 25 % of conflict-free unswizzled
}

static bool csp_geometry(int mode, int H, int W, int wd, int nbtl, int catC, size_t extra, int th, int tw, CspGeom* g) {
  g->TH = th; g->TW = tw; g->halo = 2 * nbtl;
  g->RH = th + 2 * g->halo; g->RW = tw + 2 * g->halo;
  const int RP = g->RH * g->RW;
  // the last pixel group of a 3x3 conv ends < hi + 15 and its taps reach RW + 1 further; hi <= RP - RW - 1: reads stay below RP + 15
  g->RPA = ((RP + 15 + 15) / 16) * 16;
  g->TPA = ((th * tw + 15) / 16) * 16;
  g->CS = (catC - wd) * 2;
  g->tiles_x = W / tw; g->tiles_y = H / th;
  g->lds = 2 * (size_t)g->RPA * (wd * 2) + (size_t)g->TPA * g->CS + extra;
  (void)mode;
  return g->lds <= 156 * 1024;
}

static int csp_chain_nbk(int wd) { return wd >= 16 ? wd / 16 : 1; }
static int csp_pool_gst(int cout) { const int nbo = (cout + 15) / 16; return (nbo < CSP_NW && CSP_NW % nbo == 0) ? CSP_NW / nbo : 1; }

// mode 2 (CSP_C3, the C3 block of the YOLOv5 graphs): csp_c3.hip
int csp_c3_supported(int cin, int cout, int wd, int nbtl, int h, int w, int dtype);
int csp_c3_tiles(int n, int cin, int cout, int wd, int nbtl, int h, int w, int* geom8);
int csp_c3_fwd(const mgdt_view* x, const void* const* mid, const float* const* mid_bias, int nbtl, int shortcut, const void* back, const float* back_bias,
               int wd, const mgdt_view* y, mgdt_stream s);

/* supported configurations of the fused block: bf16, wd in {8,16,32,64}, n in {1,2}; MSPA: even H, W; C2f: Cin % 32 == 0, Cin <= 256 */
extern "C" int mgdt_csp_block_supported(int mode, int cin, int cout, int wd, int nbtl, int h, int w, int dtype) {
  if (mode == 2) return csp_c3_supported(cin, cout, wd, nbtl, h, w, dtype);
  if (mode != 0 && mode != 1) return 0;
  if (dtype != MGDT_BF16 || (wd != 8 && wd != 16 && wd != 32 && wd != 64) || nbtl < 1 || nbtl > 2 || cout % 4) return 0;
  const int catC = (mode == 0 ? 3 : 2) * wd + nbtl * wd;
  if (catC > 256 || catC % 8) return 0;
  if (mode == 0) {
    if (cin != 4 * wd || h % 2 || w % 2 || h < 4 || w < 4) return 0;
  } else {
    if (cin != 2 * wd || wd < 16) return 0;
  }
  return 1;
}

// residency: wd <= 32 builds fit two workgroups per CU in registers (<= 128 VGPRs); then a tile whose LDS keeps it at one workgroup per
// CU pays CSP_1WG_COST (nothing overlaps its barriers and table / front latency; with batches in flight it also locks other kernels out
// of the CU).  wd = 64 needs > 128 VGPRs: one workgroup per CU whatever its LDS.
constexpr size_t CSP_LDS_2WG = 80 * 1024;
constexpr double CSP_1WG_COST = 2.0;

static bool csp_pick_tile(int mode, int H, int W, int N, int wd, int nbtl, int catC, size_t extra, CspGeom* best) {
  int fth = 0, ftw = 0;
  knob_pair("MGDT_CSP_TILE", &fth, &ftw);       // experiment knob "th,tw", read per call (not part of the ABI)
  const int qh = mode == 0 ? H / 2 : H, qw = mode == 0 ? W / 2 : W;     // MSPA: a tile must lie inside one adaptive_avg_pool2d(2) bin
  double best_cost = 1e30;
  bool found = false;
  for (int th = 2; th <= std::min(qh, 32); ++th) {
    if (qh % th) continue;
    for (int tw = 2; tw <= std::min(qw, 32); ++tw) {
      if (qw % tw) continue;
      if (fth && (th != fth || tw != ftw)) continue;
      CspGeom g;
      if (!csp_geometry(mode, H, W, wd, nbtl, catC, extra, th, tw, &g)) continue;
      const double wgs = (double)N * g.tiles_x * g.tiles_y;
      const double ratio = (double)(g.RH * g.RW) / (th * tw);
      const double fill = (double)(th * tw) / g.TPA;              // lanes of the tile's last pixel group that do work
      double cost = ratio / fill;
      if (wgs < 256) cost *= 256.0 / wgs;                        // fewer workgroups than CUs: the chip is not filled (measured: 128 big tiles beat 512 small ones at 20x20)
      if (wd <= 32 && g.lds > CSP_LDS_2WG) cost *= CSP_1WG_COST;
      if (cost < best_cost) { best_cost = cost; *best = g; found = true; }
    }
  }
  return found;
}

/* x: N x H x W x Cin view, y: N x H x W x Cout view (bf16 NHWC).  front: MSPA - the blob of mgdt_pw_chain_pack (3 convs); C2f - the
 * mgdt_conv_pack panel of cv1 (+ front_bias).  mid[2*nbtl] / mid_bias: mgdt_conv_pack panels of the bottlenecks' 3x3 convs in
 * execution order.  back / back_bias: the 1x1 conv over the concat.  pool: NULL or fp32 [N][slots][Cout] per-tile channel sums of y
 * (slots and the tile grid: mgdt_csp_block_tiles). */
extern "C" int mgdt_csp_block_tiles(int mode, int n, int cin, int cout, int wd, int nbtl, int h, int w, int* geom6) {
  if (mode == 2) return csp_c3_tiles(n, cin, cout, wd, nbtl, h, w, geom6);
  if (!mgdt_csp_block_supported(mode, cin, cout, wd, nbtl, h, w, MGDT_BF16)) return 0;
  const int catC = (mode == 0 ? 3 : 2) * wd + nbtl * wd;
  const int nbk = csp_chain_nbk(wd);
  const size_t extra = mode == 0 ? (size_t)3 * ((nbk + 1) / 2) * nbk * 1024 + 3 * nbk * 16 * 4 : 0;
  CspGeom g;
  if (!csp_pick_tile(mode, h, w, n, wd, nbtl, catC, extra, &g)) return 0;
  if (geom6) {
    geom6[0] = g.TH; geom6[1] = g.TW; geom6[2] = g.RH; geom6[3] = g.RW; geom6[4] = (int)g.lds; geom6[5] = n * g.tiles_x * g.tiles_y;
    geom6[6] = g.tiles_x; geom6[7] = g.tiles_y;
  }
  return g.tiles_x * g.tiles_y * csp_pool_gst(cout);      // pool slots per image
}

extern "C" int mgdt_csp_block_fwd(int mode, const mgdt_view* x, const void* front, const float* front_bias, const void* const* mid,
                                  const float* const* mid_bias, int nbtl, int shortcut, const void* back, const float* back_bias, int wd, int act,
                                  const mgdt_view* y, float* pool, int dtype, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(y) || (mode == 0 && !front) || !mid || !mid_bias || !back || !back_bias) MGDT_FAIL(MGDT_BAD_ARG, "csp_block: null/empty argument");
  if (!mgdt_csp_block_supported(mode, x->c, y->c, wd, nbtl, x->h, x->w, dtype))
    MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block: mode=%d cin=%d cout=%d wd=%d n=%d %dx%d dtype=%d not covered", mode, x->c, y->c, wd, nbtl, x->h, x->w, dtype);
  if (x->n != y->n || x->h != y->h || x->w != y->w) MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block: x and y must have one spatial size");
  if (act != MGDT_ACT_SILU) MGDT_FAIL(MGDT_BAD_ARG, "csp_block: activation %d (only SiLU, the blocks' default, is built)", act);
  for (int j = 0; j < 2 * nbtl; ++j)
    if (!mid[j] || !mid_bias[j]) MGDT_FAIL(MGDT_BAD_ARG, "csp_block: missing conv panel %d", j);
  if (mode == 2) return csp_c3_fwd(x, mid, mid_bias, nbtl, shortcut, back, back_bias, wd, y, s);
  CspArgs a;
  memset(&a, 0, sizeof(a));
  const ViewPolicy pol = {4, true, 0, 0, false};      // 8-byte pieces of NHWC bf16
  const char* yp = nullptr;
  if (!bind_view(x, 2, pol, &a.x, &a.xsn, &a.xsh, &a.xsw, &a.x_bytes) || !bind_view(y, 2, pol, &yp, &a.ysn, &a.ysh, &a.ysw, &a.y_bytes))
    MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block: views must be aligned NHWC (sc == 1) and span < 2 GiB");
  a.y = (char*)yp;
  a.front = (const char*)front; a.front_bias = front_bias;
  for (int j = 0; j < 2 * nbtl; ++j) { a.mid[j] = (const char*)mid[j]; a.mid_bias[j] = mid_bias[j]; }
  a.back = (const char*)back; a.back_bias = back_bias; a.pool = pool;
  a.N = x->n; a.H = x->h; a.W = x->w; a.Cin = x->c; a.Cout = y->c; a.wd = wd; a.nbtl = nbtl; a.shortcut = shortcut; a.act = act;
  a.catC = (mode == 0 ? 3 : 2) * wd + nbtl * wd;
  a.nchb = (a.catC / 8 + 3) / 4; a.nbo = (a.Cout + 15) / 16; a.pool_gst = csp_pool_gst(a.Cout);
  const int nbk = csp_chain_nbk(wd);
  a.chain_words = mode == 0 ? 3 * ((nbk + 1) / 2) * nbk * 64 : 0;
  const size_t extra = mode == 0 ? (size_t)a.chain_words * 16 + 3 * nbk * 16 * 4 : 0;
  CspGeom g;
  if (!csp_pick_tile(mode, a.H, a.W, a.N, wd, nbtl, a.catC, extra, &g)) MGDT_FAIL(MGDT_BAD_SHAPE, "csp_block: no tile fits %dx%d wd=%d n=%d", a.H, a.W, wd, nbtl);
  a.TH = g.TH; a.TW = g.TW; a.halo = g.halo; a.RH = g.RH; a.RW = g.RW; a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y;
  a.RPA = g.RPA; a.TPA = g.TPA; a.CS = g.CS;
  a.catS = a.catC - wd;
  csp_cat_swizzle(a.catS / 8, &a.cmsk, &a.csh);
  a.total_tiles = a.N * g.tiles_x * g.tiles_y;
  a.fd_rw = make_fastdiv((uint32_t)g.RW); a.fd_tw = make_fastdiv((uint32_t)g.TW); a.fd_tx = make_fastdiv((uint32_t)g.tiles_x);
  a.fd_tpi = make_fastdiv((uint32_t)(g.tiles_x * g.tiles_y));
  for (int j = 0; j < 2 * nbtl; ++j) a.fd_cw[j] = make_fastdiv((uint32_t)(g.RW - 2 * j - 2));
  a.per_xcd = cdiv(a.total_tiles, 8);
  const int grid = 8 * a.per_xcd;
  hipStream_t st = (hipStream_t)s;
  static StampBuf stamps;            // MGDT_CSP_DBG=1: per-workgroup phase stamps, printed after the launch (debug only)
  const bool dbg = knob_set("MGDT_CSP_DBG");
  if (dbg && !stamps.ensure((size_t)a.total_tiles * 8)) MGDT_FAIL(MGDT_WORKSPACE, "csp_block: no memory for the MGDT_CSP_DBG stamps");
  a.dbg = dbg ? stamps.p : nullptr;
  // experiment knob, read per call (not part of the ABI): MGDT_CSP_PAIR=0 = the unpaired wd = 8 form
  const bool pair = knob_unless0("MGDT_CSP_PAIR");
  // likewise MGDT_CSP_COMPACT=0 = the linear pixel walk of the 3x3 convs (same MFMAs per needed pixel: bit-identical outputs)
  const bool compact = knob_unless0("MGDT_CSP_COMPACT");
#define CSP_LAUNCH(...)                                                                                              \
  do {                                                                                                                      \
    if (int rc_ = lds_optin<csp_block_kernel<__VA_ARGS__>>("csp_block")) return rc_;                                        \
    csp_block_kernel<__VA_ARGS__><<<grid, CSP_THREADS, g.lds, st>>>(a);                                                      \
  } while (0)
#define CSP_WALK(...) do { if (compact) CSP_LAUNCH(__VA_ARGS__, true); else CSP_LAUNCH(__VA_ARGS__, false); } while (0)
  if (mode == 0) {
    switch (wd) { case 8: if (pair) CSP_WALK(8, 0, true); else CSP_WALK(8, 0, false); break; case 16: CSP_WALK(16, 0, false); break; case 32: CSP_WALK(32, 0, false); break; default: CSP_WALK(64, 0, false); break; }
  } else {
    switch (wd) { case 16: CSP_WALK(16, 1, false); break; case 32: CSP_WALK(32, 1, false); break; default: CSP_WALK(64, 1, false); break; }
  }
#undef CSP_WALK
#undef CSP_LAUNCH
  MGDT_CHECK_LAUNCH("csp_block_fwd");
  if (a.dbg) {
    const std::vector<unsigned long long> h = stamps.read((size_t)a.total_tiles * 8, st);
    unsigned long long t0 = ~0ull, t1 = 0;
    double ph[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < a.total_tiles; ++i) {
      t0 = std::min(t0, h[(size_t)i * 8]); t1 = std::max(t1, h[(size_t)i * 8 + 6]);
      for (int k = 0; k < 6; ++k) ph[k] += (double)(h[(size_t)i * 8 + k + 1] - h[(size_t)i * 8 + k]);
    }
    const double nw = a.total_tiles;
    fprintf(stderr, "csp_block mode %d wd %d n %d %dx%d tile %dx%d (%d wgs, lds %zu): span %.1f us; avg per WG (us): tables %.2f front %.2f sync %.2f conv0 %.2f "
                    "other convs %.2f back %.2f\n", mode, wd, nbtl, a.H, a.W, g.TH, g.TW, a.total_tiles, g.lds, (t1 - t0) * 0.01, ph[0] / nw * 0.01,
            ph[1] / nw * 0.01, ph[2] / nw * 0.01, ph[3] / nw * 0.01, ph[4] / nw * 0.01, ph[5] / nw * 0.01);
  }
  return MGDT_OK;
}
