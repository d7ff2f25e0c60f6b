// The two stride-2 3x3 convolutions at the top of every YOLOv8 graph (layers 0 and 1: 3 -> 16 -> 32 channels at scale n) in ONE launch,
// bf16 inference path.  Reference: nn/modules/conv.py:25-42 (Conv = conv + BN + SiLU), models/v8/*.yaml rows 0-1; the uint8 / 255
// of the predictor's preprocess (yolo/engine/predictor.py:128-129) is folded into the loader.
//
// Why: unfused, layer 0 reads the image with 27 scattered 2-byte loads per output pixel and does 432 VALU FMAs for it (the stem kernel is
// VALU- and load-issue-bound at ~1.5 TB/s), writes 105 MB (B=32, 640^2) that layer 1 immediately reads back.  Here the unit of work is an
// 8 x 16 tile of layer 1's output: the 35 x 80 input patch (3 planes) comes in with 16-byte row loads, layer 0 runs on MFMA straight out
// of LDS (K = 9 (plane, row) combos x 4 consecutive columns, the first column's weight is zero so that every fragment piece is an aligned
// 4-byte LDS word: no packing instructions), its 17 x 33 x 16 output stays in LDS as the NHWC map layer 1 (an ordinary implicit GEMM,
// K = 144) reads; only layer 1's output goes to HBM.
//
// The kernel is persistent: the grid is min(tiles, 3 workgroups per compute unit of the device) and a workgroup walks its tiles.  Weight
// fragments, biases, the loader's per-thread (row, column, LDS offset), the LDS addresses of layer 0's fragment reads and of layer 1's
// taps are set up once per workgroup and stay in registers (no scratch); on the 16-byte path the next tile's patch is requested before
// layer 0 of the current tile and stored to LDS after it.  Per tile there are two barriers; a workgroup never waits for another one, so
// the grid size (MGDT_STEM_WGS caps it for experiments) changes speed only, never values.  MGDT_STEM_DBG=1 launches the diagnostic
// instantiation that sums wall-clock time per phase and prints the means.
#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>

#include "conv_igemm_kernel.h"

struct StemArgs {
  const void* x; long xsn, xsc, xsh, xsw;     // element strides of the NCHW image
  const char* w0; const float* b0;            // layer 0: [2 chunks][64 lanes][16 B] bf16 fragments (see mgdt_stem2_pack) + bias[16]
  const char* w1; const float* b1;            // layer 1: mgdt_conv_pack(16, 32, 3, bf16) panel + bias[32]
  char* y; int ysn, ysh, ysw; uint32_t y_bytes;
  int N, H, W, H0, W0, H1, W1, tiles_x, tiles_y, total, per_xcd, fast;
  unsigned long long* dbg;                    // MGDT_STEM_DBG: 8 words per workgroup (tiles walked + 7 phase sums, 10 ns units)
};

constexpr int ST_TH = 8, ST_TW = 16;                 // layer-1 output tile
constexpr int ST_R0H = 2 * ST_TH + 1, ST_R0W = 2 * ST_TW + 1;      // layer-0 region 17 x 33
constexpr int ST_XH = 2 * ST_R0H + 1, ST_XWV = 80, ST_XW = 88;     // input patch 35 rows x 80 columns (row pitch 88 elements)
constexpr int ST_PS = 48;                            // layer-0 map: 16 channels (32 B) + 16 B pad per pixel
constexpr int ST_RP0 = ST_R0H * ST_R0W, ST_RP0A = (ST_RP0 + 15) / 16 * 16;
constexpr int ST_NI = 3 * ST_XH * (ST_XWV / 8), ST_NU = (ST_NI + 255) / 256;     // fast loader: 16-byte vectors per patch, per thread
constexpr int ST_G0 = ST_RP0A / 16 / 4;              // layer-0 pixel groups per wave
constexpr int ST_WGS_PER_CU = 3;                     // what __launch_bounds__(256, 3) and the LDS below allow; the grid is sized from it
constexpr int ST_LDS_BYTES = 3 * ST_XH * ST_XW * 2 + ST_RP0A * ST_PS + 256 * 4;   // X + Y0 + the uint8 table (the largest instantiation)
static_assert(ST_RP0A / 16 % 4 == 0, "every wave takes the same number of layer-0 groups");
static_assert(ST_WGS_PER_CU * ST_LDS_BYTES <= 160 * 1024, "three workgroups share a CU's LDS");

__device__ __forceinline__ float stem_silu(float v) { return v * fast_sigmoid(v); }

template <typename TX, bool DBG>
__global__ __launch_bounds__(256, ST_WGS_PER_CU) void stem2_kernel(const StemArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 X[3][ST_XH][ST_XW];
  __shared__ __attribute__((aligned(16))) char Y0[ST_RP0A * ST_PS];
  __shared__ float lut[std::is_same<TX, uint8_t>::value ? 256 : 1];
  typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  // Tiles: XCD k (workgroups with blockIdx % 8 == k) takes the contiguous range [k * per_xcd, (k + 1) * per_xcd) (halo rows shared in its L2); its wx
  // workgroups walk it interleaved, so the workgroups that run at the same time work on adjacent tiles.  A workgroup depends on no other one: any
  // grid size computes the same values.
  const int v = blockIdx.x, G = gridDim.x;
  const int xcd = v & 7, wx = (G - xcd + 7) >> 3;
  const int tend = min((xcd + 1) * a.per_xcd, a.total);
  int tlin = xcd * a.per_xcd + (v >> 3);
  if (tlin >= tend) return;
  const int tpi = a.tiles_x * a.tiles_y;
  struct Tile { int n, ty0, tx0; };
  auto tile_of = [&](int t) __attribute__((always_inline)) {
    const int n = t / tpi, trem = t - n * tpi, ty = trem / a.tiles_x;
    return Tile{n, ty * ST_TH, (trem - ty * a.tiles_x) * ST_TW};
  };
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
  auto stamp = [&](int k) __attribute__((always_inline)) {     // adds the time since the previous stamp to phase k (diagnostic instantiation only)
    if constexpr (DBG) {
      const unsigned long long t = __builtin_amdgcn_s_memrealtime();
      ph[k] += t - tlast;
      tlast = t;
    }
  };
  if constexpr (DBG) tlast = __builtin_amdgcn_s_memrealtime();

  // ================= once per workgroup: everything that does not depend on the tile
  // layer-1 weights: 5 K chunks x 2 cout blocks
  bf16x8 A1[5][2];
#pragma unroll
  for (int kc = 0; kc < 5; ++kc)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) A1[kc][nb] = *(const bf16x8*)(a.w1 + ((size_t)(kc * 2 + nb) * 64 + lane) * 16);
  const bf16x8 A0a = *(const bf16x8*)(a.w0 + (size_t)lane * 16), A0b = *(const bf16x8*)(a.w0 + (size_t)(64 + lane) * 16);
  const f32x4 bias0 = *(const f32x4*)(a.b0 + 4 * g);
  f32x4 bias1[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) bias1[nb] = *(const f32x4*)(a.b1 + nb * 16 + 4 * g);
  if constexpr (std::is_same<TX, uint8_t>::value) {
    lut[tid] = __fdiv_rn((float)tid, 255.f);     // the preprocess division, exact
    __syncthreads();
  }
  // fast loader: vector i = tid + u * 256 of the patch is (plane, row, 8-column segment); per tile only the tile origin is added and the bounds tested
  int lrow[ST_NU], lcol[ST_NU], lofs[ST_NU];
  long lpl[ST_NU];
  if constexpr (std::is_same<TX, bf16>::value) {
#pragma unroll
    for (int u = 0; u < ST_NU; ++u) {
      const int i = min(tid + u * 256, ST_NI - 1);
      const int pl = i / (ST_XH * (ST_XWV / 8)), rem = i - pl * (ST_XH * (ST_XWV / 8));
      const int row = rem / (ST_XWV / 8), seg = rem - row * (ST_XWV / 8);
      lrow[u] = row; lcol[u] = seg * 8; lpl[u] = (long)pl * a.xsc;
      lofs[u] = ((pl * ST_XH + row) * ST_XW + seg * 8) * 2;
    }
  }
  // layer 0, group k of this wave (pixel q = (wave + 4k) * 16 + r of the 17 x 33 region): LDS byte offset of X[0][2 ry][4 + 2 rx], ry, rx in one word
  unsigned l0t[ST_G0];
#pragma unroll
  for (int k = 0; k < ST_G0; ++k) {
    const int q = (wave + 4 * k) * 16 + r;
    const int qq = q < ST_RP0 ? q : ST_RP0 - 1;
    const int ry = qq / ST_R0W, rx = qq - ry * ST_R0W;
    l0t[k] = (unsigned)((2 * ry * ST_XW + 4 + 2 * rx) * 2) | (unsigned)ry << 16 | (unsigned)rx << 24;
  }
  // ... + the (plane, ky) combo of the lane's K slots: chunk 0 holds combos 2g and 2g + 1 (< 8), chunk 1 combo 8 = (plane 2, ky 2) in g == 0 only
  const int cb = 2 * g;
  const int c0 = ((cb / 3) * ST_XH + cb % 3) * ST_XW * 2, c1 = (((cb + 1) / 3) * ST_XH + (cb + 1) % 3) * ST_XW * 2, c2 = (2 * ST_XH + 2) * ST_XW * 2;
  const int y0st = (wave * 16 + r) * ST_PS + 8 * g;            // Y0 store offset of group 0; group k: + k * 64 * ST_PS
  // layer 1: taps at region pixel (2 oy + ky, 2 r + kx); piece kc of the lane = (tap, channel half)
  int boff[5];
#pragma unroll
  for (int kc = 0; kc < 5; ++kc) {
    const int p = kc * 4 + g;
    int tap = p >> 1, cp = p & 1;
    if (tap >= 9) { tap = 4; cp = 0; }                        // padded piece: zero weights
    boff[kc] = ((2 * wave) * ST_R0W + 2 * r) * ST_PS + ((tap / 3) * ST_R0W + tap % 3) * ST_PS + cp * 16;
  }
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, a.y_bytes, 0x00020000);
  const int yst = wave * a.ysh + r * a.ysw + 8 * g;            // lane's output offset inside a tile (row wave, pixel r, channels 4g..)
  char* const Xb = (char*)&X[0][0][0];

  // ================= the patch of a tile: rows 4*ty0-3 .. +34, columns 4*tx0-8 .. +79 of the three planes, zero outside the image
  // Fast path (bf16 image, rows contiguous and 16-byte aligned, W % 8 == 0: whole 8-element vectors are inside or outside): all of a thread's 16-byte
  // requests go out before anything waits for them (clamped address, zeroed when outside the image), and they go out ONE TILE AHEAD: request() for
  // tile i + 1 is issued before layer 0 of tile i, commit() writes the registers to X after the barrier that ends layer 0 (layer 1 reads only Y0).
  uint4 val[ST_NU];
  unsigned inb = 0;
  auto request = [&](const Tile& t) __attribute__((always_inline)) {
    if constexpr (std::is_same<TX, bf16>::value) {
      const int iy0 = 4 * t.ty0 - 3, ix0 = 4 * t.tx0 - 8;
      const bf16* xb = (const bf16*)a.x + (long)t.n * a.xsn;
      inb = 0;
#pragma unroll
      for (int u = 0; u < ST_NU; ++u) {
        const int iy = iy0 + lrow[u], ix = ix0 + lcol[u];
        if ((unsigned)iy < (unsigned)a.H && ix >= 0 && ix + 8 <= a.W) inb |= 1u << u;
        const int iyc = min(max(iy, 0), a.H - 1), ixc = min(max(ix, 0), a.W - 8);
        val[u] = *(const uint4*)(xb + lpl[u] + (long)iyc * a.xsh + ixc);
      }
    }
  };
  auto commit = [&]() __attribute__((always_inline)) {
    if constexpr (std::is_same<TX, bf16>::value) {
#pragma unroll
      for (int u = 0; u < ST_NU; ++u)
        if (u < ST_NU - 1 || tid < ST_NI - (ST_NU - 1) * 256) *(uint4*)(Xb + lofs[u]) = (inb >> u & 1) ? val[u] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  // Generic path (uint8 / fp32 / strided image): element by element, straight into X
  auto fill = [&](const Tile& t) __attribute__((always_inline)) {
    const int iy0 = 4 * t.ty0 - 3, ix0 = 4 * t.tx0 - 8;
    const TX* xb = (const TX*)a.x + (long)t.n * a.xsn;
    for (int i = tid; i < 3 * ST_XH * ST_XWV; i += 256) {
      const int pl = i / (ST_XH * ST_XWV), rem = i - pl * (ST_XH * ST_XWV);
      const int row = rem / ST_XWV, col = rem - row * ST_XWV;
      const int iy = iy0 + row, ix = ix0 + col;
      float val = 0.f;
      if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
        const TX e = xb[(long)pl * a.xsc + (long)iy * a.xsh + (long)ix * a.xsw];
        if constexpr (std::is_same<TX, uint8_t>::value) val = lut[e];
        else val = (float)e;
      }
      X[pl][row][col] = (bf16)val;
    }
  };
  const bool fast = std::is_same<TX, bf16>::value && a.fast;

  Tile t = tile_of(tlin);
  stamp(0);                                                    // setup
  if (fast) { request(t); commit(); }
  else fill(t);
  stamp(1);                                                    // first patch: request, wait, LDS
  // Everything requested so far (weights, biases, first patch) is complete from here on.  Without this the compiler cannot prove it for the weight registers on
  // every path into the loop and puts a vmcnt wait that also covers most of the NEXT patch's requests in front of the first MFMA of layer 0.
  __builtin_amdgcn_s_waitcnt(0x0F70);                          // vmcnt(0) alone
  int ntiles = 0;
  for (;;) {
    const int tnext = tlin + wx;
    const bool more = tnext < tend;
    Tile tn = t;
    if (more) {
      tn = tile_of(tnext);
      if (fast) request(tn);
    }
    stamp(2);                                                  // next patch requested
    __syncthreads();                                           // X holds this tile's patch; every wave is done with the previous tile's Y0
    stamp(3);

    // ---- layer 0 on the 17 x 33 region: K = 9 (plane, ky) combos x 4 columns {2x-2 (zero weight), 2x-1, 2x, 2x+1}
    {
      const int y00 = 2 * t.ty0 - 1, x00 = 2 * t.tx0 - 1;      // image coordinates of the region's first layer-0 pixel
#pragma unroll
      for (int k = 0; k < ST_G0; ++k) {
        const int qb = l0t[k] & 0xffff, ry = (l0t[k] >> 16) & 0xff, rx = l0t[k] >> 24;
        u4 f0, f1 = {0u, 0u, 0u, 0u};
        {                                                       // no branch in this loop body: the compiler issues the LDS reads of several groups together
          const char* p0 = Xb + qb + c0;
          const char* p1 = Xb + qb + c1;
          f0[0] = *(const unsigned*)p0; f0[1] = *(const unsigned*)(p0 + 4);
          f0[2] = *(const unsigned*)p1; f0[3] = *(const unsigned*)(p1 + 4);
        }
        {
          const char* p0 = Xb + qb + c2;                        // read by every lane, kept by g == 0 (the other lanes' K slots are padding: zero)
          const unsigned e0 = *(const unsigned*)p0, e1 = *(const unsigned*)(p0 + 4);
          f1[0] = g == 0 ? e0 : 0u; f1[1] = g == 0 ? e1 : 0u;
        }
        f32x4 acc = bias0;
        acc = mma(A0a, __builtin_bit_cast(bf16x8, f0), acc);
        acc = mma(A0b, __builtin_bit_cast(bf16x8, f1), acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = stem_silu(acc[j]);
        const int yy = y00 + ry, xx = x00 + rx;
        if (!((unsigned)yy < (unsigned)a.H0 && (unsigned)xx < (unsigned)a.W0)) acc = f32x4{0.f, 0.f, 0.f, 0.f};   // layer 1's zero padding
        bf16x4 o;                                               // pixels ST_RP0 .. ST_RP0A - 1 are padding of Y0 that layer 1 never reads
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16)acc[j];
        *(bf16x4*)(Y0 + y0st + k * 64 * ST_PS) = o;
      }
    }
    stamp(4);                                                  // layer 0
    __syncthreads();                                           // Y0 complete; nobody reads X any more
    stamp(5);
    if (more) {
      if (fast) commit();
      else fill(tn);
    }
    stamp(6);                                                  // next patch into X (fast path: requested before layer 0, so no wait is expected here)

    // ---- layer 1: output row oy = wave, wave + 4 of the tile = one 16-pixel group each (lane r = ox)
    {
      const int ybase = t.n * a.ysn + t.ty0 * a.ysh + t.tx0 * a.ysw + yst;
      const int gx = t.tx0 + r;
#pragma unroll
      for (int h = 0; h < ST_TH / 4; ++h) {
        f32x4 acc[2] = {bias1[0], bias1[1]};
#pragma unroll
        for (int kc = 0; kc < 5; ++kc) {
          const bf16x8 B = *(const bf16x8*)(Y0 + boff[kc] + h * 8 * ST_R0W * ST_PS);
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) acc[nb] = mma(A1[kc][nb], B, acc[nb]);
        }
        const int gy = t.ty0 + wave + 4 * h;
        const int yo = (gy < a.H1 && gx < a.W1) ? ybase + 4 * h * a.ysh : MGDT_OOB;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[nb][j] = stem_silu(acc[nb][j]);
          bstore4<bf16>(yrs, (uint32_t)yo + (uint32_t)(nb * 32), acc[nb]);
        }
      }
    }
    stamp(7);                                                  // layer 1
    ++ntiles;
    if (!more) break;
    tlin = tnext;
    t = tn;
  }
  if constexpr (DBG) {
    if (tid == 0) {
      a.dbg[(size_t)v * 8] = (unsigned long long)ntiles;
      a.dbg[(size_t)v * 8 + 1] = ph[0];
      a.dbg[(size_t)v * 8 + 2] = ph[1];
      a.dbg[(size_t)v * 8 + 3] = ph[2];
      a.dbg[(size_t)v * 8 + 4] = ph[3] + ph[5];
      a.dbg[(size_t)v * 8 + 5] = ph[4];
      a.dbg[(size_t)v * 8 + 6] = ph[6];
      a.dbg[(size_t)v * 8 + 7] = ph[7];
    }
  }
}

// layer-0 weights in fragment order: w_folded fp32 [16][3][3][3] (BN already folded) -> bf16 [2][64][8]
__global__ void stem2_pack_kernel(const float* __restrict__ w, bf16* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * 64 * 8) return;
  const int j = i & 7, lane = (i >> 3) & 63, c = i >> 9;
  const int k = c * 32 + 8 * (lane >> 4) + j, cout = lane & 15;
  const int cb = k >> 2, e = k & 3;                               // combo = plane * 3 + ky; e = column 0 (zero weight), 1..3 = kx 0..2
  float v = 0.f;
  if (cb < 9 && e >= 1) v = w[((cout * 3 + cb / 3) * 3 + cb % 3) * 3 + (e - 1)];
  out[i] = (bf16)v;
}

extern "C" size_t mgdt_stem2_packed_bytes(void) { return 2 * 64 * 16; }

/* w_folded: fp32 [16][3][3][3] with the BatchNorm scale already multiplied in (fuse_conv_and_bn's W'); packed: mgdt_stem2_packed_bytes() */
extern "C" int mgdt_stem2_pack(const float* w_folded, void* packed, mgdt_stream s) {
  if (!w_folded || !packed) MGDT_FAIL(MGDT_BAD_ARG, "stem2_pack: null pointer");
  stem2_pack_kernel<<<4, 256, 0, (hipStream_t)s>>>(w_folded, (bf16*)packed);
  MGDT_CHECK_LAUNCH("stem2_pack");
  return MGDT_OK;
}

// compute units of the current device (read once per device)
static int stem2_cu_count() {
  static std::atomic<int> cached[64];
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  if (dev < 64 && (n = cached[dev].load(std::memory_order_relaxed)) > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (dev < 64) cached[dev].store(n, std::memory_order_relaxed);
  return n;
}

// persistent grid: no more workgroups than tiles or than the chip holds at once (ST_WGS_PER_CU per compute unit); cap > 0 lowers it further
static int stem2_grid(int tiles, int cus, int cap) {
  int g = std::min(tiles, ST_WGS_PER_CU * cus);
  if (cap > 0) g = std::min(g, cap);
  return std::max(g, 1);
}

/* Debug: the launch geometry mgdt_stem2_fwd uses for an n x 3 x h x w image on a device with cu_count compute units (<= 0: the current device's):
 * out[0] = tiles, out[1] = workgroups launched, out[2] = LDS bytes per workgroup, out[3] = workgroups per compute unit the grid is sized for,
 * out[4] = compute units. */
extern "C" int mgdt_stem2_geometry(int n, int h, int w, int cu_count, int* out) {
  if (n <= 0 || h <= 0 || w <= 0 || !out) MGDT_FAIL(MGDT_BAD_ARG, "stem2_geometry: bad argument");
  if (cu_count <= 0) cu_count = stem2_cu_count();
  if (cu_count <= 0) MGDT_FAIL(MGDT_LAUNCH_FAIL, "stem2_geometry: cannot read the device's compute-unit count");
  const int H0 = (h - 1) / 2 + 1, W0 = (w - 1) / 2 + 1, H1 = (H0 - 1) / 2 + 1, W1 = (W0 - 1) / 2 + 1;
  const long tiles = (long)n * cdiv(W1, ST_TW) * cdiv(H1, ST_TH);
  if (tiles >= 0x7fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "stem2_geometry: too many tiles");
  out[0] = (int)tiles; out[1] = stem2_grid((int)tiles, cu_count, knob_stem_wgs()); out[2] = ST_LDS_BYTES; out[3] = ST_WGS_PER_CU; out[4] = cu_count;
  return MGDT_OK;
}

// Everything mgdt_stem2_fwd decides from the two views (reported by mgdt_stem2_route): the checks the launch makes before it launches, the tile
// decomposition and the loader.  Pointers are tested for alignment only.
static int stem2_plan(const mgdt_view* x, int x_dtype, const mgdt_view* y, StemArgs& a) {
  memset(&a, 0, sizeof(a));
  if (x->c != 3 || y->c != 32 || y->sc != 1 || !view_aligned(y, 4, 2)) MGDT_FAIL(MGDT_BAD_SHAPE, "stem2: x must have 3 channels, y 32 (NHWC, 8-byte aligned)");
  const int H0 = (x->h - 1) / 2 + 1, W0 = (x->w - 1) / 2 + 1, H1 = (H0 - 1) / 2 + 1, W1 = (W0 - 1) / 2 + 1;
  if (y->n != x->n || y->h != H1 || y->w != W1) MGDT_FAIL(MGDT_BAD_SHAPE, "stem2: y is %dx%dx%d, expected %dx%dx%d", y->n, y->h, y->w, x->n, H1, W1);
  // NHWC and 8-byte pieces were tested above (their own message), so only the extent can refuse here; a route query's pointer is only tested for alignment
  const char* yp = nullptr;
  if (!bind_view(y, 2, {4, true, 0, 0, true}, &yp, &a.ysn, &a.ysh, &a.ysw, &a.y_bytes)) MGDT_FAIL(MGDT_BAD_SHAPE, "stem2: y spans >= 2 GiB");
  a.x = x->p; a.xsn = x->sn; a.xsc = x->sc; a.xsh = x->sh; a.xsw = x->sw;
  a.y = (char*)yp;
  a.N = x->n; a.H = x->h; a.W = x->w; a.H0 = H0; a.W0 = W0; a.H1 = H1; a.W1 = W1;
  a.tiles_x = cdiv(W1, ST_TW); a.tiles_y = cdiv(H1, ST_TH);
  a.total = a.N * a.tiles_x * a.tiles_y;
  a.fast = x_dtype == MGDT_BF16 && x->sw == 1 && x->w % 8 == 0 && x->sh % 8 == 0 && x->sc % 8 == 0 && x->sn % 8 == 0 && (uintptr_t)x->p % 16 == 0;
  if (x_dtype != MGDT_BF16 && x_dtype != MGDT_F32 && x_dtype != MGDT_U8) MGDT_FAIL(MGDT_BAD_DTYPE, "stem2: image dtype %d", x_dtype);
  return MGDT_OK;
}

// the persistent grid and the XCD ranges of a plan on a device with `cus` compute units
static int stem2_plan_grid(StemArgs& a, int cus) {
  const int grid = stem2_grid(a.total, cus, knob_stem_wgs());           // experiment knob, read per call: cap on the grid (not part of the ABI)
  a.per_xcd = cdiv(a.total, std::min(grid, 8));
  return grid;
}

extern "C" int mgdt_stem2_route(const mgdt_view* x, int x_dtype, const mgdt_view* y, int cu_count, int* out) {
  if (!x || !y || !out || x->n <= 0 || x->h <= 0 || x->w <= 0 || x->c <= 0 || y->n <= 0 || y->h <= 0 || y->w <= 0 || y->c <= 0)
    MGDT_FAIL(MGDT_BAD_ARG, "stem2_route: null/empty argument");
  for (int i = 0; i < 7; ++i) out[i] = 0;
  StemArgs a;
  if ((out[6] = stem2_plan(x, x_dtype, y, a)) != MGDT_OK) return MGDT_OK;
  if (cu_count <= 0) cu_count = stem2_cu_count();
  if (cu_count <= 0) MGDT_FAIL(MGDT_LAUNCH_FAIL, "stem2_route: cannot read the device's compute-unit count");
  const int grid = stem2_plan_grid(a, cu_count);
  out[0] = a.fast; out[1] = a.tiles_x; out[2] = a.tiles_y; out[3] = a.total; out[4] = grid; out[5] = a.per_xcd;
  return MGDT_OK;
}

/* y = SiLU(conv1(SiLU(conv0(x)))): x = N x 3 x H x W image (NCHW, any strides; x_dtype MGDT_BF16 / MGDT_F32 / MGDT_U8 (u8: / 255 on the fly)),
 * conv0 = 3x3 s2 3 -> 16 (packed0 from mgdt_stem2_pack + bias0[16]), conv1 = 3x3 s2 16 -> 32 (packed1 = mgdt_conv_pack(16, 32, 3, bf16) +
 * bias1[32]); y = N x H1 x W1 x 32 bf16 NHWC view. */
extern "C" int mgdt_stem2_fwd(const mgdt_view* x, int x_dtype, const void* packed0, const float* bias0, const void* packed1, const float* bias1,
                              const mgdt_view* y, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(y) || !packed0 || !bias0 || !packed1 || !bias1) MGDT_FAIL(MGDT_BAD_ARG, "stem2: null/empty argument");
  StemArgs a;
  if (int e = stem2_plan(x, x_dtype, y, a)) return e;
  a.w0 = (const char*)packed0; a.b0 = bias0; a.w1 = (const char*)packed1; a.b1 = bias1;
  const int cus = stem2_cu_count();
  if (cus <= 0) MGDT_FAIL(MGDT_LAUNCH_FAIL, "stem2: cannot read the device's compute-unit count");
  const int grid = stem2_plan_grid(a, cus);
  hipStream_t st = (hipStream_t)s;
  static StampBuf stamps;            // MGDT_STEM_DBG=1: per-workgroup phase sums, printed after the launch (debug only)
  const bool dbg = knob_set("MGDT_STEM_DBG");
  if (dbg && !stamps.ensure((size_t)grid * 8)) MGDT_FAIL(MGDT_WORKSPACE, "stem2: no memory for the MGDT_STEM_DBG stamps");
  a.dbg = dbg ? stamps.p : nullptr;
  if (dbg) stamps.zero((size_t)grid * 8, st);        // a workgroup whose XCD range is empty writes nothing
#define STEM_LAUNCH(TXV)                                                      \
  do {                                                                        \
    if (dbg) stem2_kernel<TXV, true><<<grid, 256, 0, st>>>(a);                \
    else stem2_kernel<TXV, false><<<grid, 256, 0, st>>>(a);                   \
  } while (0)
  if (x_dtype == MGDT_BF16) STEM_LAUNCH(bf16);
  else if (x_dtype == MGDT_F32) STEM_LAUNCH(float);
  else STEM_LAUNCH(uint8_t);
#undef STEM_LAUNCH
  MGDT_CHECK_LAUNCH("stem2_fwd");
  if (dbg) {
    const std::vector<unsigned long long> h = stamps.read((size_t)grid * 8, st);
    double ph[7] = {0, 0, 0, 0, 0, 0, 0}, nt = 0, nw = 0;
    unsigned long long mx = 0;
    for (int i = 0; i < grid; ++i) {
      if (!h[(size_t)i * 8]) continue;
      nw += 1; nt += (double)h[(size_t)i * 8];
      unsigned long long sum = 0;
      for (int k = 0; k < 7; ++k) { ph[k] += (double)h[(size_t)i * 8 + 1 + k]; sum += h[(size_t)i * 8 + 1 + k]; }
      mx = std::max(mx, sum);
    }
    fprintf(stderr, "stem2 dtype %d fast %d n %d %dx%d (%d tiles, %d wgs of which %.0f have tiles, %d CUs): longest workgroup %.1f us; per workgroup (us): setup %.2f "
                    "first patch %.2f; avg per tile (us): next patch request %.2f barriers %.2f layer 0 %.2f next patch wait+LDS store %.2f layer 1 %.2f; sum %.2f\n",
            x_dtype, a.fast, a.N, a.H, a.W, a.total, grid, nw, cus, mx * 0.01, ph[0] / nw * 0.01, ph[1] / nw * 0.01, ph[2] / nt * 0.01, ph[3] / nt * 0.01,
            ph[4] / nt * 0.01, ph[5] / nt * 0.01, ph[6] / nt * 0.01, (ph[2] + ph[3] + ph[4] + ph[5] + ph[6]) / nt * 0.01);
  }
  return MGDT_OK;
}
