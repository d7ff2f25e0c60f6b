// Instance-segmentation inference (reference nn/modules/head.py:189-212 Segment, nn/modules/block.py:57-69 Proto,
// yolo/utils/ops.py:541-636 crop_mask / process_mask / process_mask_upsample / process_mask_native).
//
//   deconv2x2      Proto.upsample = nn.ConvTranspose2d(c, c, 2, 2, 0, bias): kernel size == stride, so output pixel (2y + dy, 2x + dx) depends on
//                  input pixel (y, x) alone: four 1x1 implicit GEMMs (one panel per (dy, dx)) whose output views are the four stride-2 phases
//                  of y.  No new arithmetic: the MFMA kernel of mgdt_conv2d_fwd writes through the strided views.
//   seg_concat     (B, 4+nc, A) prediction of Detect + the per-level NHWC cv4 maps -> the (B, 4+nc+nm, A) prediction the reference returns.
//   seg_masks      the mask assembly in one launch.  A workgroup owns (image, 16 detections, one tile of output pixels):
//                    1. logits of the proto pixels under the tile (the source rectangle of the tile's bilinear taps) on MFMA: pixels are the
//                       M rows (16 per instruction, A operand = one 16-byte (bf16) / two 16-byte (fp32) loads of a pixel's nm = 32 coefficients
//                       per lane), the 16 detections the N columns (B operand: their 32 mask coefficients, loaded once per workgroup);
//                       sigmoid (and, for process_mask, the crop at proto resolution) in the accumulator registers, then one 16-byte LDS write
//                       per lane: S[det][pixel .. pixel + 3]
//                    2. every thread resamples runs of 16 consecutive output pixels of one (detection, row) out of LDS (align_corners=False
//                       weights in PyTorch's CPU arithmetic, see tta.hip), crops, thresholds > 0.5 and stores the run as 16 bytes (uint8) or
//                       four 16-byte pieces (fp32)
//                  A detection whose crop box misses the tile stores zeros without touching LDS; a workgroup where that holds for all its
//                  detections skips the GEMM as well.  The tests compare against the launch with `no_skip`.
#include "common.h"

// ================================================================================================ transposed 2x2 stride-2 convolution
extern "C" int mgdt_deconv2x2_fwd(const mgdt_view* x, const void* const* packed4, const float* bias, const mgdt_view* y, int dtype, mgdt_stream s) {
  if (!view_ok(x) || !view_ok(y) || !packed4 || !bias) MGDT_FAIL(MGDT_BAD_ARG, "deconv2x2: null/empty view or weights");
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "deconv2x2: dtype %d", dtype);
  if (y->n != x->n || y->h != 2 * x->h || y->w != 2 * x->w)
    MGDT_FAIL(MGDT_BAD_SHAPE, "deconv2x2: y is %dx%dx%d, expected %dx%dx%d (kernel 2, stride 2, padding 0)", y->n, y->h, y->w, x->n, 2 * x->h, 2 * x->w);
  for (int ph = 0; ph < 4; ++ph) {
    if (!packed4[ph]) MGDT_FAIL(MGDT_BAD_ARG, "deconv2x2: panel %d is null", ph);
    const int dy = ph >> 1, dx = ph & 1;
    mgdt_view v = *y;
    v.p = (char*)y->p + ((int64_t)dy * y->sh + (int64_t)dx * y->sw) * (int64_t)dtype_size(dtype);
    v.h = x->h; v.w = x->w; v.sh = 2 * y->sh; v.sw = 2 * y->sw;
    const int st = mgdt_conv2d_fwd(x, nullptr, nullptr, nullptr, packed4[ph], bias, 1, 1, MGDT_ACT_NONE, nullptr, nullptr, &v, dtype, s);
    if (st != MGDT_OK) return st;
  }
  return MGDT_OK;
}

// ================================================================================================ prediction + mask coefficients
#define SEG_MAX_LEVELS 4
struct SegCatArgs {
  const float* y; float* out;
  const void* mc[SEG_MAX_LEVELS]; long sn[SEG_MAX_LEVELS], sp[SEG_MAX_LEVELS];   // level maps: image stride, pixel stride (elements); w == row length
  long sh[SEG_MAX_LEVELS];
  int lw[SEG_MAX_LEVELS], a_off[SEG_MAX_LEVELS + 1];
  int B, rows, nm, A, levels;
};

template <typename T>
__global__ __launch_bounds__(256) void seg_concat_kernel(const SegCatArgs a) {
  const int b = blockIdx.y, an = blockIdx.x * 256 + threadIdx.x;
  if (an >= a.A) return;
  const float* src = a.y + (long)b * a.rows * a.A + an;
  float* dst = a.out + (long)b * (a.rows + a.nm) * a.A + an;
  for (int r = 0; r < a.rows; ++r) dst[(long)r * a.A] = src[(long)r * a.A];
  int l = 0;
  while (l + 1 < a.levels && an >= a.a_off[l + 1]) ++l;
  const int pix = an - a.a_off[l], py = pix / a.lw[l], px = pix - py * a.lw[l];
  const T* m = (const T*)a.mc[l] + (long)b * a.sn[l] + (long)py * a.sh[l] + (long)px * a.sp[l];
  dst += (long)a.rows * a.A;
  for (int k = 0; k < a.nm; k += 4) {           // nm % 4 == 0, 4-element aligned pieces (checked by the host)
    const f32x4 v = load4<T>(m + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[(long)(k + e) * a.A] = v[e];
  }
}

extern "C" int mgdt_seg_concat_fwd(const float* y, int n, int rows, int a_total, const mgdt_view* const* mc, int n_levels, int nm, float* out, int dtype,
                                   mgdt_stream s) {
  if (!y || !out || !mc) MGDT_FAIL(MGDT_BAD_ARG, "seg_concat: null pointer");
  if (n < 1 || rows < 5 || a_total < 1 || nm < 4 || nm % 4 || n_levels < 1 || n_levels > SEG_MAX_LEVELS || n > 65535)
    MGDT_FAIL(MGDT_BAD_SHAPE, "seg_concat: n=%d rows=%d a=%d nm=%d (a multiple of 4) levels=%d (<= %d)", n, rows, a_total, nm, n_levels, SEG_MAX_LEVELS);
  SegCatArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y; a.out = out; a.B = n; a.rows = rows; a.nm = nm; a.A = a_total; a.levels = n_levels;
  int off = 0;
  const size_t es = dtype_size(dtype);
  for (int l = 0; l < n_levels; ++l) {
    const mgdt_view* v = mc[l];
    if (!view_ok(v) || v->n != n || v->c != nm || v->sc != 1) MGDT_FAIL(MGDT_BAD_SHAPE, "seg_concat: level %d must be an NHWC view of %d x h x w x %d", l, n, nm);
    if (v->sn % 4 || v->sh % 4 || v->sw % 4 || ((uintptr_t)v->p % (4 * es))) MGDT_FAIL(MGDT_BAD_SHAPE, "seg_concat: level %d is not made of 4-element aligned pieces", l);
    a.mc[l] = v->p; a.sn[l] = v->sn; a.sh[l] = v->sh; a.sp[l] = v->sw; a.lw[l] = v->w; a.a_off[l] = off;
    off += v->h * v->w;
  }
  a.a_off[n_levels] = off;
  if (off != a_total) MGDT_FAIL(MGDT_BAD_SHAPE, "seg_concat: the levels hold %d anchors, the prediction %d", off, a_total);
  const dim3 grid(cdiv(a_total, 256), n);
  MGDT_DISPATCH_DTYPE(dtype, (seg_concat_kernel<T><<<grid, 256, 0, (hipStream_t)s>>>(a)));
  MGDT_CHECK_LAUNCH("seg_concat_fwd");
  return MGDT_OK;
}

// ================================================================================================ fused mask assembly
#define SEG_NM 32                 // K of the logit GEMM: one 16x16x32 bf16 MFMA, eight 16x16x4 fp32 ones
#define SEG_DETS 16               // detections per workgroup (N of the MFMA)
#define SEG_CAP 512               // proto pixels under one tile (LDS: 16 x (512 + 4) fp32 = 32.25 KiB)
#define SEG_SROW (SEG_CAP + 4)    // LDS row stride: 16-byte aligned and not a multiple of 32 banks (the phase-1 write still collides: lanes (j, g) and (j + 1, g - 1) share banks)
#define SEG_RUN 16                // output pixels per thread step

struct SegMaskArgs {
  const void* protos; long psn, psh, psw;      // (B, mh, mw, 32) NHWC, element strides
  const float* rows; const int32_t* counts; const int32_t* offsets;
  void* out;
  int mh, mw, max_det, row_w;
  int top, left, wh, ww;                       // source window of the protos (process_mask_native: letter-box crop; else the whole map)
  int OH, OW, TOH, TOW, tiles_x;
  float sy, sx;                                // (float)wh / OH, (float)ww / OW
  int crop_before, crop_after, no_skip, vec;
  float bsx, bsy;                              // crop_before: box * (mw / iw), box * (mh / ih) (ops.py:601-605)
};

// source index / weight of output coordinate o (PyTorch CPU upsample_bilinear2d, align_corners=False, output size given)
__device__ __forceinline__ void seg_tap(float scale, int o, int n_in, int& i0, int& i1, float& w1) {
  const float s = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);
  i0 = min((int)s, n_in - 1);
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  w1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

template <typename T, typename TO>
__global__ __launch_bounds__(256) void seg_mask_kernel(const SegMaskArgs a) {
  __shared__ __attribute__((aligned(16))) float S[SEG_DETS * SEG_SROW];
  __shared__ float s_box[SEG_DETS][4];
  __shared__ int s_live[SEG_DETS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, d0 = blockIdx.y * SEG_DETS;
  const int cnt = min(a.counts[b], a.max_det);
  if (d0 >= cnt) return;                                     // uniform
  const int nd = min(SEG_DETS, cnt - d0);
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int oy0 = ty * a.TOH, ox0 = tx * a.TOW;
  const int oy1 = min(oy0 + a.TOH, a.OH), ox1 = min(ox0 + a.TOW, a.OW);     // exclusive
  // source rectangle of the tile's taps (window coordinates): i0 of the first output row / column .. i1 of the last one (both monotone)
  int ry0, ry1, rx0, rx1, t;
  float tw;
  seg_tap(a.sy, oy0, a.wh, ry0, t, tw);
  seg_tap(a.sy, oy1 - 1, a.wh, t, ry1, tw);
  seg_tap(a.sx, ox0, a.ww, rx0, t, tw);
  seg_tap(a.sx, ox1 - 1, a.ww, t, rx1, tw);
  const int RW = min(rx1 - rx0 + 1, SEG_CAP);
  int RH = ry1 - ry0 + 1;
  if (RH * RW > SEG_CAP) RH = SEG_CAP / RW;                  // cannot happen (the host sizes the tile); keeps every LDS index in range
  const int NP = RH * RW;
  const float* R = a.rows + ((long)b * a.max_det + d0) * a.row_w;

  // ---- which detections can be non-zero inside this tile
  if (tid < SEG_DETS) {
    int live = 0;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (tid < nd) {
      const float* r = R + (long)tid * a.row_w;
      x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
      live = 1;
      if (!a.no_skip) {
        if (a.crop_after) {                                   // every output pixel of the tile fails r >= x1 && r < x2 && c >= y1 && c < y2
          if ((float)(ox1 - 1) < x1 || !((float)ox0 < x2) || (float)(oy1 - 1) < y1 || !((float)oy0 < y2)) live = 0;
        }
        if (a.crop_before) {                                  // every tap of the tile is cropped to zero
          const float bx1 = x1 * a.bsx, bx2 = x2 * a.bsx, by1 = y1 * a.bsy, by2 = y2 * a.bsy;
          if ((float)(a.left + rx1) < bx1 || !((float)(a.left + rx0) < bx2) || (float)(a.top + ry1) < by1 || !((float)(a.top + ry0) < by2)) live = 0;
        }
      }
    }
    s_box[tid][0] = x1; s_box[tid][1] = y1; s_box[tid][2] = x2; s_box[tid][3] = y2;
    s_live[tid] = live;
  }
  __syncthreads();
  int any_live = 0;
#pragma unroll
  for (int j = 0; j < SEG_DETS; ++j) any_live |= s_live[j];

  // ---- 1. logits -> sigmoid (-> crop at proto resolution) -> LDS
  if (any_live) {
    const int j = lane & 15, g = lane >> 4;                   // B operand: detection j, k = 8g .. 8g + 7; D: detection j, pixels 4g .. 4g + 3
    float cf[8];
    {
      const float* r = R + (long)min(j, nd - 1) * a.row_w + 6 + 8 * g;
#pragma unroll
      for (int e = 0; e < 8; ++e) cf[e] = j < nd ? r[e] : 0.f;
    }
    bf16x8 cb;
#pragma unroll
    for (int e = 0; e < 8; ++e) cb[e] = (bf16)cf[e];
    const float bx1 = s_box[j][0] * a.bsx, by1 = s_box[j][1] * a.bsy, bx2 = s_box[j][2] * a.bsx, by2 = s_box[j][3] * a.bsy;
    const T* P = (const T*)a.protos + (long)b * a.psn;
    for (int p0 = wave * 16; p0 < NP; p0 += 64) {             // 16 pixels per wave step
      const int p = min(p0 + j, NP - 1);                      // A operand: pixel p0 + (lane & 15), k = 8g .. 8g + 7
      const int py = p / RW, px = p - py * RW;
      const T* src = P + (long)(a.top + ry0 + py) * a.psh + (long)(a.left + rx0 + px) * a.psw + 8 * g;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if constexpr (sizeof(T) == 2) {
        const bf16x8 v = *(const bf16x8*)src;
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v, cb, acc, 0, 0, 0);
      } else {
        const f32x4 v0 = *(const f32x4*)src, v1 = *(const f32x4*)(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[e], cf[e], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[e], cf[4 + e], acc, 0, 0, 0);
      }
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = fast_sigmoid(acc[e]);
        if (a.crop_before) {
          const int q = min(p0 + 4 * g + e, NP - 1), qy = q / RW, qx = q - qy * RW;
          const float fx = (float)(a.left + rx0 + qx), fy = (float)(a.top + ry0 + qy);
          if (!(fx >= bx1 && fx < bx2 && fy >= by1 && fy < by2)) v = 0.f;
        }
        o[e] = v;
      }
      *(f32x4*)&S[j * SEG_SROW + p0 + 4 * g] = o;             // p0 + 15 < SEG_CAP: NP <= SEG_CAP, which is a multiple of 16
    }
  }
  __syncthreads();

  // ---- 2. resample, crop, threshold, store
  const int runs_x = (ox1 - ox0 + SEG_RUN - 1) / SEG_RUN, th = oy1 - oy0;
  const int per_det = th * runs_x, total = nd * per_det;
  const long plane = (long)a.OH * a.OW;
  TO* O = (TO*)a.out + ((long)a.offsets[b] + d0) * plane;
  for (int it = tid; it < total; it += 256) {
    const int j = it / per_det, rem = it - j * per_det;
    const int row = rem / runs_x, run = rem - row * runs_x;
    const int oy = oy0 + row, oxs = ox0 + run * SEG_RUN;
    const int nx = min(SEG_RUN, ox1 - oxs);
    float val[SEG_RUN];
    const float x1 = s_box[j][0], y1 = s_box[j][1], x2 = s_box[j][2], y2 = s_box[j][3];
    const bool row_in = !a.crop_after || ((float)oy >= y1 && (float)oy < y2);
    if (s_live[j] && row_in) {
      int iy0, iy1;
      float h1;
      seg_tap(a.sy, oy, a.wh, iy0, iy1, h1);
      const float h0 = 1.f - h1;
      const float* s0 = &S[j * SEG_SROW + min(iy0 - ry0, RH - 1) * RW];
      const float* s1 = &S[j * SEG_SROW + min(iy1 - ry0, RH - 1) * RW];
      int c0 = -1, c1 = -1;
      float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;         // (row iy0, row iy1) at columns c0 / c1
#pragma unroll
      for (int k = 0; k < SEG_RUN; ++k) {
        int ix0, ix1;
        float w1;
        seg_tap(a.sx, min(oxs + k, ox1 - 1), a.ww, ix0, ix1, w1);
        ix0 = min(ix0 - rx0, RW - 1); ix1 = min(ix1 - rx0, RW - 1);
        if (ix0 != c0) {
          if (ix0 == c1) { a0 = a1; b0 = b1; } else { a0 = s0[ix0]; b0 = s1[ix0]; }
          c0 = ix0;
        }
        if (ix1 != c1) {
          if (ix1 == c0) { a1 = a0; b1 = b0; } else { a1 = s0[ix1]; b1 = s1[ix1]; }
          c1 = ix1;
        }
        const float w0 = 1.f - w1;
        float v = (a0 * w0 + a1 * w1) * h0 + (b0 * w0 + b1 * w1) * h1;
        if (a.crop_after) {
          const float fx = (float)(oxs + k);
          if (!(fx >= x1 && fx < x2)) v = 0.f;
        }
        val[k] = v > 0.5f ? 1.f : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < SEG_RUN; ++k) val[k] = 0.f;
    }
    TO* o = O + (long)j * plane + (long)oy * a.OW + oxs;
    if (a.vec && nx == SEG_RUN) {
      if constexpr (sizeof(TO) == 1) {
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
        u32x4 w;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          w[q] = (unsigned)val[4 * q] | ((unsigned)val[4 * q + 1] << 8) | ((unsigned)val[4 * q + 2] << 16) | ((unsigned)val[4 * q + 3] << 24);
        *(u32x4*)o = w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) *(f32x4*)(o + 4 * q) = f32x4{val[4 * q], val[4 * q + 1], val[4 * q + 2], val[4 * q + 3]};
      }
    } else {
#pragma unroll
      for (int k = 0; k < SEG_RUN; ++k)
        if (k < nx) o[k] = (TO)val[k];
    }
  }
}

// Tile of the mask kernel for an (wh x ww) source window resampled to OH x OW: the largest of the candidates whose taps fit SEG_CAP proto
// pixels.  geom4 = {TOH, TOW, tiles_y, tiles_x}; returns 0 when even one 16-pixel run does not fit (down-sampling by more than ~30x).
static int seg_tile(int wh, int ww, int OH, int OW, int* geom4) {
  const float sy = (float)wh / (float)OH, sx = (float)ww / (float)OW;
  auto span = [](float sc, int t, int n_in) { return std::min((int)(sc * (float)t) + 3, n_in); };     // source rows / columns under t output ones (upper bound)
  int TOH = 32, TOW = 128;
  auto fits = [&]() {
    const int rh = span(sy, TOH, wh), rw = span(sx, TOW, ww);
    return (rh * rw + 15) / 16 * 16 <= SEG_CAP;
  };
  while (!fits() && TOH > 1) TOH >>= 1;
  while (!fits() && TOW > SEG_RUN) TOW >>= 1;
  if (!fits()) return 0;
  geom4[0] = TOH; geom4[1] = TOW; geom4[2] = cdiv(OH, TOH); geom4[3] = cdiv(OW, TOW);
  return 1;
}

extern "C" int mgdt_seg_mask_geometry(int wh, int ww, int oh, int ow, int* geom4) {
  if (!geom4 || wh < 1 || ww < 1 || oh < 1 || ow < 1) MGDT_FAIL(MGDT_BAD_ARG, "seg_mask_geometry: bad argument");
  return seg_tile(wh, ww, oh, ow, geom4);
}

extern "C" int mgdt_seg_masks_fwd(const mgdt_view* protos, const float* rows, const int32_t* counts, const int32_t* offsets, int max_det, int nm,
                                  int top, int left, int win_h, int win_w, int out_h, int out_w, int crop_before, float box_sx, float box_sy,
                                  int crop_after, int no_skip, void* out, int out_u8, int dtype, mgdt_stream s) {
  if (!view_ok(protos) || !rows || !counts || !offsets || !out) MGDT_FAIL(MGDT_BAD_ARG, "seg_masks: null/empty argument");
  if (nm != SEG_NM || protos->c != nm) MGDT_FAIL(MGDT_BAD_SHAPE, "seg_masks: built for nm = %d mask coefficients (rows have %d, protos %d channels)", SEG_NM, nm, protos->c);
  if (dtype != MGDT_F32 && dtype != MGDT_BF16) MGDT_FAIL(MGDT_BAD_DTYPE, "seg_masks: dtype %d", dtype);
  const int pe = dtype == MGDT_BF16 ? 8 : 4;
  if (protos->sc != 1 || protos->sw % pe || protos->sh % pe || protos->sn % pe || ((uintptr_t)protos->p & 15))
    MGDT_FAIL(MGDT_BAD_SHAPE, "seg_masks: protos must be an NHWC view (sc == 1) of 16-byte aligned pixels");
  if (max_det < 1 || protos->n > 65535 || top < 0 || left < 0 || win_h < 1 || win_w < 1 || top + win_h > protos->h || left + win_w > protos->w || out_h < 1 || out_w < 1)
    MGDT_FAIL(MGDT_BAD_SHAPE, "seg_masks: window %d+%d x %d+%d of %dx%d protos, output %dx%d, max_det %d", top, win_h, left, win_w, protos->h, protos->w, out_h, out_w, max_det);
  if ((long)out_h * out_w > 0x3fffffffL) MGDT_FAIL(MGDT_BAD_SHAPE, "seg_masks: output plane too large");
  int geom[4];
  if (!seg_tile(win_h, win_w, out_h, out_w, geom))
    MGDT_FAIL(MGDT_BAD_SHAPE, "seg_masks: %dx%d -> %dx%d shrinks the protos too much for one tile's %d source pixels", win_h, win_w, out_h, out_w, SEG_CAP);
  SegMaskArgs a;
  a.protos = protos->p; a.psn = protos->sn; a.psh = protos->sh; a.psw = protos->sw;
  a.rows = rows; a.counts = counts; a.offsets = offsets; a.out = out;
  a.mh = protos->h; a.mw = protos->w; a.max_det = max_det; a.row_w = 6 + nm;
  a.top = top; a.left = left; a.wh = win_h; a.ww = win_w;
  a.OH = out_h; a.OW = out_w; a.TOH = geom[0]; a.TOW = geom[1]; a.tiles_x = geom[3];
  a.sy = (float)win_h / (float)out_h; a.sx = (float)win_w / (float)out_w;
  a.crop_before = crop_before ? 1 : 0; a.crop_after = crop_after ? 1 : 0; a.no_skip = no_skip ? 1 : 0;
  a.bsx = box_sx; a.bsy = box_sy;
  const int es = out_u8 ? 1 : 4;
  a.vec = ((long)out_w * es) % 16 == 0 && ((uintptr_t)out & 15) == 0;      // every run of 16 pixels starts on a 16-byte boundary
  const dim3 grid(geom[2] * geom[3], cdiv(max_det, SEG_DETS), protos->n);
  if (grid.y > 65535) MGDT_FAIL(MGDT_BAD_SHAPE, "seg_masks: max_det %d too large", max_det);
#define SEG_LAUNCH(T, TO) seg_mask_kernel<T, TO><<<grid, 256, 0, (hipStream_t)s>>>(a)
  if (dtype == MGDT_BF16) { if (out_u8) SEG_LAUNCH(bf16, uint8_t); else SEG_LAUNCH(bf16, float); }
  else { if (out_u8) SEG_LAUNCH(float, uint8_t); else SEG_LAUNCH(float, float); }
#undef SEG_LAUNCH
  MGDT_CHECK_LAUNCH("seg_masks_fwd");
  return MGDT_OK;
}
