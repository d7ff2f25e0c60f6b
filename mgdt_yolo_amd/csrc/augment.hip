// Training augmentation on the device (reference yolo/data/augment.py:762-790 v8_transforms, detection, stretch=False): Mosaic(4) (:117-188) or
// LetterBox (:538-601) placement, RandomPerspective without perspective (:289-476), RandomHSV (:479-501), RandomFlip (:504-535) and Format (:692-746)
// for a whole batch in two launches.  Every random draw is made on the host (mgdt_yolo_amd/yolo/data/augment.py TrainAugment.sample, in the
// reference's order); the kernels read one mgdt_aug_record per output image (include/mgdt.h) from device memory.
//
//   aug_warp_kernel    output pixel (x, y) of image b <- flips undone <- source point inv * (x, y, 1) on the canvas <- bilinear over the four integer
//                      neighbours, each read from the rectangle of the record that holds it (114 outside every rectangle or outside the canvas: the
//                      canvas itself is never stored) <- BGR -> HSV, three LUTs, HSV -> BGR <- planes R, G, B of the (B, 3, S, S) batch.
//                      Coordinates and interpolation are fp64 (the six coefficients are fp32 words): the result is the nearest integer of the exact
//                      bilinear value of those coefficients.  cv2.warpAffine's own fixed point (1/32 pixel, 15-bit weights) is NOT reproduced.
//                      The 8-bit colour conversions follow OpenCV's documented formulas (V = max, S = 255 (V - min) / V, H / 2 in 0..179) in exact
//                      integer arithmetic, rounded half to even; H is rounded before the wrap by 180.  cv2's tables may differ by one level.
//   aug_labels_kernel  one wave per output image: the labels of its sources in source order, each in the reference's fp32 operation order (this
//                      file is built with -ffp-contract=off), kept rows compacted with a ballot prefix (no atomics).
#include "common.h"
#include <algorithm>

#define AUG_LUT_BYTES 768
#define AUG_PX 4            // adjacent output pixels of one row per lane: one 4-byte store per plane

static_assert(sizeof(mgdt_aug_record) == 224, "mgdt_aug_record is 56 words");
static_assert(sizeof(mgdt_aug_image) == 24, "mgdt_aug_image is 24 bytes");

struct AugRect { int dx1, dy1, dx2, dy2, w; long base; };      // canvas pixel (tx, ty) inside [dx1, dx2) x [dy1, dy2) reads pool[base + (ty * w + tx) * 3 ..]

// n >= 0, 0 < d, n / d < 2^15: n / d rounded half to even.  The float quotient is within 1 of the integer quotient; the remainder settles it.
__device__ __forceinline__ int aug_div_rne(int n, int d) {
  int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
  int r = n - q * d;
  if (r < 0) { q -= 1; r += d; }
  else if (r >= d) { q += 1; r -= d; }
  return q + ((2 * r > d || (2 * r == d && (q & 1))) ? 1 : 0);
}

__device__ __forceinline__ void aug_hsv(const uint8_t* lut, int& b, int& g, int& r) {
  const int v = max(b, max(g, r)), mn = min(b, min(g, r)), diff = v - mn;
  const int s = v ? aug_div_rne(255 * diff, v) : 0;
  int h = 0;
  if (diff) {
    int num, off;
    if (v == r) { num = g - b; off = 0; }
    else if (v == g) { num = b - r; off = 60; }
    else { num = r - g; off = 120; }
    const int a = aug_div_rne(30 * abs(num), diff);
    h = (num < 0 ? -a : a) + off;
    if (h < 0) h += 180;
  }
  int h2 = lut[h], s2 = lut[256 + s], v2 = lut[512 + v];
  if (h2 >= 180) h2 -= 180;
  const int sec = h2 / 30, f = h2 - sec * 30;
  // 255 * {p, q, t} of the hexcone with V = v2 / 255, S = s2 / 255, fraction f / 30: numerators over 7650
  auto rne = [](int n) { const int q = n / 7650, rr = n - q * 7650; return q + ((2 * rr > 7650 || (2 * rr == 7650 && (q & 1))) ? 1 : 0); };
  const int p = rne(v2 * (255 - s2) * 30), q = rne(v2 * (7650 - s2 * f)), t = rne(v2 * (7650 - s2 * (30 - f)));
  switch (sec) {
    case 0: r = v2; g = t; b = p; break;
    case 1: r = q; g = v2; b = p; break;
    case 2: r = p; g = v2; b = t; break;
    case 3: r = p; g = q; b = v2; break;
    case 4: r = t; g = p; b = v2; break;
    default: r = v2; g = p; b = q; break;
  }
}

__global__ __launch_bounds__(256) void aug_warp_kernel(const uint8_t* __restrict__ pool, size_t pool_bytes, const mgdt_aug_image* __restrict__ images,
                                                       int n_pool, const mgdt_aug_record* __restrict__ rec, const uint8_t* __restrict__ luts,
                                                       size_t lut_bytes, int S, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t lut[AUG_LUT_BYTES];
  const int b = blockIdx.y, tid = threadIdx.x;
  const mgdt_aug_record& R = rec[b];          // uniform address: scalar loads, the rectangle tests and the matrix stay in SGPRs
  const int canvas = R.canvas, fl = R.flags, nrect = min(max(R.nrect, 0), 4);
  const bool hsv = R.lut >= 0 && (R.lut & 3) == 0 && (size_t)R.lut + AUG_LUT_BYTES <= lut_bytes;
  if (hsv && tid < AUG_LUT_BYTES / 4) ((uint32_t*)lut)[tid] = ((const uint32_t*)(luts + R.lut))[tid];
  // a record that names what the pool does not hold reads 114 there: the rectangles are cut to their source image here, once per workgroup
  AugRect rc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rc[k] = AugRect{0, 0, 0, 0, 0, 0};
    const int src = R.rect[k][0];
    if (k < nrect && src >= 0 && src < n_pool) {
      const mgdt_aug_image im = images[src];
      const int dx1 = R.rect[k][1], dy1 = R.rect[k][2], sx1 = R.rect[k][5], sy1 = R.rect[k][6];
      const bool ok = im.h > 0 && im.w > 0 && im.offset >= 0 && (size_t)im.offset + (size_t)im.h * im.w * 3 <= pool_bytes && dx1 >= 0 && dy1 >= 0 &&
                      sx1 >= 0 && sy1 >= 0 && sx1 < im.w && sy1 < im.h;
      if (ok) {
        rc[k].dx1 = dx1; rc[k].dy1 = dy1; rc[k].w = im.w;
        rc[k].dx2 = min(min(R.rect[k][3], canvas), dx1 + (im.w - sx1));
        rc[k].dy2 = min(min(R.rect[k][4], canvas), dy1 + (im.h - sy1));
        rc[k].base = im.offset + ((long)(sy1 - dy1) * im.w + (sx1 - dx1)) * 3;
      }
    }
  }
  __syncthreads();
  const int qrow = S / AUG_PX;
  const int q = blockIdx.x * 256 + tid;
  if (q >= S * qrow) return;
  const int y = q / qrow, x0 = (q - y * qrow) * AUG_PX;
  const double ia = R.inv[0], ib = R.inv[1], ic = R.inv[2], id = R.inv[3], ie = R.inv[4], iff = R.inv[5];
  const int uy = (fl & 1) ? S - 1 - y : y;
  const double rx = ib * uy + ic, ry = ie * uy + iff;
  const double lim = (double)canvas + 1.0;

  auto tap = [&](int tx, int ty, int* px) __attribute__((always_inline)) {      // BGR of canvas pixel (tx, ty)
    long a = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)                                                  // a later rectangle overwrites an earlier one, as the assignments of _mosaic4 do
      if (tx >= rc[k].dx1 && tx < rc[k].dx2 && ty >= rc[k].dy1 && ty < rc[k].dy2) a = rc[k].base + ((long)ty * rc[k].w + tx) * 3;
    if (a >= 0) { px[0] = pool[a]; px[1] = pool[a + 1]; px[2] = pool[a + 2]; }
    else px[0] = px[1] = px[2] = 114;
  };

  uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
  for (int j = 0; j < AUG_PX; ++j) {
    const int x = x0 + j, ux = (fl & 2) ? S - 1 - x : x;
    // beyond [-1, canvas) every neighbour is 114: the clamp keeps the integer part small, the value does not change
    const double sx = fmin(fmax(ia * ux + rx, -2.0), lim), sy = fmin(fmax(id * ux + ry, -2.0), lim);
    const double fx0 = floor(sx), fy0 = floor(sy), fx = sx - fx0, fy = sy - fy0;
    const int ix = (int)fx0, iy = (int)fy0;
    int p00[3], p01[3], p10[3], p11[3];
    tap(ix, iy, p00); tap(ix + 1, iy, p01); tap(ix, iy + 1, p10); tap(ix + 1, iy + 1, p11);
    int c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double top = (1.0 - fx) * p00[ch] + fx * p01[ch], bot = (1.0 - fx) * p10[ch] + fx * p11[ch];
      c[ch] = min(max((int)rint((1.0 - fy) * top + fy * bot), 0), 255);
    }
    if (hsv) aug_hsv(lut, c[0], c[1], c[2]);
    w0 |= (uint32_t)c[2] << (8 * j); w1 |= (uint32_t)c[1] << (8 * j); w2 |= (uint32_t)c[0] << (8 * j);      // Format: planes R, G, B
  }
  const size_t plane = (size_t)S * S;
  uint8_t* o = out + (size_t)b * 3 * plane + (size_t)y * S + x0;
  *(uint32_t*)o = w0; *(uint32_t*)(o + plane) = w1; *(uint32_t*)(o + 2 * plane) = w2;
}

__global__ __launch_bounds__(64) void aug_labels_kernel(const float* __restrict__ pl, long n_labels, const mgdt_aug_image* __restrict__ images, int n_pool,
                                                        const mgdt_aug_record* __restrict__ rec, int S, int cap, float* __restrict__ gt,
                                                        float* __restrict__ labels, int32_t* __restrict__ nlabels, int32_t* __restrict__ flags) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const mgdt_aug_record& R = rec[b];
  const int nrect = min(max(R.nrect, 0), 4), fl = R.flags;
  const float cf = (float)R.canvas, Sf = (float)S, inv = (float)(1.0 / (double)S), sc = R.scale;
  const float m0 = R.m[0], m1 = R.m[1], m2 = R.m[2], m3 = R.m[3], m4 = R.m[4], m5 = R.m[5];
  const float eps = 1e-16f;
  float* G = gt + (size_t)b * cap * 5;
  float* Lb = labels + (size_t)b * cap * 5;
  int cnt = 0;
  for (int k = 0; k < nrect; ++k) {
    const int src = R.rect[k][0];
    if (src < 0 || src >= n_pool) continue;
    const mgdt_aug_image im = images[src];
    const long start = im.label_start;
    const int n = (start >= 0 && im.label_count > 0 && start + im.label_count <= n_labels) ? im.label_count : 0;
    const float wf = (float)im.w, hf = (float)im.h, px = R.pad[k][0], py = R.pad[k][1];
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      bool keep = false;
      float row[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, box[4] = {0.f, 0.f, 0.f, 0.f};
      if (i < n) {
        const float* l = pl + (start + i) * 5;
        const float x = l[1], y = l[2], w = l[3], h = l[4];
        // xywh2xyxy, denormalize by the source's (w, h), add_padding (Mosaic._update_labels :239-245; CopyPaste :615-616 + LetterBox._update_labels :595-601)
        float x1 = (x - w / 2.f) * wf + px, y1 = (y - h / 2.f) * hf + py, x2 = (x + w / 2.f) * wf + px, y2 = (y + h / 2.f) * hf + py;
        bool good = true;
        if (fl & 4) {      // Mosaic._cat_labels :264-266: clip to the canvas, remove_zero_area_boxes
          x1 = fminf(fmaxf(x1, 0.f), cf); x2 = fminf(fmaxf(x2, 0.f), cf); y1 = fminf(fmaxf(y1, 0.f), cf); y2 = fminf(fmaxf(y2, 0.f), cf);
          good = (x2 - x1) * (y2 - y1) > 0.f;
        }
        // apply_bboxes :348-371: corners x1y1, x2y2, x1y2, x2y1 through M, new box = their extent; clip to (S, S)
        const float ax = x1 * m0 + y1 * m1 + m2, ay = x1 * m3 + y1 * m4 + m5, bx = x2 * m0 + y2 * m1 + m2, by = x2 * m3 + y2 * m4 + m5;
        const float cx_ = x1 * m0 + y2 * m1 + m2, cy_ = x1 * m3 + y2 * m4 + m5, dx = x2 * m0 + y1 * m1 + m2, dy = x2 * m3 + y1 * m4 + m5;
        float nx1 = fminf(fminf(ax, bx), fminf(cx_, dx)), nx2 = fmaxf(fmaxf(ax, bx), fmaxf(cx_, dx));
        float ny1 = fminf(fminf(ay, by), fminf(cy_, dy)), ny2 = fmaxf(fmaxf(ay, by), fmaxf(cy_, dy));
        nx1 = fminf(fmaxf(nx1, 0.f), Sf); nx2 = fminf(fmaxf(nx2, 0.f), Sf); ny1 = fminf(fmaxf(ny1, 0.f), Sf); ny2 = fminf(fmaxf(ny2, 0.f), Sf);
        // box_candidates :471-476 against the source box scaled by s
        const float w1 = x2 * sc - x1 * sc, h1 = y2 * sc - y1 * sc, w2 = nx2 - nx1, h2 = ny2 - ny1;
        const float ar = fmaxf(w2 / (h2 + eps), h2 / (w2 + eps));
        keep = good && w2 > 2.f && h2 > 2.f && w2 * h2 / (w1 * h1 + eps) > 0.1f && ar < 100.f;
        // Albumentations.__call__ :677-678 (xywh, normalize), RandomFlip on normalized xywh, Format :716-729 (denormalize, normalize)
        float cx = (nx1 + nx2) / 2.f * inv, cy = (ny1 + ny2) / 2.f * inv;
        const float bw = w2 * inv * Sf * inv, bh = h2 * inv * Sf * inv;
        if (fl & 1) cy = 1.f - cy;
        if (fl & 2) cx = 1.f - cx;
        cx = cx * Sf * inv; cy = cy * Sf * inv;
        row[0] = l[0]; row[1] = cx; row[2] = cy; row[3] = bw; row[4] = bh;
        // v8DetectionLoss.preprocess: xywh * (w, h, w, h), xywh2xyxy
        const float X = cx * Sf, Y = cy * Sf, W = bw * Sf, H = bh * Sf;
        box[0] = X - W / 2.f; box[1] = Y - H / 2.f; box[2] = X + W / 2.f; box[3] = Y + H / 2.f;
      }
      const unsigned long long mask = __ballot(keep);
      const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep && pos < cap) {
#pragma unroll
        for (int e = 0; e < 5; ++e) Lb[pos * 5 + e] = row[e];
        G[pos * 5] = row[0];
#pragma unroll
        for (int e = 0; e < 4; ++e) G[pos * 5 + 1 + e] = box[e];
      }
      cnt += __popcll(mask);
    }
  }
  const int nout = min(cnt, cap);
  for (int e = nout * 5 + lane; e < cap * 5; e += 64) { G[e] = 0.f; Lb[e] = 0.f; }
  if (lane == 0) { nlabels[b] = nout; flags[b] = cnt > cap ? 1 : 0; }
}

static bool aug_finite(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!(v[i] - v[i] == 0.f)) return false;
  return true;
}

extern "C" int mgdt_aug_check(const mgdt_aug_record* records, int batch, const mgdt_aug_image* images, int n_pool, size_t pool_bytes, long n_labels,
                              size_t lut_bytes, int imgsz) {
  if (!records || !images) MGDT_FAIL(MGDT_BAD_ARG, "aug_check: null pointer");
  if (batch < 1 || batch > 65535 || n_pool < 1 || imgsz < 4 || imgsz > 8192 || imgsz % AUG_PX || n_labels < 0)
    MGDT_FAIL(MGDT_BAD_SHAPE, "aug_check: batch=%d (1..65535) n_pool=%d (>= 1) imgsz=%d (4..8192, a multiple of %d) n_labels=%ld", batch, n_pool, imgsz,
              AUG_PX, n_labels);
  for (int i = 0; i < n_pool; ++i) {
    const mgdt_aug_image& im = images[i];
    if (im.h < 1 || im.w < 1 || im.h > imgsz || im.w > imgsz || im.offset < 0 || (size_t)im.offset + (size_t)im.h * im.w * 3 > pool_bytes)
      MGDT_FAIL(MGDT_BAD_SHAPE, "aug_check: pool image %d: %d x %d at byte %lld does not lie in a pool of %zu bytes of images up to %d", i, im.h, im.w,
                (long long)im.offset, pool_bytes, imgsz);
    if (im.label_start < 0 || im.label_count < 0 || (long)im.label_start + im.label_count > n_labels)
      MGDT_FAIL(MGDT_BAD_SHAPE, "aug_check: pool image %d: labels %d..+%d of %ld", i, im.label_start, im.label_count, n_labels);
  }
  for (int b = 0; b < batch; ++b) {
    const mgdt_aug_record& r = records[b];
    if (r.nrect < 0 || r.nrect > 4 || r.canvas < 1 || r.canvas > 2 * imgsz || (r.flags & ~7))
      MGDT_FAIL(MGDT_BAD_SHAPE, "aug_check: record %d: nrect=%d (0..4) canvas=%d (1..%d) flags=%d (0..7)", b, r.nrect, r.canvas, 2 * imgsz, r.flags);
    if (r.lut != -1 && (r.lut < 0 || (r.lut & 3) || (size_t)r.lut + AUG_LUT_BYTES > lut_bytes))
      MGDT_FAIL(MGDT_BAD_ARG, "aug_check: record %d: LUT offset %d (-1, or a multiple of 4 with 768 bytes inside %zu)", b, r.lut, lut_bytes);
    if (!aug_finite(r.inv, 6) || !aug_finite(r.m, 6) || !aug_finite(&r.scale, 1) || !aug_finite(&r.pad[0][0], 8))
      MGDT_FAIL(MGDT_BAD_ARG, "aug_check: record %d holds a non-finite coefficient", b);
    for (int k = 0; k < r.nrect; ++k) {
      const int32_t* q = r.rect[k];
      if (q[0] < 0 || q[0] >= n_pool) MGDT_FAIL(MGDT_BAD_ARG, "aug_check: record %d rectangle %d: source id %d outside 0..%d", b, k, q[0], n_pool - 1);
      const mgdt_aug_image& im = images[q[0]];
      if (q[1] < 0 || q[2] < 0 || q[3] < q[1] || q[4] < q[2] || q[3] > r.canvas || q[4] > r.canvas || q[5] < 0 || q[6] < 0 ||
          q[5] + (q[3] - q[1]) > im.w || q[6] + (q[4] - q[2]) > im.h)
        MGDT_FAIL(MGDT_BAD_SHAPE, "aug_check: record %d rectangle %d: [%d, %d) x [%d, %d) from (%d, %d) of a %d x %d image on a canvas of %d", b, k, q[1],
                  q[3], q[2], q[4], q[5], q[6], im.h, im.w, r.canvas);
    }
  }
  return MGDT_OK;
}

extern "C" int mgdt_aug_warp_fwd(const void* pool, size_t pool_bytes, const mgdt_aug_image* images_dev, const mgdt_aug_image* images_host, int n_pool,
                                 const mgdt_aug_record* records_dev, const mgdt_aug_record* records_host, const void* luts, size_t lut_bytes, int batch,
                                 int imgsz, void* out, mgdt_stream s) {
  if (!pool || !images_dev || !images_host || !records_dev || !records_host || !out || (lut_bytes && !luts))
    MGDT_FAIL(MGDT_BAD_ARG, "aug_warp_fwd: null pointer");
  if (((uintptr_t)images_dev & 7) || ((uintptr_t)records_dev & 7) || ((uintptr_t)luts & 3) || ((uintptr_t)out & 3))
    MGDT_FAIL(MGDT_BAD_ARG, "aug_warp_fwd: images / records must be 8-byte aligned, luts / out 4-byte aligned");
  const int st = mgdt_aug_check(records_host, batch, images_host, n_pool, pool_bytes, 0x7fffffffL, lut_bytes, imgsz);
  if (st != MGDT_OK) return st;
  const long quads = (long)imgsz * (imgsz / AUG_PX);
  aug_warp_kernel<<<dim3((unsigned)cdiv(quads, 256), (unsigned)batch), 256, 0, (hipStream_t)s>>>((const uint8_t*)pool, pool_bytes, images_dev, n_pool,
                                                                                                  records_dev, (const uint8_t*)luts, lut_bytes, imgsz,
                                                                                                  (uint8_t*)out);
  MGDT_CHECK_LAUNCH("aug_warp_fwd");
  return MGDT_OK;
}

extern "C" int mgdt_aug_labels_fwd(const float* pool_labels, long n_labels, const mgdt_aug_image* images_dev, const mgdt_aug_image* images_host,
                                   int n_pool, const mgdt_aug_record* records_dev, const mgdt_aug_record* records_host, int batch, int imgsz, int cap,
                                   float* gt, float* labels, int32_t* nlabels, int32_t* flags, mgdt_stream s) {
  if (!images_dev || !images_host || !records_dev || !records_host || !gt || !labels || !nlabels || !flags || (n_labels > 0 && !pool_labels))
    MGDT_FAIL(MGDT_BAD_ARG, "aug_labels_fwd: null pointer");
  if (((uintptr_t)images_dev & 7) || ((uintptr_t)records_dev & 7) || ((uintptr_t)pool_labels & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)labels & 3) ||
      ((uintptr_t)nlabels & 3) || ((uintptr_t)flags & 3))
    MGDT_FAIL(MGDT_BAD_ARG, "aug_labels_fwd: images / records must be 8-byte aligned, every other array 4-byte aligned");
  if (cap < 16 || cap % 16 || cap > (1 << 20)) MGDT_FAIL(MGDT_BAD_SHAPE, "aug_labels_fwd: capacity %d (a multiple of 16 in 16..2^20)", cap);
  if (n_labels < 0) MGDT_FAIL(MGDT_BAD_SHAPE, "aug_labels_fwd: n_labels=%ld", n_labels);
  size_t worst = 0;      // the pool bytes the image table needs: this call reads no pixel
  for (int i = 0; images_host && i < n_pool; ++i)
    if (images_host[i].offset >= 0 && images_host[i].h > 0 && images_host[i].w > 0)
      worst = std::max(worst, (size_t)images_host[i].offset + (size_t)images_host[i].h * images_host[i].w * 3);
  const int st = mgdt_aug_check(records_host, batch, images_host, n_pool, worst, n_labels, (size_t)1 << 40, imgsz);
  if (st != MGDT_OK) return st;
  aug_labels_kernel<<<batch, 64, 0, (hipStream_t)s>>>(pool_labels, n_labels, images_dev, n_pool, records_dev, imgsz, cap, gt, labels, nlabels, flags);
  MGDT_CHECK_LAUNCH("aug_labels_fwd");
  return MGDT_OK;
}
