// RT-DETR criterion and validator post-processing (reference vit/utils/ops.py:12-111 HungarianMatcher, vit/utils/loss.py DETRLoss /
// RTDETRDetectionLoss, yolo/utils/loss.py:16-53 VarifocalLoss / FocalLoss, yolo/utils/metrics.py:75-128 bbox_iou, vit/rtdetr/val.py:90-106).
// This file is built with -ffp-contract=off: the assignment is discontinuous in the costs, so the cost arithmetic rounds after every operation,
// in the reference's operation order.
//
//   match     one workgroup of ONE wave per (layer, image): the wave first writes the image's cost block, ground-truth major
//             (ws[layer][global gt][nq] fp32, the row a scan reads is contiguous over the lanes), then solves it.  The block lives in the caller's
//             workspace, layers * G * nq * 4 bytes (2.7 MB at 7 layers, 320 ground truths, 300 queries: L2-resident); LDS holds only the solver's
//             vectors (28 bytes per query rounded to 64, 8 bytes per ground truth).
//   solver    linear_sum_assignment on the ng x nq block (ng <= nq): shortest augmenting paths, the ground truths in sequence as rows, the
//             queries as columns spread over the lanes, fp64 potentials; every ground truth ends on a distinct query.  Exact for the fp32 cost
//             values up to fp64 rounding of path sums.  On equal reduced costs the lower query wins.  A cost that is not finite (NaN, +-inf) is
//             replaced by DL_BIG_COST = 1e18 (finite in fp32, and 256 of them still add exactly enough in fp64 to order below 1e300): no
//             fault, no endless loop - every loop has a fixed bound.  A class index outside [0, nc) is clamped.
//   loss      one launch for every layer: a workgroup owns 64 queries of one (layer, image).  Its first wave does the box terms of the matched
//             queries in fp64 (IoU target score, L1, GIoU and their gradients), all four waves the class terms in fp32 (varifocal or focal),
//             accumulated in fp64.  The three sums go to a per-workgroup partial; the workgroup that arrives last (one integer counter, which it
//             puts back to 0) adds the partials of every layer in a fixed order, and the auxiliary layers' sums.  No floating-point atomic:
//             losses and gradients are bit-equal from run to run.  The partials are published with returning agent-scope exchanges and read
//             with agent-scope loads (as cnx_block does), so no cache-wide fence is needed.
//   val_post  the validator's rows: one workgroup per image, class maximum per query (lowest class on ties, NaN propagates as torch.max does),
//             then every query counts the queries that precede it: descending confidence, equal confidences by ascending query index, NaN last
//             (the reference's argsort(descending=True) leaves ties unspecified).  All nq rows are written, no threshold.
//   quirks    kept from the reference: the class loss is normalised by the number of matched PAIRS (max(.., 1)), not by the batch's ground
//             truths; with no pair at all the focal branch is taken even when use_vfl is set; the IoU target is a constant for the gradient.
#include "common.h"

#define DL_GCAP MGDT_DETR_GCAP
#define DL_MAX_NQ MGDT_DETR_MAX_NQ
#define DL_BIG 1e300
#define DL_BIG_COST 1e18f
#define DL_QT 64            // queries of one loss workgroup

__device__ __forceinline__ float dl_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// ================================================================================================ costs + assignment
struct DlMatchArgs {
  const float* boxes; const float* logits; const float* gt_boxes; const int32_t* gt_cls; const int32_t* gt_off;
  float* ws; int32_t* assign; float* cost;
  long ld;
  int layers, batch, nq, nc, G, layer_of_match;
  float g_class, g_bbox, g_giou, alpha, gamma;
};

// bbox_iou(xywh=True, GIoU=True, eps=1e-7) in fp32, the reference's operation order
__device__ __forceinline__ float dl_giou_f32(const float* a, const float* b) {
  const float eps = 1e-7f;
  const float w1_ = a[2] / 2.f, h1_ = a[3] / 2.f, w2_ = b[2] / 2.f, h2_ = b[3] / 2.f;
  const float ax1 = a[0] - w1_, ax2 = a[0] + w1_, ay1 = a[1] - h1_, ay2 = a[1] + h1_;
  const float bx1 = b[0] - w2_, bx2 = b[0] + w2_, by1 = b[1] - h2_, by2 = b[1] + h2_;
  float iw = fminf(ax2, bx2) - fmaxf(ax1, bx1), ih = fminf(ay2, by2) - fmaxf(ay1, by1);
  iw = iw < 0.f ? 0.f : iw;
  ih = ih < 0.f ? 0.f : ih;
  const float inter = iw * ih;
  const float uni = a[2] * a[3] + b[2] * b[3] - inter + eps;
  const float iou = inter / uni;
  const float cw = fmaxf(ax2, bx2) - fminf(ax1, bx1), ch = fmaxf(ay2, by2) - fminf(ay1, by1);
  const float c_area = cw * ch + eps;
  return iou - (c_area - uni) / c_area;
}

__global__ __launch_bounds__(64) void dl_match_kernel(const DlMatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int layer = a.layer_of_match >= 0 ? a.layer_of_match : (int)blockIdx.y;
  const int nq = a.nq, nqp = (nq + 63) & ~63;
  double* v = (double*)smem;                      // [nqp] column potentials
  double* minv = v + nqp;                         // [nqp]
  double* u = minv + nqp;                         // [DL_GCAP] row potentials
  int* way = (int*)(u + DL_GCAP);                 // [nqp]
  int* used = way + nqp;                          // [nqp]
  int* p = used + nqp;                            // [nqp + 1] row of a column, -1 = free; p[nq] = the row being inserted
  int g0 = a.gt_off[b], g1 = a.gt_off[b + 1];
  g0 = max(0, min(g0, a.G));                      // the host checked its copy; the device copy cannot lead outside the arrays either way
  g1 = max(g0, min(g1, a.G));
  int ng = g1 - g0;
  ng = min(ng, min(nq, DL_GCAP));
  const long img = (long)layer * a.batch + b;
  float* C = a.ws + ((long)layer * a.G + g0) * nq;      // [ng][nq]
  // ---- costs
  for (int q = lane; q < nq; q += 64) {
    const float* bx = a.boxes + (img * nq + q) * 4;
    const float pb[4] = {bx[0], bx[1], bx[2], bx[3]};
    const float* lg = a.logits + (img * nq + q) * a.ld;
    for (int g = 0; g < ng; ++g) {
      const float* gp = a.gt_boxes + (long)(g0 + g) * 4;
      const float gb[4] = {gp[0], gp[1], gp[2], gp[3]};
      int cls = a.gt_cls[g0 + g];
      cls = max(0, min(cls, a.nc - 1));
      const float ps = dl_sigmoid(lg[cls]);
      const float om = 1.f - ps;
      const float pg = a.gamma == 2.f ? ps * ps : powf(ps, a.gamma), og = a.gamma == 2.f ? om * om : powf(om, a.gamma);
      const float neg = (1.f - a.alpha) * pg * (-logf(om + 1e-8f));
      const float pos = a.alpha * og * (-logf(ps + 1e-8f));
      const float cc = pos - neg;
      const float cb = ((fabsf(pb[0] - gb[0]) + fabsf(pb[1] - gb[1])) + fabsf(pb[2] - gb[2])) + fabsf(pb[3] - gb[3]);
      const float cg = 1.0f - dl_giou_f32(pb, gb);
      float c = (a.g_class * cc + a.g_bbox * cb) + a.g_giou * cg;
      if (!(fabsf(c) <= 3.0e38f)) c = DL_BIG_COST;
      C[(long)g * nq + q] = c;
      if (a.cost) {
        if (a.layer_of_match >= 0) {
          for (int l = 0; l < a.layers; ++l) a.cost[(((long)l * a.batch + b) * nq + q) * DL_GCAP + g] = c;
        } else {
          a.cost[(img * nq + q) * DL_GCAP + g] = c;
        }
      }
    }
  }
  for (int j = lane; j < nqp; j += 64) { v[j] = 0.; p[j] = -1; }
  for (int i = lane; i < DL_GCAP; i += 64) u[i] = 0.;
  if (lane == 0) p[nqp] = -1;
  __syncthreads();                                // (a lane reads back only the cost entries it stored itself: columns lane + 64 k)
  // ---- shortest augmenting paths, one row (ground truth) after another
  const int m = nq;                               // sentinel column
  for (int i = 0; i < ng; ++i) {
    for (int j = lane; j < nqp; j += 64) { minv[j] = DL_BIG; used[j] = 0; }
    if (lane == 0) p[m] = i;
    __syncthreads();
    int j0 = m;
    bool found = false;
    for (int it = 0; it <= ng; ++it) {            // every pass puts one more column into the tree; a free column ends the path
      if (j0 < m && (j0 & 63) == lane) used[j0] = 1;
      const int i0 = p[j0];
      const double ui0 = u[i0];
      const float* Cr = C + (long)i0 * nq;
      double best = DL_BIG;
      int bj = 0x7fffffff;
      for (int j = lane; j < nq; j += 64) {
        if (!used[j]) {
          const double cur = (double)Cr[j] - ui0 - v[j];
          if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
          const double mj = minv[j];
          if (mj < best) { best = mj; bj = j; }   // ascending j: the lower column on a tie
        }
      }
      for (int off = 32; off; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
      }
      if (bj >= nq) break;                        // no column left (cannot happen with ng <= nq and finite costs)
      const double delta = best;
      for (int j = lane; j < nq; j += 64) {
        if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
        else minv[j] -= delta;
      }
      if (lane == 0) u[i] += delta;
      __syncthreads();
      j0 = bj;
      if (p[j0] < 0) { found = true; break; }
    }
    if (lane == 0 && found) {
      int jj = j0;
      for (int it = 0; it <= ng && jj != m; ++it) { const int j1 = way[jj]; p[jj] = p[j1]; jj = j1; }
    }
    __syncthreads();
  }
  // ---- query-major result: the global ground-truth index or -1
  for (int q = lane; q < nq; q += 64) {
    const int r = p[q];
    const int val = (r >= 0 && r < ng) ? g0 + r : -1;
    if (a.layer_of_match >= 0) {
      for (int l = 0; l < a.layers; ++l) a.assign[((long)l * a.batch + b) * nq + q] = val;
    } else {
      a.assign[img * nq + q] = val;
    }
  }
}

static size_t dl_match_lds(int nq) {
  const size_t nqp = ((size_t)nq + 63) & ~(size_t)63;
  return nqp * 16 + (size_t)DL_GCAP * 8 + nqp * 8 + (nqp + 1) * 4;
}

extern "C" size_t mgdt_detr_match_workspace_bytes(int layers, int G, int nq) {
  if (layers < 1 || G < 0 || nq < 1) return 0;
  return (size_t)layers * (size_t)(G > 0 ? G : 1) * (size_t)nq * sizeof(float);
}

extern "C" int mgdt_detr_match_fwd(const float* boxes, const float* logits, long ld_logits, int layers, int batch, int nq, int nc, const float* gt_boxes,
                                   const int32_t* gt_cls, const int32_t* gt_off_dev, const int32_t* gt_off_host, float g_class, float g_bbox, float g_giou,
                                   float alpha, float gamma, int layer_of_match, void* workspace, size_t workspace_bytes, int32_t* assign, float* cost,
                                   mgdt_stream s) {
  if (!boxes || !logits || !gt_off_dev || !gt_off_host || !assign || !workspace) MGDT_FAIL(MGDT_BAD_ARG, "detr_match: null pointer");
  if (layers < 1 || layers > 65535 || batch < 1 || batch > (1 << 20) || nq < 1 || nq > DL_MAX_NQ || nc < 1 || ld_logits < nc)
    MGDT_FAIL(MGDT_BAD_SHAPE, "detr_match: layers = %d (1..65535), batch = %d, nq = %d (1..%d), nc = %d, logit row stride %ld", layers, batch, nq, DL_MAX_NQ, nc,
              ld_logits);
  if (layer_of_match < -1 || layer_of_match >= layers) MGDT_FAIL(MGDT_BAD_ARG, "detr_match: layer_of_match = %d with %d layers", layer_of_match, layers);
  if (gt_off_host[0] != 0) MGDT_FAIL(MGDT_BAD_ARG, "detr_match: gt_off[0] = %d, not 0", gt_off_host[0]);
  for (int b = 0; b < batch; ++b) {
    const long ng = (long)gt_off_host[b + 1] - gt_off_host[b];
    if (ng < 0) MGDT_FAIL(MGDT_BAD_ARG, "detr_match: gt_off decreases at image %d", b);
    if (ng > nq || ng > DL_GCAP)
      MGDT_FAIL(MGDT_BAD_SHAPE, "detr_match: image %d has %ld ground truths, more than nq = %d or the cap of %d", b, ng, nq, DL_GCAP);
  }
  const int G = gt_off_host[batch];
  if (G > 0 && (!gt_boxes || !gt_cls)) MGDT_FAIL(MGDT_BAD_ARG, "detr_match: null ground truths");
  if (workspace_bytes < mgdt_detr_match_workspace_bytes(layers, G, nq))
    MGDT_FAIL(MGDT_BAD_ARG, "detr_match: workspace of %zu bytes, %zu needed", workspace_bytes, mgdt_detr_match_workspace_bytes(layers, G, nq));
  DlMatchArgs a;
  a.boxes = boxes; a.logits = logits; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_off = gt_off_dev; a.ws = (float*)workspace; a.assign = assign; a.cost = cost;
  a.ld = ld_logits; a.layers = layers; a.batch = batch; a.nq = nq; a.nc = nc; a.G = G; a.layer_of_match = layer_of_match;
  a.g_class = g_class; a.g_bbox = g_bbox; a.g_giou = g_giou; a.alpha = alpha; a.gamma = gamma;
  const dim3 grid(batch, layer_of_match >= 0 ? 1 : layers);
  dl_match_kernel<<<grid, 64, dl_match_lds(nq), (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("detr_match_fwd");
  return MGDT_OK;
}

// ================================================================================================ losses + head gradients
struct DlLossArgs {
  const float* boxes; const float* logits; const float* gt_boxes; const int32_t* gt_cls; const int32_t* assign;
  unsigned* counter; unsigned long long* part;
  float* out; float* gt_score; float* d_boxes; float* d_logits;
  long ld;
  int layers, batch, nq, nc, G, nblk, vfl;
  double s_class, s_bbox, s_giou;     // gain / normaliser of the three losses
  double gscale;
};

__device__ __forceinline__ double dl_wave_sum(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

__global__ __launch_bounds__(256) void dl_loss_kernel(const DlLossArgs a) {
  __shared__ float sc[DL_QT];
  __shared__ int lab[DL_QT];
  __shared__ double red[3][4];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qb = blockIdx.x, b = blockIdx.y, l = blockIdx.z;
  const int nq = a.nq, nc = a.nc, q0 = qb * DL_QT;
  const long img = (long)l * a.batch + b;
  double s_cls = 0., s_l1 = 0., s_gi = 0.;
  if (tid < DL_QT) {
    const int q = q0 + tid;
    float score = 0.f;
    int label = -1;
    if (q < nq) {
      const long row = img * nq + q;
      const int g = a.assign[row];
      double db[4] = {0., 0., 0., 0.};
      if (g >= 0 && g < a.G) {
        int cls = a.gt_cls[g];
        label = max(0, min(cls, nc - 1));
        const float* pp = a.boxes + row * 4;
        const float* gp = a.gt_boxes + (long)g * 4;
        const double x = pp[0], y = pp[1], w = pp[2], h = pp[3], X = gp[0], Y = gp[1], W = gp[2], H = gp[3];
        const double eps = 1e-7;
        const double ax1 = x - w / 2, ax2 = x + w / 2, ay1 = y - h / 2, ay2 = y + h / 2;
        const double bx1 = X - W / 2, bx2 = X + W / 2, by1 = Y - H / 2, by2 = Y + H / 2;
        const double iwr = fmin(ax2, bx2) - fmax(ax1, bx1), ihr = fmin(ay2, by2) - fmax(ay1, by1);
        const double iw = iwr < 0. ? 0. : iwr, ih = ihr < 0. ? 0. : ihr;
        const double inter = iw * ih;
        const double uni = w * h + W * H - inter + eps;
        const double iou = inter / uni;
        const double cw = fmax(ax2, bx2) - fmin(ax1, bx1), ch = fmax(ay2, by2) - fmin(ay1, by1);
        const double c_area = cw * ch + eps;
        const double giou = iou - (c_area - uni) / c_area;
        score = (float)iou;
        s_l1 = fabs(x - X) + fabs(y - Y) + fabs(w - W) + fabs(h - H);
        s_gi = 1.0 - giou;
        if (a.d_boxes) {
          // giou = inter / uni - 1 + uni / c_area with uni = w h + W H - inter + eps
          const double gU = -inter / (uni * uni) + 1.0 / c_area;      // d giou / d uni
          const double gI = 1.0 / uni - gU;                           // d giou / d inter (through uni as well)
          const double gC = -uni / (c_area * c_area);                 // d giou / d c_area
          const double g_iw = iwr >= 0. ? gI * ih : 0., g_ih = ihr >= 0. ? gI * iw : 0.;
          const double g_cw = gC * ch, g_ch = gC * cw;
          // minimum / maximum pass the gradient to the smaller / larger argument, half each on a tie (torch.minimum / maximum)
          const double mnx2 = ax2 < bx2 ? 1. : (ax2 == bx2 ? .5 : 0.), mxx1 = ax1 > bx1 ? 1. : (ax1 == bx1 ? .5 : 0.);
          const double mny2 = ay2 < by2 ? 1. : (ay2 == by2 ? .5 : 0.), mxy1 = ay1 > by1 ? 1. : (ay1 == by1 ? .5 : 0.);
          const double mxx2 = ax2 > bx2 ? 1. : (ax2 == bx2 ? .5 : 0.), mnx1 = ax1 < bx1 ? 1. : (ax1 == bx1 ? .5 : 0.);
          const double mxy2 = ay2 > by2 ? 1. : (ay2 == by2 ? .5 : 0.), mny1 = ay1 < by1 ? 1. : (ay1 == by1 ? .5 : 0.);
          const double d_ax2 = g_iw * mnx2 + g_cw * mxx2, d_ax1 = -g_iw * mxx1 - g_cw * mnx1;
          const double d_ay2 = g_ih * mny2 + g_ch * mxy2, d_ay1 = -g_ih * mxy1 - g_ch * mny1;
          const double dg[4] = {d_ax1 + d_ax2, d_ay1 + d_ay2, (d_ax2 - d_ax1) / 2 + gU * h, (d_ay2 - d_ay1) / 2 + gU * w};
          const double dv[4] = {x - X, y - Y, w - W, h - H};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double sg = dv[e] > 0. ? 1. : (dv[e] < 0. ? -1. : 0.);
            db[e] = a.gscale * (a.s_bbox * sg - a.s_giou * dg[e]);
          }
        }
      }
      a.gt_score[row] = score;
      if (a.d_boxes) {
        f32x4 o = {(float)db[0], (float)db[1], (float)db[2], (float)db[3]};
        *(f32x4*)(a.d_boxes + row * 4) = o;
      }
    }
    sc[tid] = score;
    lab[tid] = label;
  }
  __syncthreads();
  // ---- class terms: element e = (query e / nc, class e % nc) of this workgroup's rows, contiguous in memory when ld == nc
  const int nrow = min(DL_QT, nq - q0);
  const float gcls = (float)(a.gscale * a.s_class);
  for (int e = tid; e < nrow * nc; e += 256) {
    const int r = e / nc, c = e - r * nc;
    const long row = img * nq + q0 + r;
    const float x = a.logits[row * a.ld + c];
    const float sg = dl_sigmoid(x);
    const float yl = lab[r] == c ? 1.f : 0.f;
    const float gs = sc[r];
    const float sp = fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));      // softplus(x): binary_cross_entropy_with_logits(x, t) = softplus(x) - x t
    float loss, grad;
    if (a.vfl) {
      const float t = gs * yl;
      const float bce = sp - x * t;
      const float wgt = 0.75f * (sg * sg) * (1.f - yl) + gs * yl;
      loss = bce * wgt;
      grad = (1.5f * sg * sg * (1.f - sg) * (1.f - yl)) * bce + wgt * (sg - t);
    } else {
      const float bce = sp - x * yl;
      const float pt = yl * sg + (1.f - yl) * (1.f - sg);
      const float om = 1.f - pt, rt = sqrtf(om);
      const float md = om * rt;                                       // (1 - p_t) ** 1.5
      const float af = yl * 0.25f + (1.f - yl) * 0.75f;
      const float dom = (1.f - 2.f * yl) * sg * (1.f - sg);           // d (1 - p_t) / dx
      loss = bce * md * af;
      grad = af * (md * (sg - yl) + bce * 1.5f * rt * dom);
    }
    s_cls += (double)loss;
    if (a.d_logits) a.d_logits[row * nc + c] = gcls * grad;
  }
  // ---- workgroup partial: lanes by butterfly, waves in sequence
  s_cls = dl_wave_sum(s_cls); s_l1 = dl_wave_sum(s_l1); s_gi = dl_wave_sum(s_gi);
  if (lane == 0) { red[0][wave] = s_cls; red[1][wave] = s_l1; red[2][wave] = s_gi; }
  __syncthreads();
  if (tid == 0) {
    const long blk = (long)b * gridDim.x + qb;
    unsigned long long* pp = a.part + ((long)l * a.nblk + blk) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double t = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
      const unsigned long long prev = __hip_atomic_exchange(pp + k, (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("" ::"v"(prev));                                   // the returned value is waited for: the exchange has been performed
    }
    const unsigned total = gridDim.x * gridDim.y * gridDim.z;
    const unsigned old = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == total - 1u;
    if (old == total - 1u) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // at rest again for the next call
  }
  __syncthreads();
  if (!last) return;
  // ---- the last workgroup: every layer's three sums, partials strided over the threads, then the same butterfly + sequence
  double aux[3] = {0., 0., 0.};                                       // thread 0: the auxiliary layers' sum (every layer but the last), in layer order
  for (int o = 0; o < a.layers * 3; ++o) {
    const int ll = o / 3, k = o - ll * 3;
    double t = 0.;
    for (int i = tid; i < a.nblk; i += 256)
      t += __longlong_as_double((long long)__hip_atomic_load(a.part + ((long)ll * a.nblk + i) * 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    t = dl_wave_sum(t);
    __syncthreads();
    if (lane == 0) red[0][wave] = t;
    __syncthreads();
    if (tid == 0) {
      const double tot = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
      const double sk = k == 0 ? a.s_class : (k == 1 ? a.s_bbox : a.s_giou);
      a.out[o] = (float)(tot * sk);
      if (ll < a.layers - 1) aux[k] += tot * sk;
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out[a.layers * 3 + k] = (float)aux[k];
  }
}

extern "C" size_t mgdt_detr_loss_workspace_bytes(int layers, int batch, int nq) {
  if (layers < 1 || batch < 1 || nq < 1) return 0;
  return 16 + (size_t)layers * batch * cdiv(nq, DL_QT) * 3 * sizeof(double);
}

extern "C" int mgdt_detr_loss_fwd(const float* boxes, const float* logits, long ld_logits, int layers, int batch, int nq, int nc, const float* gt_boxes,
                                  const int32_t* gt_cls, int G, const int32_t* assign, long num_pairs, float g_class, float g_bbox, float g_giou, int use_vfl,
                                  float gscale, void* workspace, size_t workspace_bytes, float* out, float* gt_score, float* d_boxes, float* d_logits,
                                  mgdt_stream s) {
  if (!boxes || !logits || !assign || !out || !gt_score || !workspace) MGDT_FAIL(MGDT_BAD_ARG, "detr_loss: null pointer");
  if (layers < 1 || layers > 65535 || batch < 1 || batch > 65535 || nq < 1 || nq > (1 << 24) || nc < 1 || nc > (1 << 20) || ld_logits < nc)
    MGDT_FAIL(MGDT_BAD_SHAPE, "detr_loss: layers = %d, batch = %d (1..65535 each), nq = %d, nc = %d, logit row stride %ld", layers, batch, nq, nc, ld_logits);
  if (G < 0 || num_pairs < 0 || (G > 0 && (!gt_boxes || !gt_cls))) MGDT_FAIL(MGDT_BAD_ARG, "detr_loss: G = %d, num_pairs = %ld, or null ground truths", G, num_pairs);
  if ((d_boxes == nullptr) != (d_logits == nullptr)) MGDT_FAIL(MGDT_BAD_ARG, "detr_loss: both gradient pointers or neither");
  if (((uintptr_t)workspace % 16) || ((uintptr_t)d_boxes % 16)) MGDT_FAIL(MGDT_BAD_ARG, "detr_loss: workspace and d_boxes 16-byte aligned");
  if (workspace_bytes < mgdt_detr_loss_workspace_bytes(layers, batch, nq))
    MGDT_FAIL(MGDT_BAD_ARG, "detr_loss: workspace of %zu bytes, %zu needed", workspace_bytes, mgdt_detr_loss_workspace_bytes(layers, batch, nq));
  DlLossArgs a;
  a.boxes = boxes; a.logits = logits; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.assign = assign;
  a.counter = (unsigned*)workspace; a.part = (unsigned long long*)((char*)workspace + 16);
  a.out = out; a.gt_score = gt_score; a.d_boxes = d_boxes; a.d_logits = d_logits;
  a.ld = ld_logits; a.layers = layers; a.batch = batch; a.nq = nq; a.nc = nc; a.G = G; a.nblk = batch * cdiv(nq, DL_QT);
  a.vfl = (use_vfl && num_pairs > 0) ? 1 : 0;
  a.s_class = (double)g_class / (double)(num_pairs > 0 ? num_pairs : 1);
  a.s_bbox = num_pairs > 0 ? (double)g_bbox / (double)num_pairs : 0.;
  a.s_giou = num_pairs > 0 ? (double)g_giou / (double)num_pairs : 0.;
  a.gscale = (double)gscale;
  const dim3 grid(cdiv(nq, DL_QT), batch, layers);
  dl_loss_kernel<<<grid, 256, 0, (hipStream_t)s>>>(a);
  MGDT_CHECK_LAUNCH("detr_loss_fwd");
  return MGDT_OK;
}

// ================================================================================================ validator rows
__global__ __launch_bounds__(256) void dl_val_post_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, int nq, int nc,
                                                          const float* __restrict__ wh, float* __restrict__ rows, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* conf = (float*)smem;                     // [nq]
  int* cl = (int*)(conf + nq);                    // [nq]
  const int b = blockIdx.x, tid = threadIdx.x;
  const float sw = wh ? wh[2 * b] : 1.f, sh = wh ? wh[2 * b + 1] : 1.f;
  for (int q = tid; q < nq; q += 256) {
    const float* sr = scores + ((long)b * nq + q) * nc;
    float best = sr[0];
    int cls = 0;
    for (int c = 1; c < nc; ++c) {
      const float vv = sr[c];
      if (vv > best || (vv != vv && best == best)) { best = vv; cls = c; }      // the first NaN wins, as torch.max returns it
    }
    conf[q] = best;
    cl[q] = cls;
  }
  __syncthreads();
  for (int q = tid; q < nq; q += 256) {
    const float mine = conf[q];
    const bool mnan = mine != mine;
    int rank = 0;
    for (int o = 0; o < nq; ++o) {
      const float ov = conf[o];
      const bool onan = ov != ov;
      const bool before = mnan ? (!onan || o < q) : (!onan && (ov > mine || (ov == mine && o < q)));
      rank += before ? 1 : 0;
    }
    const float* bx = boxes + ((long)b * nq + q) * 4;
    const float dw = bx[2] / 2.f, dh = bx[3] / 2.f;                              // ops.xywh2xyxy
    float* o = rows + ((long)b * nq + rank) * 6;
    o[0] = (bx[0] - dw) * sw; o[1] = (bx[1] - dh) * sh; o[2] = (bx[0] + dw) * sw; o[3] = (bx[1] + dh) * sh;
    o[4] = mine; o[5] = (float)cl[q];
  }
  if (tid == 0) counts[b] = nq;
}

extern "C" int mgdt_rtdetr_val_post_fwd(const float* boxes, const float* scores, int batch, int nq, int nc, const float* wh, float* rows, int32_t* counts,
                                        mgdt_stream s) {
  if (!boxes || !scores || !rows || !counts) MGDT_FAIL(MGDT_BAD_ARG, "rtdetr_val_post: null pointer");
  if (batch < 1 || nq < 1 || nq > MGDT_RTDETR_VAL_MAX_NQ || nc < 1)
    MGDT_FAIL(MGDT_BAD_SHAPE, "rtdetr_val_post: batch = %d, nq = %d (1..%d), nc = %d", batch, nq, MGDT_RTDETR_VAL_MAX_NQ, nc);
  dl_val_post_kernel<<<batch, 256, (size_t)nq * 8, (hipStream_t)s>>>(boxes, scores, nq, nc, wh, rows, counts);
  MGDT_CHECK_LAUNCH("rtdetr_val_post_fwd");
  return MGDT_OK;
}
