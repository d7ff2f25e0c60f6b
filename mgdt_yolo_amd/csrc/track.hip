// ByteTrack (reference tracker/trackers/byte_tracker.py:181-295 BYTETracker.update, tracker/utils/kalman_filter.py KalmanFilterXYAH,
// tracker/utils/matching.py) for B video streams in one launch: one workgroup of ONE wave per stream, the phases of a frame separated by workgroup
// barriers (with a single wave they cost nothing, and every list below is built and read by the same 64 lanes).
//
//   state   per stream tk_state_bytes(cap) bytes: int32 {frame_id, id counter, 0, 0}, then structure-of-arrays over the cap slots:
//           fp64 mean[8], fp64 cov[12] (the 8x8 filter decouples into four 2x2 blocks, coordinate i with its velocity: P[i][i], P[i][i+4], P[i+4][i+4];
//           every other entry of the reference's matrix is exactly 0), int32 id, state (0 free, 1 Tracked, 2 Lost, 3 Removed), is_activated, frame_id,
//           start_frame, tracklet_len, rem (the id is in the reference's removed_stracks), fp32 score, cls, idx.
//           The kernel works on an LDS copy and writes it back only when the frame fits: on overflow the state stays as it was.
//   costs   fp32 in the reference's operation order (this file is built with -ffp-contract=off): the fp64 state as tlbr cast to fp32, a detection as
//           STrack keeps it (_tlwh = float32(x2 - x1), tlbr = x1 + w), bbox_ious with eps 1e-7, 1 - iou, fused 1 - (1 - cost) * score.
//   solver  the reference calls lap.lapjv(cost, extend_cost=True, cost_limit=t): minimise sum(c_ij - t) over a partial matching.  Here: shortest
//           augmenting paths, rows in sequence, the column scan two columns per lane, fp64 potentials; every row owns a zero-cost dummy column (stay
//           unmatched), pairs with c_ij >= t are no edges.  Exact for the fp32 cost values up to fp64 rounding of path sums.
//   quirk   kept from the reference: :288 subtracts removed_stracks from the lost list before :290 extends it, so a lost track removed after the
//           buffer stays in the lost list in state Removed until the end of the NEXT frame (it is in the duplicate check, and in the next pool, where
//           a match re-activates it); once its id is in removed_stracks it leaves the lost list whenever it is in it again.
#include "common.h"

#define TK_CAP 128          // most slots per stream, most detections above track_low_thresh per frame, most rows / columns of one assignment
#define TK_LD 128
#define TK_BIG 1e300
#define TK_FLAG_DETS 1
#define TK_FLAG_TRACKS 2
#define TK_W_POS (1. / 20)
#define TK_W_VEL (1. / 160)

__host__ __device__ static inline size_t tk_state_bytes(int cap) { return 16 + (size_t)200 * cap; }

struct TkState {      // views into one stream's state (global or its LDS copy)
  int32_t* hdr; double* mean; double* cov; int32_t *id, *state, *act, *fid, *start, *tlen, *rem; float *score, *cls, *idx; int T;
  __device__ __forceinline__ TkState(char* base, int cap) : T(cap) {
    hdr = (int32_t*)base;
    mean = (double*)(base + 16);
    cov = mean + 8 * cap;
    id = (int32_t*)(cov + 12 * cap);
    state = id + cap; act = state + cap; fid = act + cap; start = fid + cap; tlen = start + cap; rem = tlen + cap;
    score = (float*)(rem + cap); cls = score + cap; idx = cls + cap;
  }
  __device__ __forceinline__ void tlbr(int t, float* o) const {      // STrack.tlwh / .tlbr in fp64, then the cast of np.ascontiguousarray(dtype=float32)
    const double a = mean[2 * T + t], h = mean[3 * T + t];
    const double w = a * h;
    const double x1 = mean[t] - w / 2, y1 = mean[T + t] - h / 2;
    o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)(w + x1); o[3] = (float)(h + y1);
  }
};

__device__ __forceinline__ float tk_iou_cost(const float* a, const float* b) {      // matching.py:199-229 (box1 = a, box2 = b), then 1 - iou
  float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  iw = iw < 0.f ? 0.f : iw;
  ih = ih < 0.f ? 0.f : ih;
  const float inter = iw * ih;
  const float a1 = (a[2] - a[0]) * (a[3] - a[1]), a2 = (b[2] - b[0]) * (b[3] - b[1]);
  return 1.f - inter / (a2 + a1 - inter + 1e-7f);
}

// x[i] = column of row i or -1.  C: LDS, TK_LD floats per row; u[TK_CAP], p[TK_CAP + 1], way[TK_CAP], x[TK_CAP]: LDS.  n, m <= TK_CAP.  All 64 lanes.
__device__ void tk_solve(const float* C, int n, int m, float thresh, double* u, int* p, int* way, int* x, int lane) {
  for (int i = lane; i < TK_CAP; i += 64) { u[i] = 0.; x[i] = -1; }
  for (int j = lane; j <= TK_CAP; j += 64) p[j] = -1;
  double v[2] = {0., 0.};
  __syncthreads();
  if (n <= 0 || m <= 0) return;
  const double th = (double)thresh;
  for (int i = 0; i < n; ++i) {
    if (lane == 0) p[m] = i;
    __syncthreads();
    int j0 = m, way_d = m;
    double minv[2] = {TK_BIG, TK_BIG}, minv_d = TK_BIG;
    bool used[2] = {false, false}, term = false;
    for (int it = 0; it <= m; ++it) {      // every pass puts one more column into the tree or ends the path
      if (j0 < m && (j0 & 63) == lane) { if (j0 < 64) used[0] = true; else used[1] = true; }
      const int i0 = p[j0];
      const double ui0 = u[i0];
      if (-ui0 < minv_d) { minv_d = -ui0; way_d = j0; }
      double best = TK_BIG;
      int bj = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        if (j < m && !used[k]) {
          const float c = C[i0 * TK_LD + j];
          if (c < thresh) {
            const double cur = ((double)c - th) - ui0 - v[k];
            if (cur < minv[k]) { minv[k] = cur; way[j] = j0; }
          }
          if (minv[k] < best) { best = minv[k]; bj = j; }
        }
      }
      for (int off = 32; off; off >>= 1) {      // first minimum: the lower column on a tie
        const double ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
      }
      term = !(best < minv_d) || it == m;
      const double delta = term ? minv_d : best;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        if (j < m) {
          if (used[k]) { u[p[j]] += delta; v[k] -= delta; }
          else minv[k] -= delta;
        }
      }
      if (lane == 0) u[i] += delta;
      minv_d -= delta;
      __syncthreads();
      if (term) break;
      j0 = bj;
      if (p[j0] < 0) break;
    }
    if (lane == 0) {
      int jj = term ? way_d : j0;
      for (int it = 0; it <= m && jj != m; ++it) { const int j1 = way[jj]; p[jj] = p[j1]; jj = j1; }
    }
    __syncthreads();
  }
  for (int j = lane; j < m; j += 64)
    if (p[j] >= 0) x[p[j]] = j;
  __syncthreads();
}

// ascending list of the k < n with pred(k); entries past TK_CAP are counted, not stored
template <class Pred>
__device__ __forceinline__ int tk_compact(int n, int* list, int at, int lane, Pred pred) {
  int cnt = at;
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool f = k < n && pred(k);
    const unsigned long long mask = __ballot(f);
    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    if (f && pos < TK_CAP) list[pos] = k;
    cnt += __popcll(mask);
  }
  return cnt;
}

struct TkCfg { float high, low, newt, match; int max_time_lost; };

__global__ __launch_bounds__(64) void bytetrack_update_kernel(const float* __restrict__ rows, const int32_t* __restrict__ counts,
                                                              const uint8_t* __restrict__ active, char* __restrict__ state, int T, int max_det, TkCfg cfg,
                                                              float* __restrict__ tracks, int32_t* __restrict__ ntracks, int32_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t sb = tk_state_bytes(T);
  float* C = (float*)smem;
  char* sm = smem + TK_CAP * TK_LD * 4;
  TkState S(sm, T);
  sm += (sb + 15) & ~(size_t)15;
  double* u = (double*)sm; sm += TK_CAP * 8;
  int* p = (int*)sm; sm += (TK_CAP + 4) * 4;
  int* way = (int*)sm; sm += TK_CAP * 4;
  int* x = (int*)sm; sm += TK_CAP * 4;
  int* ra = (int*)sm; sm += TK_CAP * 4;
  int* rb = (int*)sm; sm += TK_CAP * 4;
  int* dl = (int*)sm; sm += TK_CAP * 4;
  int* colmap = (int*)sm; sm += TK_CAP * 4;
  int* colused = (int*)sm; sm += TK_CAP * 4;
  int* st0 = (int*)sm; sm += TK_CAP * 4;
  int* mark = (int*)sm; sm += TK_CAP * 4;
  int* dupm = (int*)sm; sm += TK_CAP * 4;
  float* dsc = (float*)sm; sm += TK_CAP * 4;
  float* dbox = (float*)sm; sm += TK_CAP * 16;
  float* dz = (float*)sm; sm += TK_CAP * 16;
  float* tb = (float*)sm;

  char* G = state + (size_t)b * sb;
  float* out = tracks + (size_t)b * T * 8;
  if (active && !active[b]) {      // the reference hook skips the update of a frame without detections: nothing of this stream moves
    for (int e = lane; e < T * 8; e += 64) out[e] = 0.f;
    if (lane == 0) { ntracks[b] = 0; flags[b] = 0; }
    return;
  }
  for (int w = lane; w < (int)(sb / 4); w += 64) ((uint32_t*)S.hdr)[w] = ((const uint32_t*)G)[w];
  for (int t = lane; t < TK_CAP; t += 64) { colused[t] = 0; mark[t] = 0; dupm[t] = 0; }
  __syncthreads();
  const int fid = S.hdr[0] + 1, count0 = S.hdr[1];
  for (int t = lane; t < T; t += 64) st0[t] = S.state[t];

  // ---- detections: high (> track_high_thresh) first, then second (> low and < high), each in ascending row order ----
  const float* R = rows + (size_t)b * max_det * 6;
  const int nd = min(max(counts[b], 0), max_det);
  const int nh = tk_compact(nd, dl, 0, lane, [&](int d) { return R[d * 6 + 4] > cfg.high; });
  const int ndet = tk_compact(nd, dl, nh, lane, [&](int d) { const float s = R[d * 6 + 4]; return s > cfg.low && s < cfg.high; });
  int flag = ndet > TK_CAP ? TK_FLAG_DETS : 0;
  __syncthreads();
  if (!flag) {
    const int ns = ndet - nh;
    for (int k = lane; k < ndet; k += 64) {
      const float* r = R + dl[k] * 6;
      const float x1 = r[0], y1 = r[1], w = r[2] - x1, h = r[3] - y1;
      dbox[k * 4] = x1; dbox[k * 4 + 1] = y1; dbox[k * 4 + 2] = x1 + w; dbox[k * 4 + 3] = y1 + h;
      dz[k * 4] = x1 + w / 2.f; dz[k * 4 + 1] = y1 + h / 2.f; dz[k * 4 + 2] = w / h; dz[k * 4 + 3] = h;
      dsc[k] = r[4];
    }
    // a matched track takes the detection: STrack.update / re_activate (byte_tracker.py:79-111) with KalmanFilterXYAH.update, the innovation
    // covariance diagonal (no Cholesky): per coordinate S = P_pp + r, K = [P_pp, P_pv] / S
    auto hit = [&](int t, int k) {
      const int d = dl[k];
      S.tlen[t] = S.state[t] == 1 ? S.tlen[t] + 1 : 0;
      const double h = S.mean[3 * T + t];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double pp = S.cov[(3 * i) * T + t], pv = S.cov[(3 * i + 1) * T + t], vv = S.cov[(3 * i + 2) * T + t];
        const double r = i == 2 ? 1e-1 * 1e-1 : (TK_W_POS * h) * (TK_W_POS * h);
        const double Sv = pp + r, kp = pp / Sv, kv = pv / Sv;
        const double inn = (double)dz[k * 4 + i] - S.mean[i * T + t];
        S.mean[i * T + t] += inn * kp;
        S.mean[(i + 4) * T + t] += inn * kv;
        S.cov[(3 * i) * T + t] = pp - kp * Sv * kp;
        S.cov[(3 * i + 1) * T + t] = pv - kp * Sv * kv;
        S.cov[(3 * i + 2) * T + t] = vv - kv * Sv * kv;
      }
      S.state[t] = 1; S.act[t] = 1; S.fid[t] = fid;
      S.score[t] = R[d * 6 + 4]; S.cls[t] = R[d * 6 + 5]; S.idx[t] = (float)d;
    };

    // ---- pool = activated Tracked + the lost list; multi_predict (mean[7] of a non-Tracked track zeroed) ----
    const int np_ = tk_compact(T, ra, 0, lane, [&](int t) { return (st0[t] == 1 && S.act[t] != 0) || st0[t] == 2 || st0[t] == 3; });
    __syncthreads();
    for (int r = lane; r < np_; r += 64) {
      const int t = ra[r];
      if (S.state[t] != 1) S.mean[7 * T + t] = 0.;
      const double h = S.mean[3 * T + t];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double pp = S.cov[(3 * i) * T + t], pv = S.cov[(3 * i + 1) * T + t], vv = S.cov[(3 * i + 2) * T + t];
        const double sp = i == 2 ? 1e-2 : TK_W_POS * h, sv = i == 2 ? 1e-5 : TK_W_VEL * h;
        S.cov[(3 * i) * T + t] = (pp + pv) + (pv + vv) + sp * sp;
        S.cov[(3 * i + 1) * T + t] = pv + vv;
        S.cov[(3 * i + 2) * T + t] = vv + sv * sv;
        S.mean[i * T + t] = S.mean[i * T + t] + S.mean[(i + 4) * T + t];
      }
    }
    __syncthreads();
    for (int t = lane; t < T; t += 64)
      if (S.state[t] != 0) S.tlbr(t, tb + t * 4);
    __syncthreads();

    // ---- first association: pool x high, fused cost, match_thresh ----
    for (int r = 0; r < np_; ++r)
      for (int c = lane; c < nh; c += 64) C[r * TK_LD + c] = 1.f - (1.f - tk_iou_cost(tb + ra[r] * 4, dbox + c * 4)) * dsc[c];
    __syncthreads();
    tk_solve(C, np_, nh, cfg.match, u, p, way, x, lane);
    for (int r = lane; r < np_; r += 64)
      if (x[r] >= 0) { hit(ra[r], x[r]); colused[x[r]] = 1; }
    __syncthreads();

    // ---- second: the unmatched Tracked tracks of the pool x second detections, IoU distance, 0.5; still unmatched: Lost ----
    const int n2 = tk_compact(np_, rb, 0, lane, [&](int r) { return x[r] < 0 && st0[ra[r]] == 1; });
    __syncthreads();
    for (int r = lane; r < n2; r += 64) rb[r] = ra[rb[r]];
    __syncthreads();
    for (int r = 0; r < n2; ++r)
      for (int c = lane; c < ns; c += 64) C[r * TK_LD + c] = tk_iou_cost(tb + rb[r] * 4, dbox + (nh + c) * 4);
    __syncthreads();
    tk_solve(C, n2, ns, 0.5f, u, p, way, x, lane);
    for (int r = lane; r < n2; r += 64) {
      if (x[r] >= 0) hit(rb[r], nh + x[r]);
      else S.state[rb[r]] = 2;
    }
    __syncthreads();

    // ---- unconfirmed (Tracked, never activated; not predicted) x the left-over high detections, fused cost, 0.7; unmatched: removed ----
    const int n3 = tk_compact(T, ra, 0, lane, [&](int t) { return st0[t] == 1 && S.act[t] == 0; });
    const int m3 = tk_compact(nh, colmap, 0, lane, [&](int k) { return colused[k] == 0; });
    __syncthreads();
    for (int r = 0; r < n3; ++r)
      for (int c = lane; c < m3; c += 64) C[r * TK_LD + c] = 1.f - (1.f - tk_iou_cost(tb + ra[r] * 4, dbox + colmap[c] * 4)) * dsc[colmap[c]];
    __syncthreads();
    tk_solve(C, n3, m3, 0.7f, u, p, way, x, lane);
    for (int r = lane; r < n3; r += 64) {
      if (x[r] >= 0) { hit(ra[r], colmap[x[r]]); colused[colmap[x[r]]] = 1; }
      else S.state[ra[r]] = 0;
    }
    __syncthreads();

    // ---- new tracks in ascending detection order where not score < new_track_thresh; a free slot each, or the frame does not fit ----
    const int nnew = tk_compact(m3, rb, 0, lane, [&](int c) { return colused[colmap[c]] == 0 && !(dsc[colmap[c]] < cfg.newt); });
    const int nfree = tk_compact(T, way, 0, lane, [&](int t) { return S.state[t] == 0; });
    __syncthreads();
    if (nnew > nfree) flag = TK_FLAG_TRACKS;
    if (!flag) {
      for (int q = lane; q < nnew; q += 64) {      // STrack.activate + KalmanFilterXYAH.initiate
        const int t = way[q], k = colmap[rb[q]], d = dl[k];
        const double h = (double)dz[k * 4 + 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double sp = i == 2 ? 1e-2 : (2 * TK_W_POS) * h, sv = i == 2 ? 1e-5 : (10 * TK_W_VEL) * h;
          S.mean[i * T + t] = (double)dz[k * 4 + i];
          S.mean[(i + 4) * T + t] = 0.;
          S.cov[(3 * i) * T + t] = sp * sp; S.cov[(3 * i + 1) * T + t] = 0.; S.cov[(3 * i + 2) * T + t] = sv * sv;
        }
        S.id[t] = count0 + 1 + q;
        S.state[t] = 1; S.act[t] = fid == 1 ? 1 : 0; S.fid[t] = fid; S.start[t] = fid; S.tlen[t] = 0; S.rem[t] = 0;
        S.score[t] = R[d * 6 + 4]; S.cls[t] = R[d * 6 + 5]; S.idx[t] = (float)d;
      }
      if (lane == 0) { S.hdr[0] = fid; S.hdr[1] = count0 + nnew; }
      __syncthreads();
      // ---- the lost list: Removed after the buffer (and kept one more frame, see the head of the file); out at once when the id was removed before ----
      for (int t = lane; t < T; t += 64) {
        const int st = S.state[t];
        if (st == 2 || st == 3) {
          const int m_ = st0[t] != 1 && fid - S.fid[t] > cfg.max_time_lost;
          if (m_) S.state[t] = 3;
          if (S.rem[t] != 0) S.state[t] = 0;
          mark[t] = m_;
        }
      }
      __syncthreads();
      // ---- remove_duplicate_stracks: Tracked x lost list, IoU distance < 0.15; the longer-lived stays, the tracked one goes on a tie ----
      for (int t = lane; t < T; t += 64)
        if (S.state[t] != 0) S.tlbr(t, tb + t * 4);
      __syncthreads();
      for (int a = lane; a < T; a += 64) {
        if (S.state[a] != 1) continue;
        const int timep = S.fid[a] - S.start[a];
        for (int q = 0; q < T; ++q) {
          if (S.state[q] != 2 && S.state[q] != 3) continue;
          if (tk_iou_cost(tb + a * 4, tb + q * 4) < 0.15f) {
            if (timep > S.fid[q] - S.start[q]) dupm[q] = 1;
            else dupm[a] = 1;
          }
        }
      }
      __syncthreads();
      for (int t = lane; t < T; t += 64) {
        if (dupm[t]) S.state[t] = 0;
        else if (mark[t] && S.state[t] != 0) S.rem[t] = 1;
      }
      __syncthreads();
    }
  }

  // ---- rows of the activated Tracked tracks in ascending id; the state goes back only when the frame fitted ----
  int nout = 0;
  if (!flag) {
    for (int base = 0; base < T; base += 64) {
      const int t = base + lane;
      const bool o = t < T && S.state[t] == 1 && S.act[t] != 0;
      if (o) {
        int rank = 0;
        for (int q = 0; q < T; ++q) rank += (S.state[q] == 1 && S.act[q] != 0 && S.id[q] < S.id[t]) ? 1 : 0;
        float bx[4];
        S.tlbr(t, bx);
        float* r = out + rank * 8;
        r[0] = bx[0]; r[1] = bx[1]; r[2] = bx[2]; r[3] = bx[3];
        r[4] = (float)S.id[t]; r[5] = S.score[t]; r[6] = S.cls[t]; r[7] = S.idx[t];
      }
      nout += __popcll(__ballot(o));
    }
    for (int w = lane; w < (int)(sb / 4); w += 64) ((uint32_t*)G)[w] = ((const uint32_t*)S.hdr)[w];
  }
  for (int e = nout * 8 + lane; e < T * 8; e += 64) out[e] = 0.f;
  if (lane == 0) { ntracks[b] = nout; flags[b] = flag; }
}

__global__ __launch_bounds__(64) void track_assign_kernel(const float* __restrict__ cost, const int32_t* __restrict__ n, const int32_t* __restrict__ m,
                                                          int n_max, int m_max, float thresh, int32_t* __restrict__ xo) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x, lane = threadIdx.x;
  float* C = (float*)smem;
  char* sm = smem + TK_CAP * TK_LD * 4;
  double* u = (double*)sm; sm += TK_CAP * 8;
  int* p = (int*)sm; sm += (TK_CAP + 4) * 4;
  int* way = (int*)sm; sm += TK_CAP * 4;
  int* x = (int*)sm;
  const int nn = min(max(n[b], 0), n_max), mm = min(max(m[b], 0), m_max);
  const float* A = cost + (size_t)b * n_max * m_max;
  for (int r = 0; r < nn; ++r)
    for (int c = lane; c < mm; c += 64) C[r * TK_LD + c] = A[(size_t)r * m_max + c];
  __syncthreads();
  tk_solve(C, nn, mm, thresh, u, p, way, x, lane);
  for (int i = lane; i < n_max; i += 64) xo[(size_t)b * n_max + i] = i < nn ? x[i] : -1;
}

// live tracks of one stream in ascending id
__global__ __launch_bounds__(TK_CAP) void bytetrack_export_kernel(char* __restrict__ state, int T, int32_t* __restrict__ hdr, int32_t* __restrict__ ints,
                                                                  float* __restrict__ score_cls, double* __restrict__ mean, double* __restrict__ cov) {
  TkState S(state, T);
  const int t = threadIdx.x;
  const bool live = t < T && S.state[t] != 0;
  const int nlive = __syncthreads_count(live);
  if (t == 0) { hdr[0] = nlive; hdr[1] = S.hdr[0]; hdr[2] = S.hdr[1]; }
  if (!live) return;
  int k = 0;
  for (int q = 0; q < T; ++q) k += (S.state[q] != 0 && S.id[q] < S.id[t]) ? 1 : 0;
  ints[k] = S.id[t]; ints[T + k] = S.state[t]; ints[2 * T + k] = S.act[t]; ints[3 * T + k] = S.fid[t]; ints[4 * T + k] = S.start[t];
  ints[5 * T + k] = S.tlen[t];
  score_cls[k] = S.score[t]; score_cls[T + k] = S.cls[t];
  for (int i = 0; i < 8; ++i) mean[k * 8 + i] = S.mean[i * T + t];
  double* P = cov + (size_t)k * 64;
  for (int e = 0; e < 64; ++e) P[e] = 0.;
  for (int i = 0; i < 4; ++i) {
    P[i * 8 + i] = S.cov[(3 * i) * T + t];
    P[i * 8 + i + 4] = P[(i + 4) * 8 + i] = S.cov[(3 * i + 1) * T + t];
    P[(i + 4) * 8 + i + 4] = S.cov[(3 * i + 2) * T + t];
  }
}

static size_t tk_update_lds(int cap) { return (size_t)TK_CAP * TK_LD * 4 + ((tk_state_bytes(cap) + 15) & ~(size_t)15) + TK_CAP * 8 + (TK_CAP + 4) * 4 + 10 * TK_CAP * 4 + TK_CAP * 4 + 3 * TK_CAP * 16; }
static size_t tk_assign_lds() { return (size_t)TK_CAP * TK_LD * 4 + TK_CAP * 8 + (TK_CAP + 4) * 4 + 2 * TK_CAP * 4; }

extern "C" size_t mgdt_bytetrack_state_bytes(int streams, int cap) {
  if (streams < 1 || cap < 1 || cap > TK_CAP) return 0;
  return (size_t)streams * tk_state_bytes(cap);
}

extern "C" int mgdt_bytetrack_reset(void* state, int streams, int cap, int stream, mgdt_stream s) {
  if (!state) MGDT_FAIL(MGDT_BAD_ARG, "bytetrack_reset: null pointer");
  if (streams < 1 || cap < 1 || cap > TK_CAP || stream < -1 || stream >= streams)
    MGDT_FAIL(MGDT_BAD_SHAPE, "bytetrack_reset: streams=%d cap=%d (1..%d) stream=%d (-1 = all)", streams, cap, TK_CAP, stream);
  const size_t sb = tk_state_bytes(cap);
  hipError_t e = stream < 0 ? hipMemsetAsync(state, 0, sb * streams, (hipStream_t)s) : hipMemsetAsync((char*)state + sb * stream, 0, sb, (hipStream_t)s);
  if (e != hipSuccess) MGDT_FAIL(MGDT_LAUNCH_FAIL, "bytetrack_reset: %s", hipGetErrorString(e));
  return MGDT_OK;
}

extern "C" int mgdt_bytetrack_update(const float* rows, const int32_t* counts, const uint8_t* active, int streams, int max_det, void* state, int cap,
                                     float track_high_thresh, float track_low_thresh, float new_track_thresh, float match_thresh, int max_time_lost,
                                     float* tracks, int32_t* ntracks, int32_t* flags, mgdt_stream s) {
  if (!rows || !counts || !state || !tracks || !ntracks || !flags) MGDT_FAIL(MGDT_BAD_ARG, "bytetrack_update: null pointer");
  if (streams < 1 || streams > 65535 || cap < 1 || cap > TK_CAP || max_det < 1 || max_det > (1 << 20))
    MGDT_FAIL(MGDT_BAD_SHAPE, "bytetrack_update: streams=%d (1..65535) cap=%d (1..%d) max_det=%d (1..2^20)", streams, cap, TK_CAP, max_det);
  if (int rc = lds_optin<bytetrack_update_kernel>("bytetrack_update")) return rc;
  bytetrack_update_kernel<<<streams, 64, tk_update_lds(cap), (hipStream_t)s>>>(rows, counts, active, (char*)state, cap, max_det,
                                                                                TkCfg{track_high_thresh, track_low_thresh, new_track_thresh, match_thresh, max_time_lost},
                                                                                tracks, ntracks, flags);
  MGDT_CHECK_LAUNCH("bytetrack_update");
  return MGDT_OK;
}

extern "C" int mgdt_track_assign(const float* cost, const int32_t* n, const int32_t* m, int batch, int n_max, int m_max, float thresh, int32_t* x,
                                 mgdt_stream s) {
  if (!cost || !n || !m || !x) MGDT_FAIL(MGDT_BAD_ARG, "track_assign: null pointer");
  if (batch < 1 || batch > 65535 || n_max < 1 || n_max > TK_CAP || m_max < 1 || m_max > TK_CAP)
    MGDT_FAIL(MGDT_BAD_SHAPE, "track_assign: batch=%d (1..65535) n_max=%d m_max=%d (1..%d)", batch, n_max, m_max, TK_CAP);
  if (int rc = lds_optin<track_assign_kernel>("track_assign")) return rc;
  track_assign_kernel<<<batch, 64, tk_assign_lds(), (hipStream_t)s>>>(cost, n, m, n_max, m_max, thresh, x);
  MGDT_CHECK_LAUNCH("track_assign");
  return MGDT_OK;
}

extern "C" int mgdt_bytetrack_export(const void* state, int streams, int cap, int stream, int32_t* hdr, int32_t* ints, float* score_cls, double* mean,
                                     double* cov, mgdt_stream s) {
  if (!state || !hdr || !ints || !score_cls || !mean || !cov) MGDT_FAIL(MGDT_BAD_ARG, "bytetrack_export: null pointer");
  if (streams < 1 || cap < 1 || cap > TK_CAP || stream < 0 || stream >= streams)
    MGDT_FAIL(MGDT_BAD_SHAPE, "bytetrack_export: streams=%d cap=%d (1..%d) stream=%d", streams, cap, TK_CAP, stream);
  bytetrack_export_kernel<<<1, TK_CAP, 0, (hipStream_t)s>>>((char*)state + tk_state_bytes(cap) * stream, cap, hdr, ints, score_cls, mean, cov);
  MGDT_CHECK_LAUNCH("bytetrack_export");
  return MGDT_OK;
}
