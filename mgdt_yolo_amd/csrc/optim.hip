// Optimizer step over ONE flat fp32 buffer (all parameters of the model are views into it): gradient-norm clipping,
// SGD with Nesterov momentum + per-element weight decay, EMA of the weights - three launches instead of ~600 small ATen
// kernels per step (reference: yolo/engine/trainer.py:462-470 optimizer_step, :633-664 build_optimizer groups,
// yolo/utils/torch_utils.py:335-367 ModelEMA).  The same flat gradient buffer is what the data-parallel all-reduce sends.
#include "common.h"

#define OPT_BLOCK 256
__global__ __launch_bounds__(OPT_BLOCK) void sumsq_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partial) {
  double acc = 0.0;
  for (long i = blockIdx.x * (long)OPT_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * OPT_BLOCK) { double v = g[i]; acc += v * v; }
  __shared__ double red[OPT_BLOCK];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = OPT_BLOCK / 2; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
// out[0] = total norm, out[1] = clip coefficient min(1, max_norm / (norm + 1e-6))  (torch.nn.utils.clip_grad_norm_)
__global__ __launch_bounds__(256) void clip_coef_kernel(const double* partial, int nb, float max_norm, float* out) {
  __shared__ double red[256];
  double t = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) t += partial[i];          // fixed order: thread t owns partials t, t+256, ...
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) {
    const double s = red[0];
    float norm = (float)sqrt(s);
    out[0] = norm;
    float c = max_norm / (norm + 1e-6f);
    out[1] = c < 1.f ? c : 1.f;
  }
}

extern "C" size_t mgdt_grad_norm_workspace_bytes(void) { return 1024 * sizeof(double); }
extern "C" int mgdt_grad_clip_coef(const float* g, long n, float max_norm, float* out2, void* ws, mgdt_stream s) {
  if (!g || !out2 || !ws || n <= 0) MGDT_FAIL(MGDT_BAD_ARG, "grad_clip_coef: null/empty argument");
  int nb = (int)std::min<long>((n + OPT_BLOCK - 1) / OPT_BLOCK, 1024);
  sumsq_partial_kernel<<<nb, OPT_BLOCK, 0, (hipStream_t)s>>>(g, n, (double*)ws);
  clip_coef_kernel<<<1, 256, 0, (hipStream_t)s>>>((const double*)ws, nb, max_norm, out2);
  MGDT_CHECK_LAUNCH("grad_clip_coef");
  return MGDT_OK;
}

// ---- SGD / Adam / AdamW / RMSProp and the EMA on the same flat buffers: one kernel -----------------------------------------------------------
// The reference's build_optimizer (yolo/engine/trainer.py:651-656) picks torch.optim.SGD / Adam / AdamW / RMSprop by name; `optimizer: auto` resolves
// to AdamW for short runs (:635-639).  The arithmetic below is torch's single-tensor path, one rounding per operation (this file is built without
// contraction).  Elements [0, n_param) are parameters (the family's step, then the EMA of the new value), [n_param, n_total) float buffers (EMA
// only).  A streaming kernel: up to 10 words per parameter (p, m, v, ema read and written; g, wd read; a family without m or v touches neither),
// one 16-byte load / store per lane and array where the four elements lie on one side of n_param, a scalar evaluation of the same element
// function for the straddling quad and the tail - so the vector and the scalar path, and the eager and the captured-step form (one kernel,
// scalars from arguments or from `hyper`), agree bit for bit.  No LDS, no scratch.
//
// hyper (fp32[4] for SGD, fp32[8] = MGDT_OPT_HYPER_LEN for the others; E::N_HYPER slots are read); a family ignores the slots it has no use for:
//   [0] lr   [1] lr_bias   [2] momentum (SGD, RMSProp) / beta1 (Adam)   [3] ema_decay
//   [4] lr / bc1   [5] lr_bias / bc1   [6] sqrt(bc2)   [7] 1 - beta1          (bc1 = 1 - beta1^step, bc2 = 1 - beta2^step; Adam only)
// A captured training step replays with values the host writes into `hyper` between replays (warm-up interpolation trainer.py:317-326, the EMA
// ramp torch_utils.py:342).
struct OptScalars {
  float lr, lr_bias, mom, d;              // hyper[0..3]
  float step, step_bias, sqrt_bc2, omb1;  // hyper[4..7]
  float beta2, omb2, eps;                 // constants of a run: beta2 / alpha, 1 - beta2 / 1 - alpha, eps
  int decoupled;                          // Adam: decoupled weight decay (AdamW)
  int nesterov, first;                    // SGD: Nesterov step; first step (the buffer becomes g', its old content is not used)
};
template <class E> __device__ __forceinline__ void opt_load_hyper(OptScalars& a, const float* __restrict__ hyper) {
  if (!hyper) return;
  a.lr = hyper[0]; a.lr_bias = hyper[1]; a.mom = hyper[2]; a.d = hyper[3];
  if constexpr (E::N_HYPER > 4) { a.step = hyper[4]; a.step_bias = hyper[5]; a.sqrt_bc2 = hyper[6]; a.omb1 = hyper[7]; }
}
// wd < 0 marks the reference's bias group (trainer.py:644): no decay and its own learning rate `lr_bias` (warm-up, trainer.py:323)
struct SgdElem {
  static constexpr bool HAS_M = true, HAS_V = false;
  static constexpr int N_HYPER = 4;
  // g' = c*g + wd*p; buf = first ? g' : momentum*buf + g'; p -= lr * (nesterov ? g' + momentum*buf : buf).  m is the momentum buffer.
  static __device__ __forceinline__ void run(float& p, float g, float& m, float& v, float w, const OptScalars& a, float c) {
    const float gi = c * g + (w > 0.f ? w * p : 0.f);
    const float b = a.first ? gi : a.mom * m + gi;
    m = b;
    p -= (w < 0.f ? a.lr_bias : a.lr) * (a.nesterov ? gi + a.mom * b : b);
  }
};
struct AdamElem {
  static constexpr bool HAS_M = true, HAS_V = true;
  static constexpr int N_HYPER = 8;
  // Adam: g' = c*g + wd*p; AdamW: p *= 1 - lr*wd, g' = c*g.  m.lerp_(g', 1 - beta1); v.mul_(beta2).addcmul_(g', g', 1 - beta2);
  // denom = sqrt(v) / sqrt(bc2) + eps; p.addcdiv_(m, denom, -lr / bc1)
  static __device__ __forceinline__ void run(float& p, float g, float& m, float& v, float w, const OptScalars& a, float c) {
    float gi = c * g;
    if (w > 0.f) { if (a.decoupled) p *= 1.f - a.lr * w; else gi += w * p; }
    m += (gi - m) * a.omb1;
    v = a.beta2 * v + (a.omb2 * gi) * gi;
    const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
    p -= ((w < 0.f ? a.step_bias : a.step) * m) / denom;
  }
};
template <bool MOM> struct RmsElem {
  // g' = c*g + wd*p; sq.mul_(alpha).addcmul_(g', g', 1 - alpha); avg = sqrt(sq) + eps; momentum: buf.mul_(momentum).addcdiv_(g', avg),
  // p.add_(buf, -lr); else p.addcdiv_(g', avg, -lr).  m is the momentum buffer (neither read nor written without momentum), v the square average.
  static constexpr bool HAS_M = MOM, HAS_V = true;
  static constexpr int N_HYPER = 8;
  static __device__ __forceinline__ void run(float& p, float g, float& m, float& v, float w, const OptScalars& a, float c) {
    float gi = c * g;
    if (w > 0.f) gi += w * p;
    v = a.beta2 * v + (a.omb2 * gi) * gi;
    const float avg = sqrtf(v) + a.eps;
    const float lr = w < 0.f ? a.lr_bias : a.lr;
    if (MOM) { m = a.mom * m + gi / avg; p -= lr * m; }
    else p -= (lr * gi) / avg;
  }
};
// v *= d; v += (1 - d) * w (torch_utils.py ModelEMA.update)
__device__ __forceinline__ float ema_of(float e, float x, float d) { return d * e + (1.f - d) * x; }
__device__ __forceinline__ void ema_quad(float* __restrict__ ema, long i, const float4& P, float d) {
  float4 Q = *(const float4*)(ema + i);
  Q.x = ema_of(Q.x, P.x, d); Q.y = ema_of(Q.y, P.y, d); Q.z = ema_of(Q.z, P.z, d); Q.w = ema_of(Q.w, P.w, d);
  *(float4*)(ema + i) = Q;
}
// element j on the scalar path: the family's step if it is a parameter, then the EMA
template <class E>
__device__ __forceinline__ void flat_one(long j, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                         const float* __restrict__ wd, long n_param, float* __restrict__ ema, const OptScalars& a, float c) {
  float x = p[j];
  if (j < n_param) {
    float mj = E::HAS_M ? m[j] : 0.f, vj = E::HAS_V ? v[j] : 0.f;
    E::run(x, g[j], mj, vj, wd ? wd[j] : 0.f, a, c);
    p[j] = x;
    if (E::HAS_V) v[j] = vj;
    if (E::HAS_M) m[j] = mj;
  }
  if (ema) ema[j] = ema_of(ema[j], x, a.d);
}
#define OPT_GRID_CAP 2048
template <class E>
__global__ __launch_bounds__(OPT_BLOCK) void flat_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                              const float* __restrict__ wd, long n_param, float* __restrict__ ema, long n_total, long nq,
                                                              OptScalars a, const float* __restrict__ hyper, const float* __restrict__ clip) {
  opt_load_hyper<E>(a, hyper);
  const float c = clip ? clip[1] : 1.f;
  const long t0 = blockIdx.x * (long)OPT_BLOCK + threadIdx.x, stride = (long)gridDim.x * OPT_BLOCK;
  for (long q = t0; q < nq; q += stride) {           // nq quads of four elements, every array 16-byte aligned (0 when one is not)
    const long i = q * 4;
    if (i + 4 <= n_param) {
      const float4 Z = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 P = *(const float4*)(p + i), V = Z, M = Z, W = Z;
      if (E::HAS_V) V = *(const float4*)(v + i);
      if (E::HAS_M) M = *(const float4*)(m + i);
      const float4 G = *(const float4*)(g + i);
      if (wd) W = *(const float4*)(wd + i);
      E::run(P.x, G.x, M.x, V.x, W.x, a, c);
      E::run(P.y, G.y, M.y, V.y, W.y, a, c);
      E::run(P.z, G.z, M.z, V.z, W.z, a, c);
      E::run(P.w, G.w, M.w, V.w, W.w, a, c);
      *(float4*)(p + i) = P;
      if (E::HAS_V) *(float4*)(v + i) = V;
      if (E::HAS_M) *(float4*)(m + i) = M;
      if (ema) ema_quad(ema, i, P, a.d);
    } else if (i >= n_param) {                       // float buffers (batch-norm statistics): EMA only
      if (ema) ema_quad(ema, i, *(const float4*)(p + i), a.d);
    } else {                                         // the one quad that straddles n_param
      for (long j = i; j < i + 4; ++j) flat_one<E>(j, p, g, m, v, wd, n_param, ema, a, c);
    }
  }
  // tail (n_total % 4 elements), or everything when an array is not 16-byte aligned
  for (long j = nq * 4 + t0; j < n_total; j += stride) flat_one<E>(j, p, g, m, v, wd, n_param, ema, a, c);
}
// m / v may be NULL where the family has none; ema NULL: no EMA; hyper NULL: the per-step scalars are those of `a`
template <class E>
static int flat_launch(const char* what, float* p, const float* g, float* m, float* v, const float* wd, long n_param, float* ema, long n_total,
                       const OptScalars& a, const float* hyper, const float* clip2, mgdt_stream s) {
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)wd | (uintptr_t)ema;      // NULL contributes nothing
  const long nq = (bits & 15) ? 0 : n_total / 4;
  const long work = nq + (n_total - nq * 4);
  const int nb = (int)std::min<long>((work + OPT_BLOCK - 1) / OPT_BLOCK, OPT_GRID_CAP);
  flat_step_kernel<E><<<nb, OPT_BLOCK, 0, (hipStream_t)s>>>(p, g, m, v, wd, n_param, ema, n_total, nq, a, hyper, clip2);
  MGDT_CHECK_LAUNCH(what);
  return MGDT_OK;
}
static OptScalars sgd_scalars(float lr, float lr_bias, float momentum, float ema_decay, int nesterov, int first) {
  OptScalars a = {};
  a.lr = lr; a.lr_bias = lr_bias; a.mom = momentum; a.d = ema_decay; a.nesterov = nesterov; a.first = first;
  return a;
}
// lr / bc1 and sqrt(bc2) in double, as torch's _single_tensor_adam computes them in Python floats, then rounded to fp32 once
static OptScalars adam_scalars(double lr, double lr_bias, double beta1, double beta2, double eps, int step, int decoupled) {
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  OptScalars a = {};
  a.lr = (float)lr; a.lr_bias = (float)lr_bias; a.mom = (float)beta1;
  a.step = (float)(lr / bc1); a.step_bias = (float)(lr_bias / bc1); a.sqrt_bc2 = (float)sqrt(bc2); a.omb1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2; a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps; a.decoupled = decoupled ? 1 : 0;
  return a;
}
static OptScalars rms_scalars(double lr, double lr_bias, double alpha, double eps, double momentum) {
  OptScalars a = {};
  a.lr = (float)lr; a.lr_bias = (float)lr_bias; a.mom = (float)momentum;
  a.beta2 = (float)alpha; a.omb2 = (float)(1.0 - alpha); a.eps = (float)eps;
  return a;
}
extern "C" int mgdt_sgd_step(float* p, const float* g, float* buf, const float* wd, long n, float lr, float lr_bias, float momentum, int nesterov,
                             int first, const float* clip2, mgdt_stream s) {
  if (!p || !g || !buf || n <= 0) MGDT_FAIL(MGDT_BAD_ARG, "sgd_step: null/empty argument");
  return flat_launch<SgdElem>("sgd_step", p, g, buf, nullptr, wd, n, nullptr, n, sgd_scalars(lr, lr_bias, momentum, 0.f, nesterov, first), nullptr, clip2, s);
}
extern "C" int mgdt_sgd_ema_step_dev(float* p, const float* g, float* buf, const float* wd, long n_param, float* ema, long n_total, const float* hyper4,
                                     int nesterov, int first, const float* clip2, mgdt_stream s) {
  if (!p || !g || !buf || !hyper4 || n_param <= 0 || n_total < n_param) MGDT_FAIL(MGDT_BAD_ARG, "sgd_ema_step_dev: null/empty argument");
  return flat_launch<SgdElem>("sgd_ema_step_dev", p, g, buf, nullptr, wd, n_param, ema, n_total, sgd_scalars(0.f, 0.f, 0.f, 0.f, nesterov, first), hyper4, clip2, s);
}
// n_param = 0: every element is a "buffer" and takes the EMA-only branch; the element type is never run and p never written
extern "C" int mgdt_ema_update(float* ema, const float* p, long n, float decay, mgdt_stream s) {
  if (!ema || !p || n <= 0) MGDT_FAIL(MGDT_BAD_ARG, "ema_update: null/empty argument");
  return flat_launch<SgdElem>("ema_update", const_cast<float*>(p), nullptr, nullptr, nullptr, nullptr, 0, ema, n, sgd_scalars(0.f, 0.f, 0.f, decay, 0, 0), nullptr,
                              nullptr, s);
}
extern "C" int mgdt_adam_step(float* p, const float* g, float* m, float* v, const float* wd, long n, double lr, double lr_bias, double beta1,
                              double beta2, double eps, int step, int decoupled, const float* clip2, mgdt_stream s) {
  if (!p || !g || !m || !v || n <= 0 || step < 1) MGDT_FAIL(MGDT_BAD_ARG, "adam_step: null/empty argument or step < 1");
  return flat_launch<AdamElem>("adam_step", p, g, m, v, wd, n, nullptr, n, adam_scalars(lr, lr_bias, beta1, beta2, eps, step, decoupled), nullptr, clip2, s);
}
extern "C" int mgdt_adam_ema_step_dev(float* p, const float* g, float* m, float* v, const float* wd, long n_param, float* ema, long n_total,
                                      const float* hyper8, double beta2, double eps, int decoupled, const float* clip2, mgdt_stream s) {
  if (!p || !g || !m || !v || !hyper8 || n_param <= 0 || n_total < n_param) MGDT_FAIL(MGDT_BAD_ARG, "adam_ema_step_dev: null/empty argument");
  return flat_launch<AdamElem>("adam_ema_step_dev", p, g, m, v, wd, n_param, ema, n_total, adam_scalars(0.0, 0.0, 0.0, beta2, eps, 1, decoupled), hyper8, clip2, s);
}
// buf may be NULL when momentum == 0 (it is not touched)
extern "C" int mgdt_rmsprop_step(float* p, const float* g, float* sq, float* buf, const float* wd, long n, double lr, double lr_bias, double alpha,
                                 double eps, double momentum, const float* clip2, mgdt_stream s) {
  if (!p || !g || !sq || (!buf && momentum > 0.0) || n <= 0) MGDT_FAIL(MGDT_BAD_ARG, "rmsprop_step: null/empty argument");
  const OptScalars a = rms_scalars(lr, lr_bias, alpha, eps, momentum);
  return momentum > 0.0 ? flat_launch<RmsElem<true>>("rmsprop_step", p, g, buf, sq, wd, n, nullptr, n, a, nullptr, clip2, s)
                        : flat_launch<RmsElem<false>>("rmsprop_step", p, g, nullptr, sq, wd, n, nullptr, n, a, nullptr, clip2, s);
}
extern "C" int mgdt_rmsprop_ema_step_dev(float* p, const float* g, float* sq, float* buf, const float* wd, long n_param, float* ema, long n_total,
                                         const float* hyper8, double alpha, double eps, int with_momentum, const float* clip2, mgdt_stream s) {
  if (!p || !g || !sq || (!buf && with_momentum) || !hyper8 || n_param <= 0 || n_total < n_param)
    MGDT_FAIL(MGDT_BAD_ARG, "rmsprop_ema_step_dev: null/empty argument");
  const OptScalars a = rms_scalars(0.0, 0.0, alpha, eps, 0.0);
  return with_momentum ? flat_launch<RmsElem<true>>("rmsprop_ema_step_dev", p, g, buf, sq, wd, n_param, ema, n_total, a, hyper8, clip2, s)
                       : flat_launch<RmsElem<false>>("rmsprop_ema_step_dev", p, g, nullptr, sq, wd, n_param, ema, n_total, a, hyper8, clip2, s);
}

