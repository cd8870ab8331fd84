// Training for randomized smoothing: the loss over the noisy copies of every clip and its gradient at the logits -- Gaussian-noise
// training of the smoothed classifier (Cohen, Rosenfeld, Kolter 2019) at lam = 0, MACER (Zhai et al., ICLR 2020) at lam > 0.
// (include/lipasr.h, lipasr_smooth_loss, fixes the definitions and conventions.)
//
// smooth_loss_kernel: ONE workgroup of 64 threads (one wavefront) per clip, one launch per call, no workspace, no atomics.
//   1. the clip's draws x classes logits come into LDS with coalesced loads;
//   2. lane j takes copy j: both softmaxes of its row (sm_row) into LDS, log p_jy beside them;
//   3. lane c takes class c: the means p^_c and q_c over the copies, summed in the order of j (sm_col_mean);
//   4. lane 0 takes the clip: L_C, the arg maxima, xi, the hinge, a_y and a_B (sm_head), left in LDS for every lane;
//   5. lane j writes the gradient row of copy j (sm_row_grad) over its logits in LDS, rounded to fp32;
//   6. the rows leave with coalesced stores.
//   All arithmetic is fp64.  A clip is at most 64 x 32 numbers, a call a few dozen clips: the kernel is bound by the latency of
//   its serial fp64 chains (a row of exp, one Phi^-1), not by any throughput, and the 64 workgroups of a training batch are
//   resident at once.  LDS rows are padded to an odd stride (classes | 1), so the lanes of step 2 and 5, which walk down their own
//   rows, hit different banks.  Everything a lane indexes at run time lives in LDS, never in a per-lane array (no scratch).
//
// The four sm_* functions are __host__ __device__: lipasr_smooth_loss_host runs the same text in loops, as normal4 (common.h) serves
// both sides of the noise.  The host's results differ from the device's by the last places of libm's exp / log / sqrt and of the
// multiply-adds the device fuses, nothing else.
#include "common.h"

namespace lipasr {

constexpr int kSlMaxDraws = 64;
constexpr int kSlMaxC = 32;
constexpr int kSlThreads = 64;

long g_smooth_launches[2] = {};  // lipasr_debug_smooth_loss_launches: 0 the loss kernel, 1 smooth_expand_kernel (smoothing.hip)

struct SmCfg {
  int m, C;  // draws, classes
  double sigma, lam, gamma, beta, scale;
};

// what step 4 leaves for step 5, and the clip's three outputs
struct SmHead {
  double loss, radius, lw, ay, aB;
  int B, active, bad, correct;
};

__host__ __device__ inline bool sm_finite(double v) { return v - v == 0.0; }

// Phi^-1: Wichura, Algorithm AS 241 (Applied Statistics 37, 1988), routine PPND16; 0 -> -inf, 1 -> +inf, outside [0, 1] -> NaN
__host__ __device__ inline double sm_probit(double p) {
  if (!(p >= 0.0 && p <= 1.0)) return NAN;
  if (p == 0.0) return -INFINITY;
  if (p == 1.0) return INFINITY;
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                            4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                          1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                            2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                          4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  double r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  double num, den;
  if (r <= 5.0) {
    r -= 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
               1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
             4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
               1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
             2.05319162663775882187e+0) * r + 1.0);
  } else {
    r -= 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
               2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
             5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
               7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
             5.99832206555887937690e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// one copy: p = softmax(z), s = softmax(beta z) (beta > 0: both subtract the row's maximum), log p_y; returns 1 for a row that
// poisons its clip (a non-finite logit, a label outside [0, C)), whose p and s are then zeros
__host__ __device__ inline int sm_row(const float* z, int C, int y, double beta, double* p, double* s, double* logpy) {
  bool ok = y >= 0 && y < C;
  double mx = -INFINITY;
  for (int c = 0; c < C; ++c) {
    const double v = (double)z[c];
    ok = ok && sm_finite(v);
    mx = v > mx ? v : mx;
  }
  if (!ok) {
    for (int c = 0; c < C; ++c) { p[c] = 0.0; s[c] = 0.0; }
    *logpy = 0.0;
    return 1;
  }
  double se = 0.0, sb = 0.0;
  for (int c = 0; c < C; ++c) {
    const double d = (double)z[c] - mx;
    const double e = exp(d), eb = exp(beta * d);
    p[c] = e;
    s[c] = eb;
    se += e;
    sb += eb;
  }
  for (int c = 0; c < C; ++c) { p[c] /= se; s[c] /= sb; }
  *logpy = ((double)z[y] - mx) - log(se);
  return 0;
}

// the mean over the copies of one class (a[j * stride], j = 0 .. m - 1, in that order)
__host__ __device__ inline double sm_col_mean(const double* a, int stride, int m) {
  double t = 0.0;
  for (int j = 0; j < m; ++j) t += a[(size_t)j * stride];
  return t / (double)m;
}

// the clip: phat, q [C], logpy and bad [m] -> SmHead
__host__ __device__ inline void sm_head(const SmCfg& k, int y, const double* phat, const double* q, const double* logpy, const int* bad,
                                        SmHead* h) {
  h->loss = NAN; h->radius = 0.0; h->lw = 0.0; h->ay = 0.0; h->aB = 0.0;
  h->B = 0; h->active = 0; h->correct = 0;
  int any = (y >= 0 && y < k.C) ? 0 : 1;
  for (int j = 0; j < k.m; ++j) any |= bad[j];
  h->bad = any;
  if (any) return;
  // L_C = log m - logsumexp_j log p_jy
  double mxl = -INFINITY;
  for (int j = 0; j < k.m; ++j) mxl = logpy[j] > mxl ? logpy[j] : mxl;
  double t = 0.0;
  for (int j = 0; j < k.m; ++j) t += exp(logpy[j] - mxl);
  h->lw = mxl + log(t);
  const double LC = log((double)k.m) - h->lw;
  int ap = 0, A = 0, B = -1;
  for (int c = 1; c < k.C; ++c) {
    if (phat[c] > phat[ap]) ap = c;
    if (q[c] > q[A]) A = c;
  }
  for (int c = 0; c < k.C; ++c)
    if (c != y && (B < 0 || q[c] > q[B])) B = c;
  h->correct = ap == y ? 1 : 0;
  const double qB = B >= 0 ? q[B] : 0.0;
  const double xy = sm_probit(q[y]), xB = sm_probit(qB);
  const double xi = xy - xB;
  h->B = B >= 0 ? B : 0;
  h->active = (k.lam > 0.0 && k.C > 1 && A == y && qB > 0.0 && q[y] < 1.0 && xi <= k.gamma) ? 1 : 0;
  double LR = 0.0;
  if (h->active) {
    LR = 0.5 * k.sigma * (k.gamma - xi);
    h->ay = 2.5066282746310002 * exp(0.5 * xy * xy);
    h->aB = 2.5066282746310002 * exp(0.5 * xB * xB);
  }
  h->loss = LC + k.lam * LR;
  h->radius = (A == y && k.sigma > 0.0) ? 0.5 * k.sigma * xi : 0.0;
}

// the gradient row of one copy, rounded to fp32.  d_cc - p_c is the sum of the other classes (no cancellation near p_c = 1)
__host__ __device__ inline void sm_row_grad(const SmCfg& k, const SmHead& h, int y, const double* p, const double* s, double logpy,
                                            float* dz) {
  if (h.bad) {
    for (int c = 0; c < k.C; ++c) dz[c] = NAN;
    return;
  }
  const double w = exp(logpy - h.lw);
  double py_rest = 0.0, sy_rest = 0.0, sB_rest = 0.0;
  for (int c = 0; c < k.C; ++c) {
    if (c != y) { py_rest += p[c]; sy_rest += s[c]; }
    if (c != h.B) sB_rest += s[c];
  }
  const double fy = h.active ? h.ay * s[y] : 0.0, fB = h.active ? h.aB * s[h.B] : 0.0;
  const double rob = k.lam * 0.5 * k.sigma * (k.beta / (double)k.m);
  for (int c = 0; c < k.C; ++c) {
    double g = -w * (c == y ? py_rest : -p[c]);
    if (h.active) {
      const double ty = c == y ? sy_rest : -s[c], tB = c == h.B ? sB_rest : -s[c];
      g -= rob * (fy * ty - fB * tB);
    }
    dz[c] = (float)(k.scale * g);
  }
}

__global__ __launch_bounds__(kSlThreads) void smooth_loss_kernel(const float* __restrict__ logits, const int* __restrict__ label,
                                                                  SmCfg k, float* __restrict__ dz, float* __restrict__ loss,
                                                                  float* __restrict__ correct, float* __restrict__ radius) {
  constexpr int kLd = kSlMaxC | 1;
  __shared__ float zs[kSlMaxDraws * kLd];   // the logits, then the gradient rows
  __shared__ double ps[kSlMaxDraws * kLd];  // p_j
  __shared__ double ss[kSlMaxDraws * kLd];  // s_j
  __shared__ double logpy[kSlMaxDraws];
  __shared__ int bad[kSlMaxDraws];
  __shared__ double phat[kSlMaxC], q[kSlMaxC];
  __shared__ SmHead head;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const int ld = k.C | 1, n = k.m * k.C;
  const size_t base = b * (size_t)n;
  const int y = label[b];
  for (int i = tid; i < n; i += kSlThreads) zs[(i / k.C) * ld + (i % k.C)] = logits[base + i];
  __syncthreads();
  if (tid < k.m) bad[tid] = sm_row(zs + tid * ld, k.C, y, k.beta, ps + tid * ld, ss + tid * ld, &logpy[tid]);
  __syncthreads();
  if (tid < k.C) {
    phat[tid] = sm_col_mean(ps + tid, ld, k.m);
    q[tid] = sm_col_mean(ss + tid, ld, k.m);
  }
  __syncthreads();
  if (tid == 0) {
    SmHead h;
    sm_head(k, y, phat, q, logpy, bad, &h);
    head = h;
    loss[b] = (float)h.loss;
    if (correct) correct[b] = (float)h.correct;
    if (radius) radius[b] = (float)h.radius;
  }
  __syncthreads();
  if (tid < k.m) {
    const SmHead h = head;
    sm_row_grad(k, h, y, ps + tid * ld, ss + tid * ld, logpy[tid], zs + tid * ld);
  }
  __syncthreads();
  for (int i = tid; i < n; i += kSlThreads) dz[base + i] = zs[(i / k.C) * ld + (i % k.C)];
}

static int smooth_loss_check(const char* fn, int clips, int draws, int classes, float sigma, float lam, float gamma, float beta,
                             float scale) {
  LP_CHECK_ARG(classes >= 1 && classes <= kSlMaxC, "%s: %d classes; 1 to %d are supported", fn, classes, kSlMaxC);
  LP_CHECK_ARG(draws >= 1 && draws <= kSlMaxDraws, "%s: %d draws; 1 to %d are supported", fn, draws, kSlMaxDraws);
  LP_CHECK_ARG(clips >= 0, "%s: %d clips", fn, clips);
  LP_CHECK_ARG(sigma >= 0.0f && sigma < INFINITY, "%s: sigma %g", fn, (double)sigma);
  LP_CHECK_ARG(lam >= 0.0f && lam < INFINITY, "%s: lam %g", fn, (double)lam);
  LP_CHECK_ARG(gamma > 0.0f && gamma < INFINITY, "%s: gamma %g", fn, (double)gamma);
  LP_CHECK_ARG(beta > 0.0f && beta < INFINITY, "%s: beta %g", fn, (double)beta);
  LP_CHECK_ARG(scale - scale == 0.0f, "%s: scale %g", fn, (double)scale);
  return LIPASR_OK;
}

static SmCfg smooth_cfg(int draws, int classes, float sigma, float lam, float gamma, float beta, float scale) {
  SmCfg k;
  k.m = draws; k.C = classes;
  k.sigma = sigma; k.lam = lam; k.gamma = gamma; k.beta = beta; k.scale = scale;
  return k;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_smooth_loss(lipasr_handle_t h, const float* logits, const int* label, int clips, int draws, int classes, float sigma,
                       float lam, float gamma, float beta, float scale, float* dz, float* loss, float* correct, float* radius,
                       lipasr_stream_t stream) {
  const int rc = smooth_loss_check("lipasr_smooth_loss", clips, draws, classes, sigma, lam, gamma, beta, scale);
  if (rc != LIPASR_OK) return rc;
  LP_CHECK_ARG(h != nullptr, "lipasr_smooth_loss: null handle");
  if (clips == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits && label && dz && loss, "lipasr_smooth_loss: logits, label, dz or loss is null");
  hipLaunchKernelGGL(smooth_loss_kernel, dim3((unsigned)clips), dim3(kSlThreads), 0, S(stream), logits, label,
                     smooth_cfg(draws, classes, sigma, lam, gamma, beta, scale), dz, loss, correct, radius);
  LP_LAUNCH_CHECK();
  ++g_smooth_launches[0];
  return LIPASR_OK;
}

int lipasr_smooth_loss_host(const float* logits, const int* label, int clips, int draws, int classes, float sigma, float lam,
                            float gamma, float beta, float scale, float* dz, float* loss, float* correct, float* radius) {
  const int rc = smooth_loss_check("lipasr_smooth_loss_host", clips, draws, classes, sigma, lam, gamma, beta, scale);
  if (rc != LIPASR_OK) return rc;
  if (clips == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits && label && dz && loss, "lipasr_smooth_loss_host: logits, label, dz or loss is null");
  const SmCfg k = smooth_cfg(draws, classes, sigma, lam, gamma, beta, scale);
  std::vector<double> ps((size_t)draws * classes), ss((size_t)draws * classes), logpy(draws), phat(classes), q(classes);
  std::vector<int> bad(draws);
  for (int b = 0; b < clips; ++b) {
    const size_t base = (size_t)b * draws * classes;
    const int y = label[b];
    for (int j = 0; j < draws; ++j)
      bad[j] = sm_row(logits + base + (size_t)j * classes, classes, y, k.beta, &ps[(size_t)j * classes], &ss[(size_t)j * classes], &logpy[j]);
    for (int c = 0; c < classes; ++c) {
      phat[c] = sm_col_mean(&ps[c], classes, draws);
      q[c] = sm_col_mean(&ss[c], classes, draws);
    }
    SmHead hd;
    sm_head(k, y, phat.data(), q.data(), logpy.data(), bad.data(), &hd);
    loss[b] = (float)hd.loss;
    if (correct) correct[b] = (float)hd.correct;
    if (radius) radius[b] = (float)hd.radius;
    for (int j = 0; j < draws; ++j)
      sm_row_grad(k, hd, y, &ps[(size_t)j * classes], &ss[(size_t)j * classes], logpy[j], dz + base + (size_t)j * classes);
  }
  return LIPASR_OK;
}

int lipasr_smooth_probit_host(const double* q, int n, double* out) {
  LP_CHECK_ARG(n >= 0, "lipasr_smooth_probit_host: n %d", n);
  LP_CHECK_ARG(n == 0 || (q != nullptr && out != nullptr), "lipasr_smooth_probit_host: q or out is null");
  for (int i = 0; i < n; ++i) out[i] = sm_probit(q[i]);
  return LIPASR_OK;
}

int lipasr_debug_smooth_loss_launches(int id) { return (id >= 0 && id < 2) ? (int)g_smooth_launches[id] : -1; }

}  // extern "C"
