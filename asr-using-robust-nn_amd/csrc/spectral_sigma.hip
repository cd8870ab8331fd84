// K3, the eigenvalue and rescale step of the product variant: sigma = sqrt(lambda_max) of the R x R Gram matrix by repeated
// normalised squaring, every scale factor of the sequential pass in closed form, and the multi-tensor scaling -- as two launches
// (product_sigma_kernel, scale_layers_kernel) or as one (sigma_scale_layers_kernel).  The squaring step, the closed-form scales and
// the scaling loop are written once, below, for both forms.
#include "spectral.h"

namespace lipasr {

#ifndef LIPASR_SIGMA_WGS
#define LIPASR_SIGMA_WGS 192  // workgroups of sigma_scale_layers_kernel (each recomputes sigma, then scales its slice of a layer)
#endif

// x^(1/m) for x > 0 and a small integer m (the number of layers), to fp64 accuracy without the fp64 pow() (a serial chain of
// thousands of cycles, six of them in a row per projection): range reduction by frexp, a hardware fp32 log2 / exp2 estimate of
// the root of the mantissa part (1e-7), two Newton steps on y^m = f (1e-14, 1e-28).
__device__ __forceinline__ double root_m(double x, int m) {
  if (!(x > 0.0) || !(x < 1.7e308)) return pow(x, 1.0 / (double)m);  // (zero, negative, inf, nan: the library's answers)
  int e;
  double f = frexp(x, &e);  // x = f 2^e, f in [0.5, 1)
  int q = e / m, r = e - q * m;
  if (r < 0) { r += m; q -= 1; }
  f = ldexp(f, r);  // f in [0.5, 2^(m-1)], x = f 2^(q m)
  double y = (double)exp2f(log2f((float)f) / (float)m);
#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    double ym = y;
    for (int k = 1; k < m; ++k) ym *= y;      // y^m
    y -= y * (1.0 - f / ym) / (double)m;
  }
  return ldexp(y, q);
}

// One squaring A <- A^2 / tr(A^2) by all THREADS threads of the workgroup.  *tj: the trace of the new square, the same value in
// every thread (the callers sum log lambda = log t_0 + sum_j 2^-(j+1) log t_j from the traces, each in its own order).  Returns
// true once the rank-1 projector is reached and the caller may stop: the squarings left would add < 1e-12 2^-it to log lambda (at
// 1e-15 rounding noise in the trace kept the loop running all 40 rounds).
// ONE barrier per squaring and no in-place write: the buffers keep the UNnormalised square and the factor 1 / tr of the previous
// round (c2, squared; 1 at the start, when `cur` is normalised) is applied when the next square is formed.  Every thread forms the
// trace itself from a buffer nobody writes until all threads have passed the next barrier (round 4's form rescaled `nxt` in place
// right after the trace reads, with no barrier between them: a wavefront that was late reading the diagonal saw a mix of scaled and
// unscaled entries -- ADVICE r4).
template <int THREADS>
__device__ __forceinline__ bool square_step(double*& cur, double*& nxt, double& c2, int R, double* tj_out) {
  const int RR = R * R;
  for (int e = threadIdx.x; e < RR; e += THREADS) {
    const int a = e / R, b = e - a * R;
    double s = 0.0;
    for (int c = 0; c < R; ++c) s = fma(cur[a * R + c], cur[c * R + b], s);
    nxt[e] = s * c2;
  }
  __syncthreads();
  double tj = 0.0;
  for (int a = 0; a < R; ++a) tj += nxt[a * R + a];
  *tj_out = tj;
  const double inv = 1.0 / tj;
  c2 = inv * inv;
  double* t = cur; cur = nxt; nxt = t;
  return fabs(tj - 1.0) < 1e-12;
}

// The sequential pass in closed form: visit v scales layer order[v] by s_v = (rho / (n_v + eps))^(1/n_layers), and the product's
// norm n_v (n_0 = sigma) follows it; sc[l] = product of the s_v of layer l.  norms_out (may be null): n_0 .. n_(n_order).
__device__ __forceinline__ void sequential_scales(double sigma, double rho, const OrderArgs& oa, double (&sc)[LIPASR_MAX_LAYERS],
                                                  float* __restrict__ norms_out) {
  for (int l = 0; l < oa.n_layers; ++l) sc[l] = 1.0;
  double n = sigma;
  for (int v = 0; v < oa.n_order; ++v) {
    if (norms_out) norms_out[v] = (float)n;
    const double s = root_m(rho / (n + kEps), oa.n_layers);
    sc[oa.order[v]] *= s;
    n *= s;
  }
  if (norms_out) norms_out[oa.n_order] = (float)n;
}

// w[0 .. n) *= s by the threads first, first + stride, ... (skipped when the factor is exactly 1)
__device__ __forceinline__ void scale_span(float* w, size_t n, float s, size_t first, size_t stride) {
  if (s == 1.0f) return;
  if ((reinterpret_cast<uintptr_t>(w) & 15) == 0) {
    const size_t n4 = n >> 2;
    float4* w4 = reinterpret_cast<float4*>(w);
    for (size_t i = first; i < n4; i += stride) {
      float4 x = w4[i];
      x.x *= s; x.y *= s; x.z *= s; x.w *= s;
      w4[i] = x;
    }
    for (size_t i = (n4 << 2) + first; i < n; i += stride) w[i] *= s;
  } else {
    for (size_t i = first; i < n; i += stride) w[i] *= s;
  }
}

// One workgroup: G = sum of partial Grams; sigma = sqrt(lambda_max(G)); closed-form sequential scales.
constexpr int kSigmaThreads = 1024;
constexpr int kSliceDoubles = 1024;  // LDS for the sliced partial sums: min(32, 1024 / R^2) slices x R^2 entries
static_assert(kMaxR * kMaxR <= kSigmaThreads, "product_sigma_kernel: thread (slice, entry) needs one slice at the least");

__global__ __launch_bounds__(kSigmaThreads) void product_sigma_kernel(const double* __restrict__ gram_part, int n_part,
                                                                       int R, double rho, OrderArgs oa,
                                                                       float* __restrict__ scales,
                                                                       float* __restrict__ norms_out,
                                                                       float* __restrict__ sigma_out,
                                                                       int* __restrict__ bump) {
  __shared__ double A[kMaxR * kMaxR];
  __shared__ double B[kMaxR * kMaxR];
  __shared__ double slice_sum[kSliceDoubles];
  __shared__ double tr_s;
  const int tid = threadIdx.x;
  const int RR = R * R;
  // Gram = sum of the per-workgroup partials.  The partials were written by other XCDs, so every load is a trip to
  // memory: thread (slice, entry) takes partials slice, slice + n_sl, ... with eight loads in flight, fixed order.
  {
    int n_sl = kSigmaThreads / RR;  // R <= 32, so at least one
    if (n_sl > 32) n_sl = 32;
    if (n_sl > n_part) n_sl = n_part;
    const int sl = tid / RR, ent = tid - sl * RR;
    if (sl < n_sl) {
      double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int p = sl; p < n_part; p += 8 * n_sl) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int q = p + u * n_sl;
          acc[u] += (q < n_part) ? gram_part[(size_t)q * RR + ent] : 0.0;
        }
      }
      slice_sum[sl * RR + ent] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    __syncthreads();
    for (int e = tid; e < RR; e += kSigmaThreads) {
      double s = 0.0;
      for (int k = 0; k < n_sl; ++k) s += slice_sum[k * RR + e];
      A[e] = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int a = 0; a < R; ++a) t += A[a * R + a];
    tr_s = t;
  }
  __syncthreads();
  const double t0 = tr_s;
  double log_lambda = 0.0;
  bool zero = !(t0 > 0.0);
  if (!zero) {
    log_lambda = log(t0);
    for (int e = tid; e < RR; e += kSigmaThreads) A[e] /= t0;
    __syncthreads();
    double wgt = 0.5;
    double* cur = A;
    double* nxt = B;
    double c2 = 1.0;  // (1 / trace of `cur`)^2; A was normalised above
    for (int it = 0; it < kSquarings; ++it) {
      double tj;
      const bool done = square_step<kSigmaThreads>(cur, nxt, c2, R, &tj);
      log_lambda += wgt * log(tj);
      wgt *= 0.5;
      if (done) break;
    }
  }
  if (tid == 0) {
    if (bump) *bump += 1;  // the optimizer's step counter, when this projection closes a fused Adam + projection step
    const double sigma = zero ? 0.0 : exp(0.5 * log_lambda);
    if (sigma_out) *sigma_out = (float)sigma;
    if (scales) {
      double sc[LIPASR_MAX_LAYERS];
      sequential_scales(sigma, rho, oa, sc, norms_out);
      for (int l = 0; l < oa.n_layers; ++l) scales[l] = (float)sc[l];
    }
  }
}

// blockIdx.y = layer; W_l *= scales[l] (skipped when the factor is exactly 1)
__global__ __launch_bounds__(256) void scale_layers_kernel(LayerPtrs lp, const float* __restrict__ scales) {
  const int l = blockIdx.y;
  scale_span(lp.W[l], (size_t)lp.rows[l] * lp.cols[l], scales[l], (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)gridDim.x * 256);
}

// Round 4: the eigenvalue step and the rescaling in ONE launch.  Every workgroup recomputes sigma for itself from the finished
// product P (R x n, 35 kB for the reference's model: staged in LDS, Gram in fp64, the same normalised squarings as
// product_sigma_kernel) and then scales its slice of its layer -- identical arithmetic on identical inputs in every workgroup,
// so all of them apply the same factors.  Replaces product_sigma_kernel (14 us: one workgroup summing 220 cross-XCD Gram
// partials) + a launch boundary + scale_layers_kernel (8 us) on the critical path of every training step; the chain's last
// step no longer emits Gram partials for it.  Workgroup (0, 0) also writes scales / norms / sigma and bumps the step counter.
#ifndef LIPASR_SSL_THREADS
#define LIPASR_SSL_THREADS 512
#endif
constexpr int kSslThreads = LIPASR_SSL_THREADS, kSslWaves = kSslThreads / 64;  // 256 / 512 / 1024 threads: 22.8 / 20.6 / 29.6 us (the Gram of the product, 4.8 us with four wavefronts, gets faster, everything behind a barrier slower)
static_assert(kSslWaves >= 1 && (kSslWaves & (kSslWaves - 1)) == 0, "sigma_scale_layers_kernel: the pairwise tree over the wavefronts' partial sums halves their number");
// dynamic LDS: A | B | kSslWaves Gram partials (doubles, R^2 each) | P [R][n0] floats (+ 16 for the alignment)
constexpr size_t kSslLdsMax = 96 * 1024;      // above it the two-launch form runs
constexpr size_t kSslLdsDefault = 32 * 1024;  // above it the kernel's dynamic-LDS limit is raised, to kSslLdsMax
static size_t ssl_lds_bytes(int R, int n0) {
  return (size_t)(2 + kSslWaves) * R * R * sizeof(double) + (size_t)R * n0 * sizeof(float) + 16;
}

__global__ __launch_bounds__(kSslThreads) void sigma_scale_layers_kernel(const float* __restrict__ P, int n, int R, double rho, OrderArgs oa,
                                                                  LayerPtrs lp, float* __restrict__ scales_out, float* __restrict__ norms_out,
                                                                  float* __restrict__ sigma_out, int* __restrict__ bump) {
  extern __shared__ __attribute__((aligned(16))) char ssl_raw[];
  const int tid = threadIdx.x;
  const int RR = R * R, total = R * n;
  // dynamic LDS: A | B | four Gram partials (doubles, R^2 each) | P [R][n] floats: 40 kB for 10 x 880, four workgroups per CU
  double* A = reinterpret_cast<double*>(ssl_raw);
  double* B = A + RR;
  double* gpart0 = B + RR;  // [kSslWaves][RR]
  float* Ps = reinterpret_cast<float*>(gpart0 + kSslWaves * RR);
  __shared__ float sc_s[LIPASR_MAX_LAYERS];
  if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0) {
    const float4* src = reinterpret_cast<const float4*>(P);
    float4* dst = reinterpret_cast<float4*>(Ps);
    for (int f = tid; f < (total >> 2); f += kSslThreads) dst[f] = src[f];
  } else {
    for (int f = tid; f < total; f += kSslThreads) Ps[f] = P[f];
  }
  __syncthreads();
  // Gram (symmetric: the R (R + 1) / 2 entries a <= b): wavefront w takes the column quads q = w (mod 4), lane e (and e + 64, ...)
  // the entry; float4 reads of both rows, fp64 products and sums in ascending column order
  {
    const int w = tid >> 6, lane = tid & 63;
    const int n_ent = R * (R + 1) / 2, nq = n >> 2;
    for (int e = lane; e < n_ent; e += 64) {
      int a = 0, rem = e;
      while (rem >= R - a) { rem -= R - a; ++a; }  // e -> (a, b = a + rem)
      const int b = a + rem;
      const float* pa = Ps + (size_t)a * n;
      const float* pb = Ps + (size_t)b * n;
      double s = 0.0;
      if ((n & 3) == 0) {
        for (int q = w; q < nq; q += kSslWaves) {
          const float4 x = *reinterpret_cast<const float4*>(pa + 4 * q), y = *reinterpret_cast<const float4*>(pb + 4 * q);
          s = fma((double)x.x, (double)y.x, s); s = fma((double)x.y, (double)y.y, s);
          s = fma((double)x.z, (double)y.z, s); s = fma((double)x.w, (double)y.w, s);
        }
      } else {
        for (int i = w; i < n; i += kSslWaves) s = fma((double)pa[i], (double)pb[i], s);
      }
      gpart0[w * RR + a * R + b] = s;
      gpart0[w * RR + b * R + a] = s;
    }
  }
  __syncthreads();
  for (int e = tid; e < RR; e += kSslThreads) {  // (fixed order: a pairwise tree over the wavefronts' partial sums)
    double part[kSslWaves];
#pragma unroll
    for (int w = 0; w < kSslWaves; ++w) part[w] = gpart0[w * RR + e];
#pragma unroll
    for (int h = kSslWaves / 2; h >= 1; h >>= 1)
#pragma unroll
      for (int w = 0; w < h; ++w) part[w] = part[2 * w] + part[2 * w + 1];
    A[e] = part[0];
  }
  __syncthreads();
  double t0 = 0.0;
  for (int a = 0; a < R; ++a) t0 += A[a * R + a];
  __syncthreads();
  __shared__ double tj_s[kSquarings + 1];
  __shared__ double ll_s;
  const bool zero = !(t0 > 0.0);
  int n_it = 0;
  if (!zero) {
    for (int e = tid; e < RR; e += kSslThreads) A[e] /= t0;
    __syncthreads();
    // A <- A^2 / tr(A^2).  The traces are kept and their logarithms taken AFTER the loop, all at once (one fp64 log per
    // squaring inside the loop was a serial chain of ~150 dependent instructions in every workgroup: 6 of the kernel's 22 us)
    double* cur = A;
    double* nxt = B;
    double c2 = 1.0;
    for (int it = 0; it < kSquarings; ++it) {
      double tj;
      const bool done = square_step<kSslThreads>(cur, nxt, c2, R, &tj);  // (the same value in every thread of every workgroup)
      if (tid == 0) tj_s[it] = tj;
      n_it = it + 1;
      if (done) break;
    }
    // log lambda = log t0 + sum_j 2^-(j+1) log t_j: thread j < n_it takes term j, wavefront 0 sums them in a fixed order
    if (tid < 64) {
      double term = 0.0;
      if (tid < n_it) term = ldexp(log(tj_s[tid]), -(tid + 1));
      term = wave_sum_d(term);
      if (tid == 0) ll_s = log(t0) + term;
    }
    __syncthreads();
  }
  const double log_lambda = zero ? 0.0 : ll_s;
  if (tid == 0) {
    const bool first = blockIdx.x == 0;
    if (first && bump) *bump += 1;
    const double sigma = zero ? 0.0 : exp(0.5 * log_lambda);
    if (first && sigma_out) *sigma_out = (float)sigma;
    double sc[LIPASR_MAX_LAYERS];
    sequential_scales(sigma, rho, oa, sc, first ? norms_out : nullptr);
    for (int l = 0; l < oa.n_layers; ++l) {
      sc_s[l] = (float)sc[l];
      if (first && scales_out) scales_out[l] = (float)sc[l];
    }
  }
  __syncthreads();
  int l = 0;
  while (l + 1 < lp.n_layers && (int)blockIdx.x >= lp.wg_start[l + 1]) ++l;
  const size_t j = (size_t)((int)blockIdx.x - lp.wg_start[l]);
  scale_span(lp.W[l], (size_t)lp.rows[l] * lp.cols[l], sc_s[l], j * kSslThreads + threadIdx.x,
             (size_t)(lp.wg_start[l + 1] - lp.wg_start[l]) * kSslThreads);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool sigma_fused_fits(int R, int n0, int n_order) { return n_order > 0 && ssl_lds_bytes(R, n0) <= kSslLdsMax; }

// the step's critical path: chain -> ONE launch that finds sigma and rescales (every workgroup for itself)
int launch_sigma_scale_layers(const float* P, int n0, int R, double rho, const OrderArgs& oa, LayerPtrs lp, float* scales,
                              float* norms_out, float* sigma_out, int* bump, hipStream_t st) {
  const size_t lds = ssl_lds_bytes(R, n0);
  if (lds > kSslLdsDefault) LP_DYN_LDS(sigma_scale_layers_kernel, kSslLdsMax);
  // Workgroups in proportion to the layers' sizes (every one recomputes sigma first -- fp64, the same arithmetic on the same inputs --
  // and they share the CUs' fp64 rate: 64 per layer = 384 took 23.9 us on a 128-CU share, 128 per layer 38.7, 32 per layer 26.6 because
  // layer 1's slice got long)
  size_t total = 0;
  for (int l = 0; l < lp.n_layers; ++l) total += (size_t)lp.rows[l] * lp.cols[l];
  int acc_wg = 0;
  for (int l = 0; l < lp.n_layers; ++l) {
    lp.wg_start[l] = acc_wg;
    const size_t sz = (size_t)lp.rows[l] * lp.cols[l];
    acc_wg += std::max(1, (int)((sz * LIPASR_SIGMA_WGS + total / 2) / total));
  }
  lp.wg_start[lp.n_layers] = acc_wg;
  hipLaunchKernelGGL(sigma_scale_layers_kernel, dim3(acc_wg), dim3(kSslThreads), lds, st, P, n0, R, rho, oa, lp, scales, norms_out,
                     sigma_out, bump);
  k3_count(K3_SIGMA_SCALE_LAYERS);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int launch_product_sigma(const double* gram_part, int n_part, int R, double rho, const OrderArgs& oa, float* scales, float* norms_out,
                         float* sigma_out, int* bump, hipStream_t st) {
  hipLaunchKernelGGL(product_sigma_kernel, dim3(1), dim3(kSigmaThreads), 0, st, gram_part, n_part, R, rho, oa, scales, norms_out,
                     sigma_out, bump);
  k3_count(K3_PRODUCT_SIGMA);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int launch_scale_layers(const LayerPtrs& lp, const float* scales, hipStream_t st) {
  hipLaunchKernelGGL(scale_layers_kernel, dim3(64, lp.n_layers), dim3(256), 0, st, lp, scales);
  k3_count(K3_SCALE_LAYERS);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr
