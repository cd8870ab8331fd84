// K4 in L1 / L2 (and L-inf): the stand-alone step + projection of ART's FastGradientMethod / ProjectedGradientDescent for
// any norm, and the random start of their num_random_init (ART's random_sphere).
//
// lp_step_kernel: one wavefront per row, the row held in registers.  The L1 / L2 direction needs a norm over the WHOLE row
// of g and the projection a norm over the whole row of x' - x0, so every lane must see the row twice; with the row in
// registers, g, x_adv and x0 are read from memory once and x_adv written once (4 x 4 bytes per element, the bandwidth floor),
// and both norms are a lane-serial sum followed by a fixed xor butterfly: no atomics, no LDS, no barrier, and the same bits
// on every run.  A wavefront (not a workgroup) per row because the project's rows are 880 and 2 020 floats: 3.4 and 7.9
// float4 per lane, a register footprint of 3 x 16 and 3 x 32 floats -- a workgroup per row would only add a barrier and an
// LDS round for the two reductions.  Rows stay in registers up to 4 096 floats with 16-byte loads (n a multiple of 4, the
// three bases 16-byte aligned) and up to 1 024 floats with 4-byte loads (ragged widths); longer rows take
// lp_step_stream_kernel, which re-reads the row (three passes) -- no model of the project is that wide.
//
// lp_ball_init_kernel: one wavefront per row, Philox keyed like the dropout masks (gemm.h, DropArgs): key = seed + rank x
// golden ratio, counter = (element group, row, *counter_dev).  Counter-based, so the two passes the L1 / L2 draws need (the
// row's norm, then the scaled write) regenerate the same numbers instead of holding them.
#include "common.h"
#include "row.h"

namespace lipasr {

// (kernels in namespace lipasr itself, not an anonymous one: rocprofv3 traces name them lipasr::lp_step_kernel<VEC, NV>,
// lipasr::lp_step_stream_kernel, lipasr::lp_ball_init_kernel)
constexpr double kLpTol = 1e-7;  // ART's tol = 10e-8 (fast_gradient.py, projection())

// norm codes: 0 = inf, 1 = L1, 2 = L2
__device__ __forceinline__ float sign_nan0(float v) { return (v > 0.0f) ? 1.0f : ((v < 0.0f) ? -1.0f : 0.0f); }

// ART's direction: sign(g) (norm inf) or g / (||g||_p + tol); a row whose ||g||_p is not finite (an inf entry) takes no step
__device__ __forceinline__ float dir_scale(double s, int norm) {
  const double nrm = norm == 1 ? s : sqrt(s);
  return isfinite(nrm) ? (float)(1.0 / (nrm + kLpTol)) : 0.0f;
}

// ART's projection factor min(1, eps / (||dl||_p + tol)) (eps finite)
__device__ __forceinline__ float proj_scale(double s, int norm, float eps) {
  const double nrm = norm == 1 ? s : sqrt(s);
  return (float)fmin(1.0, (double)eps / (nrm + kLpTol));
}

template <int VEC, int NV>
__global__ __launch_bounds__(256) void lp_step_kernel(float* __restrict__ x_adv, const float* __restrict__ x0,
                                                      const float* __restrict__ g, int rows, int n, int norm, float alpha,
                                                      float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int nv = n / VEC;
  const size_t base = (size_t)row * nv;
  float gv[NV][VEC], xa[NV][VEC], xb[NV][VEC];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + 64 * j;
    if (i < nv) {
      ldv<VEC>(g, base + i, gv[j]);
      ldv<VEC>(x_adv, base + i, xa[j]);
      ldv<VEC>(x0, base + i, xb[j]);
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) gv[j][c] = xa[j][c] = xb[j][c] = 0.0f;
    }
  }
  float k = 1.0f;
  if (norm != 0) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        const float v = gv[j][c] != gv[j][c] ? 0.0f : gv[j][c];  // NaN -> 0, as ART zeroes NaN gradients
        gv[j][c] = v;
        s += norm == 1 ? (double)fabsf(v) : (double)v * (double)v;
      }
    k = dir_scale(wave_sum_d(s), norm);
  }
  // x' = x_adv + alpha d, then dl = x' - x0 (kept in gv)
  double s2 = 0.0;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      const float d = norm == 0 ? sign_nan0(gv[j][c]) : (isfinite(gv[j][c]) ? gv[j][c] * k : 0.0f);  // k = 0: no step
      const float xp = xa[j][c] + alpha * d;
      const float dl = xp - xb[j][c];
      xa[j][c] = xp;
      gv[j][c] = dl;
      s2 += norm == 1 ? (double)fabsf(dl) : (double)dl * (double)dl;
    }
  const bool noproj = isinf(eps);
  float f = 1.0f;
  if (!noproj && norm != 0) f = proj_scale(wave_sum_d(s2), norm, eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + 64 * j;
    if (i >= nv) continue;
    float o[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      if (noproj) o[c] = xa[j][c];
      else if (norm == 0) o[c] = xb[j][c] + fminf(fmaxf(gv[j][c], -eps), eps);  // = K4's sign step, bit for bit
      else o[c] = xb[j][c] + gv[j][c] * f;
    }
    stv<VEC>(x_adv, base + i, o);
  }
}

// rows wider than the register-resident instances: the same arithmetic in the same summation order per lane, three passes
__global__ __launch_bounds__(256) void lp_step_stream_kernel(float* __restrict__ x_adv, const float* __restrict__ x0,
                                                             const float* __restrict__ g, int rows, int n, int norm, float alpha,
                                                             float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const size_t base = (size_t)row * n;
  auto gz = [&](int i) { const float v = g[base + i]; return v != v ? 0.0f : v; };
  float k = 1.0f;
  if (norm != 0) {
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {
      const float v = gz(i);
      s += norm == 1 ? (double)fabsf(v) : (double)v * (double)v;
    }
    k = dir_scale(wave_sum_d(s), norm);
  }
  auto dl_at = [&](int i, float& xp) {
    const float v = gz(i);
    xp = x_adv[base + i] + alpha * (norm == 0 ? sign_nan0(v) : (isfinite(v) ? v * k : 0.0f));
    return xp - x0[base + i];
  };
  const bool noproj = isinf(eps);
  float f = 1.0f;
  if (!noproj && norm != 0) {
    double s2 = 0.0;
    for (int i = lane; i < n; i += 64) {
      float xp;
      const float dl = dl_at(i, xp);
      s2 += norm == 1 ? (double)fabsf(dl) : (double)dl * (double)dl;
    }
    f = proj_scale(wave_sum_d(s2), norm, eps);
  }
  for (int i = lane; i < n; i += 64) {
    float xp;
    const float dl = dl_at(i, xp);
    const float b = x0[base + i];
    x_adv[base + i] = noproj ? xp : (norm == 0 ? b + fminf(fmaxf(dl, -eps), eps) : b + dl * f);
  }
}

// ---- random start
constexpr uint64_t kRowCtr = 0xFFFFFFFF00000000ull;  // Philox counter of the row-level draw (element groups stay below 2^30)

__device__ __forceinline__ void ball_draw4(int norm, uint64_t key, uint64_t q, uint32_t row, uint32_t ctr, float (&v)[4],
                                           float (&sg)[4]) {
  uint32_t o[4];
  Philox::gen(key, q, row, ctr, o);
  if (norm == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = 2.0f * Philox::u01(o[c]) - 1.0f;  // uniform on (-1, 1]
  } else if (norm == 2) {  // Box-Muller: four standard normals
    const float r0 = sqrtf(-2.0f * logf(Philox::u01(o[0]))), r1 = sqrtf(-2.0f * logf(Philox::u01(o[2])));
    const float t0 = 6.283185307179586f * Philox::u01(o[1]), t1 = 6.283185307179586f * Philox::u01(o[3]);
    v[0] = r0 * cosf(t0); v[1] = r0 * sinf(t0); v[2] = r1 * cosf(t1); v[3] = r1 * sinf(t1);
  } else {  // standard exponentials (u01 uses the top 24 bits; bit 0 is the independent random sign)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = -logf(Philox::u01(o[c]));
      sg[c] = (o[c] & 1u) ? -1.0f : 1.0f;
    }
  }
}

__global__ __launch_bounds__(256) void lp_ball_init_kernel(float* __restrict__ x_adv, const float* __restrict__ x0, int rows,
                                                           int n, int norm, float eps, uint64_t seed, const int* counter_dev,
                                                           int rank) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint64_t key = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(uint32_t)rank;  // as the dropout key folds the replica rank
  const uint32_t ctr = counter_dev ? (uint32_t)*counter_dev : 0u;
  const size_t base = (size_t)row * n;
  const int nq = (n + 3) / 4;
  float fac = eps;  // L-inf: eps x uniform on (-1, 1]
  if (norm != 0) {
    double s = 0.0;
    for (int q = lane; q < nq; q += 64) {
      float v[4], sg[4];
      ball_draw4(norm, key, (uint64_t)q, (uint32_t)row, ctr, v, sg);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * q + c < n) s += norm == 2 ? (double)v[c] * (double)v[c] : (double)v[c];
    }
    s = wave_sum_d(s);
    uint32_t o[4];
    Philox::gen(key, kRowCtr, (uint32_t)row, ctr, o);
    const double u = (double)Philox::u01(o[0]);
    // L2: radius eps U^(1/n) (uniform in the ball), direction a / |a|.  L1: ART's radius eps sqrt(U), split by r E_i / sum E
    // (the gaps of n-1 sorted uniforms on [0, r]), each with a random sign.
    const double r = norm == 2 ? (double)eps * exp(log(u) / (double)n) : (double)eps * sqrt(u);
    fac = s > 0.0 ? (float)(r / (norm == 2 ? sqrt(s) : s)) : 0.0f;
  }
  for (int q = lane; q < nq; q += 64) {
    float v[4], sg[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    ball_draw4(norm, key, (uint64_t)q, (uint32_t)row, ctr, v, sg);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = 4 * q + c;
      if (i < n) x_adv[base + i] = x0[base + i] + sg[c] * (v[c] * fac);
    }
  }
}

template <int VEC, int NV>
static void launch_lp(dim3 grid, hipStream_t st, float* x_adv, const float* x0, const float* g, int rows, int n, int norm, float alpha,
               float eps) {
  hipLaunchKernelGGL((lp_step_kernel<VEC, NV>), grid, dim3(256), 0, st, x_adv, x0, g, rows, n, norm, alpha, eps);
}

static int norm_code(float norm, int* code) {
  if (std::isinf(norm) && norm > 0.0f) *code = 0;
  else if (norm == 1.0f) *code = 1;
  else if (norm == 2.0f) *code = 2;
  else return LIPASR_EINVAL;
  return LIPASR_OK;
}

int lp_norm_code(const char* fn, float norm, int* code) {
  if (norm_code(norm, code) != LIPASR_OK) {
    set_error("%s: norm=%g; 1, 2 and inf are supported", fn, (double)norm);
    return LIPASR_EINVAL;
  }
  return LIPASR_OK;
}

int lp_step_launch(float* x_adv, const float* x0, const float* g, int rows, int n, int norm, float alpha, float eps,
                   hipStream_t st) {
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool al16 = (n % 4 == 0) && ((reinterpret_cast<uintptr_t>(x_adv) | reinterpret_cast<uintptr_t>(x0) |
                                      reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const int per_lane = al16 ? (n / 4 + 63) / 64 : (n + 63) / 64;  // vectors per lane
  if (al16 && per_lane <= 1) launch_lp<4, 1>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);
  else if (al16 && per_lane <= 2) launch_lp<4, 2>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);
  else if (al16 && per_lane <= 4) launch_lp<4, 4>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);   // 880
  else if (al16 && per_lane <= 8) launch_lp<4, 8>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);   // 2 020
  else if (al16 && per_lane <= 16) launch_lp<4, 16>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);
  else if (!al16 && per_lane <= 4) launch_lp<1, 4>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);
  else if (!al16 && per_lane <= 16) launch_lp<1, 16>(grid, st, x_adv, x0, g, rows, n, norm, alpha, eps);
  else hipLaunchKernelGGL(lp_step_stream_kernel, grid, dim3(256), 0, st, x_adv, x0, g, rows, n, norm, alpha, eps);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_lp_step(lipasr_handle_t h, float* x_adv, const float* x0, const float* g, int rows, int n, float norm, float alpha,
                   float eps, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && x_adv && x0 && g, "lipasr_lp_step: null argument");
  LP_CHECK_ARG(rows >= 0 && n >= 0, "lipasr_lp_step: bad shape %dx%d", rows, n);
  LP_CHECK_ARG(eps >= 0.0f && !(alpha != alpha), "lipasr_lp_step: eps=%g alpha=%g", (double)eps, (double)alpha);
  int code = 0;
  int rc = lp_norm_code("lipasr_lp_step", norm, &code);
  if (rc != LIPASR_OK) return rc;
  if (rows == 0 || n == 0) return LIPASR_OK;
  return lp_step_launch(x_adv, x0, g, rows, n, code, alpha, eps, S(stream));
}

int lipasr_lp_ball_init(lipasr_handle_t h, float* x_adv, const float* x0, int rows, int n, float norm, float eps, uint64_t seed,
                        const int* counter_dev, int rank, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && x_adv && x0, "lipasr_lp_ball_init: null argument");
  LP_CHECK_ARG(rows >= 0 && n >= 0, "lipasr_lp_ball_init: bad shape %dx%d", rows, n);
  LP_CHECK_ARG(eps >= 0.0f && !std::isinf(eps), "lipasr_lp_ball_init: eps=%g must be finite and non-negative", (double)eps);
  int code = 0;
  int rc = lp_norm_code("lipasr_lp_ball_init", norm, &code);
  if (rc != LIPASR_OK) return rc;
  if (rows == 0 || n == 0) return LIPASR_OK;
  hipLaunchKernelGGL(lp_ball_init_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S(stream), x_adv, x0, rows, n, code, eps,
                     seed, counter_dev, rank);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // extern "C"
