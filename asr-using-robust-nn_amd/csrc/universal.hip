// Universal adversarial perturbations (Moosavi-Dezfooli et al. 2017; over audio: Vadillo and Santana 2019, Neekhara et al. 2019):
// ONE noise vector of period P shared by every row of a batch.  The four kernels around the estimator's gradient, and their host
// restatements.  (include/lipasr.h, lipasr_universal_shifts / _apply / _reduce / _step, fixes the conventions.)
//
// Position k of row b is paired with noise[(k + offs[b]) mod P]: the noise loops where P < n, and a row sees a window of it where
// P > n.  Every other attack kernel is row-local; universal_reduce_kernel is the one that sums ACROSS rows.
//
// universal_shifts_kernel: one thread per row, one Philox block each.
//
// universal_apply_kernel: grid (ceil(n / 2048), batch).  A thread owns eight single elements of one row, 256 apart, so that every
//   wave-instruction reads or writes 64 consecutive dwords whatever the alignment of the row: a row of 22 050 floats starts on
//   16 bytes only every other row, and the row's shift moves the noise off any alignment in any case.  (Quads as float4 where a
//   row allows and four scalars where not measured 58.6 us at 1024 x 22 050, this form 37.8 us, a copy 31.5 us: DESIGN.md.)
//
// universal_reduce_kernel: grid (ceil(P / 256), groups), a group being LIPASR_UNIVERSAL_GROUP consecutive rows.  A LANE OWNS ONE
//   PERIOD POSITION p, consecutive lanes consecutive p, and walks the rows of its group in ascending order; in row b it reads
//   k = (p - offs[b]) mod P, k + P, k + 2 P, ... below nv_b.  Consecutive lanes read consecutive dwords (one break per row where
//   the shift wraps), so every wave-instruction is coalesced.  The sum is a chain of fp64 additions in an order that depends on
//   (batch, P) alone -- no atomics, no exchange between lanes, no partials whose count depends on the grid -- and the lane
//   stores it: sums is written, never added to.  The shifts and lengths of the group's rows go through LDS once, so that the
//   loads of a row do not wait on a scalar load of their own; with P >= n (ONE: the workload's shape) a row gives a lane at most
//   one element and the row loop unrolls into independent loads; with P < n the loop runs over (row, wrap) pairs, flat, and
//   unrolls the same way.
//
// universal_step_kernel (norm inf): element-wise, grid ceil(P / 256).  universal_step2_kernel (norm 2): ONE launch of ONE workgroup
//   of 1024 threads, three passes over P (sum G^2; sum d'^2; write), the group partials re-added in every pass rather than kept:
//   P <= 2^17 and the partials are L2-resident, and a second launch would cost more than the passes.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kUnThreads = 256;
constexpr int kUnApplyPer = 8;  // elements of a row per thread of universal_apply_kernel, kUnThreads apart
constexpr int kUnStep2Threads = 1024;
constexpr int kUnMaxBatch = 65535;
constexpr int kUnMaxN = 1 << 17;
constexpr uint32_t kUnTag = 0x554E4956u;  // "UNIV": counter word 3 of every shift draw
constexpr double kUnTol = 1e-7;           // lipasr_lp_step's tol

// the shift of row b, reduced into [0, P) whatever the caller passed
__host__ __device__ __forceinline__ int universal_off(const int* offs, int b, int P) {
  if (!offs) return 0;
  const int r = offs[b] % P;
  return r < 0 ? r + P : r;
}

__host__ __device__ __forceinline__ int universal_shift(uint64_t seed, uint32_t clip, uint32_t it, int P) {
  uint32_t o[4];
  Philox::gen(seed, (uint64_t)clip, it, kUnTag, o);
  return (int)(((uint64_t)o[0] * (uint64_t)P) >> 32);
}

// acc + g, a NaN counting as 0
__host__ __device__ __forceinline__ double universal_add(double acc, float g) { return g == g ? acc + (double)g : acc; }

// the first position of a row that period position p is paired with: (p - off) mod P
__host__ __device__ __forceinline__ int universal_first(int p, int off, int P) { return p >= off ? p - off : p - off + P; }

// G[p]: the group partials in ascending group order
__host__ __device__ __forceinline__ double universal_total(const double* __restrict__ sums, int groups, int P, int p) {
  double G = 0.0;
  for (int grp = 0; grp < groups; ++grp) G += sums[(size_t)grp * P + p];
  return G;
}

// alpha * sign(G) is +-alpha or +-0 exactly, so a contraction of the add changes nothing
__host__ __device__ __forceinline__ float universal_step_inf(float noise, double G, float alpha, float eps) {
  const float s = G > 0.0 ? 1.0f : (G < 0.0 ? -1.0f : 0.0f);
  return clampf(noise + alpha * s, -eps, eps);
}

// d' of the norm-2 step; step: N is finite
__host__ __device__ __forceinline__ double universal_step2_d(float noise, double G, float alpha, double N, bool step) {
  return step ? (double)noise + ((double)alpha * G) / (N + kUnTol) : (double)noise;
}
__host__ __device__ __forceinline__ double universal_scale(double M, float eps) {
  if (!(eps < INFINITY)) return 1.0;
  const double r = (double)eps / (M + kUnTol);
  return r < 1.0 ? r : 1.0;
}
__host__ __device__ __forceinline__ bool universal_finite(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(kUnThreads) void universal_shifts_kernel(int batch, int P, uint32_t clip0, uint32_t it, uint64_t seed,
                                                                       int* __restrict__ offs) {
  const int b = blockIdx.x * kUnThreads + threadIdx.x;
  if (b < batch) offs[b] = universal_shift(seed, clip0 + (uint32_t)b, it, P);
}

__global__ __launch_bounds__(kUnThreads) void universal_apply_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                                      const int* __restrict__ offs, const int* __restrict__ n_valid,
                                                                      int n, int P, float lo, float hi, float* __restrict__ out) {
  const int b = blockIdx.y;
  const float* __restrict__ xr = x + (size_t)b * n;
  float* __restrict__ orow = out + (size_t)b * n;
  const int nv = row_valid(n_valid, b, n);
  const int off = universal_off(offs, b, P);
  const int k0 = blockIdx.x * (kUnThreads * kUnApplyPer) + threadIdx.x;
  float v[kUnApplyPer], z[kUnApplyPer];
  // the loads first, all of them in flight; element i of the thread is k0 + 256 i
#pragma unroll
  for (int i = 0; i < kUnApplyPer; ++i) {
    const int k = k0 + i * kUnThreads;
    v[i] = k < n ? xr[k] : 0.0f;
    z[i] = k < nv ? noise[(unsigned)(k + off) % (unsigned)P] : 0.0f;  // k + off < 2^18
  }
#pragma unroll
  for (int i = 0; i < kUnApplyPer; ++i) {
    const int k = k0 + i * kUnThreads;
    if (k < n) orow[k] = k < nv ? clampf(v[i] + z[i], lo, hi) : v[i];
  }
}

template <bool ONE>
__global__ __launch_bounds__(kUnThreads) void universal_reduce_kernel(const float* __restrict__ g, const int* __restrict__ offs,
                                                                       const int* __restrict__ n_valid, int batch, int n, int P,
                                                                       double* __restrict__ sums) {
  __shared__ int s_off[LIPASR_UNIVERSAL_GROUP], s_nv[LIPASR_UNIVERSAL_GROUP];
  const int grp = blockIdx.y, tid = threadIdx.x;
  const int b0 = grp * LIPASR_UNIVERSAL_GROUP;
  const int rows = min(LIPASR_UNIVERSAL_GROUP, batch - b0);
  if (tid < rows) {
    s_off[tid] = universal_off(offs, b0 + tid, P);
    s_nv[tid] = row_valid(n_valid, b0 + tid, n);
  }
  __syncthreads();
  const int p = blockIdx.x * kUnThreads + tid;
  if (p >= P) return;
  const float* __restrict__ gr = g + (size_t)b0 * n;
  double acc = 0.0;
  if constexpr (ONE) {  // P >= n: at most one position of a row per lane
#pragma unroll 16
    for (int r = 0; r < rows; ++r) {
      const int k = universal_first(p, s_off[r], P);
      const float v = k < s_nv[r] ? gr[(size_t)r * n + k] : 0.0f;
      acc = universal_add(acc, v);
    }
  } else {
    // P < n: a row gives a lane up to wraps = ceil(n / P) positions.  One flat loop over (row, wrap) with a guarded load, so
    // that it unrolls into independent loads as above; a position at or beyond nv_b adds +0.0, which changes no bit of an
    // accumulator that started at +0.0 (it is never -0.0).
    const int wraps = (n + P - 1) / P;
    int r = 0, j = 0;
#pragma unroll 16
    for (int i = 0; i < rows * wraps; ++i) {
      const int k = universal_first(p, s_off[r], P) + j * P;
      const float v = k < s_nv[r] ? gr[(size_t)r * n + k] : 0.0f;
      acc = universal_add(acc, v);
      if (++j == wraps) { j = 0; ++r; }
    }
  }
  sums[(size_t)grp * P + p] = acc;
}

__global__ __launch_bounds__(kUnThreads) void universal_step_kernel(float* __restrict__ noise, const double* __restrict__ sums,
                                                                     int groups, int P, float alpha, float eps) {
  const int p = blockIdx.x * kUnThreads + threadIdx.x;
  if (p < P) noise[p] = universal_step_inf(noise[p], universal_total(sums, groups, P, p), alpha, eps);
}

// Thread t takes p = t, t + 1024, ... in ascending order into one fp64 partial; the partials meet in block_sum_d's order.
__global__ __launch_bounds__(kUnStep2Threads) void universal_step2_kernel(float* __restrict__ noise, const double* __restrict__ sums,
                                                                           int groups, int P, float alpha, float eps) {
  __shared__ double red[kUnStep2Threads / 64];
  const int tid = threadIdx.x;
  double part = 0.0;
  for (int p = tid; p < P; p += kUnStep2Threads) {
    const double G = universal_total(sums, groups, P, p);
    part += G * G;
  }
  const double N = sqrt(block_sum_d<kUnStep2Threads>(part, red));
  const bool step = universal_finite(N);
  part = 0.0;
  for (int p = tid; p < P; p += kUnStep2Threads) {
    const double d = universal_step2_d(noise[p], universal_total(sums, groups, P, p), alpha, N, step);
    part += d * d;
  }
  const double scale = universal_scale(sqrt(block_sum_d<kUnStep2Threads>(part, red)), eps);
  for (int p = tid; p < P; p += kUnStep2Threads)
    noise[p] = (float)(universal_step2_d(noise[p], universal_total(sums, groups, P, p), alpha, N, step) * scale);
}

// the checks the device entry points and their host twins share
static int universal_shape(const char* fn, int batch, int n, int P) {
  LP_CHECK_ARG(batch >= 0 && n >= 0 && P >= 0, "%s: bad shape %d x %d, period %d", fn, batch, n, P);
  LP_CHECK_ARG(batch <= kUnMaxBatch, "%s: %d rows; at most %d", fn, batch, kUnMaxBatch);
  LP_CHECK_ARG(n <= kUnMaxN, "%s: rows of %d; at most %d", fn, n, kUnMaxN);
  LP_CHECK_ARG(P <= kUnMaxN, "%s: period %d; at most %d", fn, P, kUnMaxN);
  return LIPASR_OK;
}

static int universal_apply_check(const char* fn, const float* x, const float* noise, int batch, int n, int P, float lo, float hi,
                                 const float* out) {
  LP_CHECK_ARG(x != nullptr && noise != nullptr && out != nullptr, "%s: a null pointer", fn);
  LP_CHECK_ARG(lo <= hi, "%s: clip range [%g, %g]", fn, (double)lo, (double)hi);
  const size_t bytes = (size_t)batch * n * sizeof(float);
  LP_CHECK_ARG(!spans_overlap(out, bytes, x, bytes), "%s: out overlaps x", fn);
  LP_CHECK_ARG(!spans_overlap(out, bytes, noise, (size_t)P * sizeof(float)), "%s: out overlaps noise", fn);
  return LIPASR_OK;
}

static int universal_reduce_check(const char* fn, const float* g, int batch, int n, int P, const double* sums) {
  LP_CHECK_ARG(g != nullptr && sums != nullptr, "%s: a null pointer", fn);
  const size_t groups = ((size_t)batch + LIPASR_UNIVERSAL_GROUP - 1) / LIPASR_UNIVERSAL_GROUP;
  LP_CHECK_ARG(!spans_overlap(sums, groups * P * sizeof(double), g, (size_t)batch * n * sizeof(float)), "%s: sums overlaps g", fn);
  return LIPASR_OK;
}

static int universal_step_check(const char* fn, int groups, int P, float norm, float alpha, float eps) {
  LP_CHECK_ARG(groups >= 0 && P >= 0, "%s: bad shape %d groups, period %d", fn, groups, P);
  LP_CHECK_ARG(groups <= (kUnMaxBatch + LIPASR_UNIVERSAL_GROUP - 1) / LIPASR_UNIVERSAL_GROUP, "%s: %d groups; at most %d", fn, groups,
               (kUnMaxBatch + LIPASR_UNIVERSAL_GROUP - 1) / LIPASR_UNIVERSAL_GROUP);
  LP_CHECK_ARG(P <= kUnMaxN, "%s: period %d; at most %d", fn, P, kUnMaxN);
  LP_CHECK_ARG(norm == 2.0f || norm == INFINITY, "%s: norm %g; 2 or inf", fn, (double)norm);
  LP_CHECK_ARG(alpha - alpha == 0.0f, "%s: alpha %g", fn, (double)alpha);
  LP_CHECK_ARG(eps >= 0.0f, "%s: eps %g", fn, (double)eps);
  return LIPASR_OK;
}

static int universal_step_pointers(const char* fn, const float* noise, const double* sums, int groups, int P) {
  LP_CHECK_ARG(noise != nullptr && sums != nullptr, "%s: a null pointer", fn);
  LP_CHECK_ARG(!spans_overlap(noise, (size_t)P * sizeof(float), sums, (size_t)groups * P * sizeof(double)), "%s: noise overlaps sums", fn);
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_universal_shifts(lipasr_handle_t h, int batch, int P, uint32_t clip0, uint32_t it, uint64_t seed, int* offs_out,
                            lipasr_stream_t stream) {
  const char* fn = "lipasr_universal_shifts";
  if (int rc = universal_shape(fn, batch, 0, P)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || P == 0) return LIPASR_OK;
  LP_CHECK_ARG(offs_out != nullptr, "%s: a null pointer", fn);
  hipLaunchKernelGGL(universal_shifts_kernel, dim3((unsigned)((batch + kUnThreads - 1) / kUnThreads)), dim3(kUnThreads), 0, S(stream),
                     batch, P, clip0, it, seed, offs_out);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_universal_shifts_host(int batch, int P, uint32_t clip0, uint32_t it, uint64_t seed, int* offs_out) {
  const char* fn = "lipasr_universal_shifts_host";
  if (int rc = universal_shape(fn, batch, 0, P)) return rc;
  if (batch == 0 || P == 0) return LIPASR_OK;
  LP_CHECK_ARG(offs_out != nullptr, "%s: a null pointer", fn);
  for (int b = 0; b < batch; ++b) offs_out[b] = universal_shift(seed, clip0 + (uint32_t)b, it, P);
  return LIPASR_OK;
}

int lipasr_universal_apply(lipasr_handle_t h, const float* x, const float* noise, const int* offs, const int* n_valid, int batch, int n,
                           int P, float clip_lo, float clip_hi, float* out, lipasr_stream_t stream) {
  const char* fn = "lipasr_universal_apply";
  if (int rc = universal_shape(fn, batch, n, P)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0 || P == 0) return LIPASR_OK;
  if (int rc = universal_apply_check(fn, x, noise, batch, n, P, clip_lo, clip_hi, out)) return rc;
  const int per_block = kUnThreads * kUnApplyPer;
  hipLaunchKernelGGL(universal_apply_kernel, dim3((unsigned)((n + per_block - 1) / per_block), (unsigned)batch), dim3(kUnThreads), 0,
                     S(stream), x, noise, offs, n_valid, n, P, clip_lo, clip_hi, out);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_universal_apply_host(const float* x, const float* noise, const int* offs, const int* n_valid, int batch, int n, int P,
                                float clip_lo, float clip_hi, float* out) {
  const char* fn = "lipasr_universal_apply_host";
  if (int rc = universal_shape(fn, batch, n, P)) return rc;
  if (batch == 0 || n == 0 || P == 0) return LIPASR_OK;
  if (int rc = universal_apply_check(fn, x, noise, batch, n, P, clip_lo, clip_hi, out)) return rc;
  for (int b = 0; b < batch; ++b) {
    const float* xr = x + (size_t)b * n;
    float* orow = out + (size_t)b * n;
    const int nv = row_valid(n_valid, b, n);
    int j = universal_off(offs, b, P);
    for (int k = 0; k < n; ++k) {
      orow[k] = k < nv ? clampf(xr[k] + noise[j], clip_lo, clip_hi) : xr[k];
      j = j + 1 == P ? 0 : j + 1;
    }
  }
  return LIPASR_OK;
}

int lipasr_universal_reduce(lipasr_handle_t h, const float* g, const int* offs, const int* n_valid, int batch, int n, int P,
                            double* sums, lipasr_stream_t stream) {
  const char* fn = "lipasr_universal_reduce";
  if (int rc = universal_shape(fn, batch, n, P)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0 || P == 0) return LIPASR_OK;
  if (int rc = universal_reduce_check(fn, g, batch, n, P, sums)) return rc;
  const dim3 grid((unsigned)((P + kUnThreads - 1) / kUnThreads), (unsigned)((batch + LIPASR_UNIVERSAL_GROUP - 1) / LIPASR_UNIVERSAL_GROUP));
  if (P >= n)
    hipLaunchKernelGGL(universal_reduce_kernel<true>, grid, dim3(kUnThreads), 0, S(stream), g, offs, n_valid, batch, n, P, sums);
  else
    hipLaunchKernelGGL(universal_reduce_kernel<false>, grid, dim3(kUnThreads), 0, S(stream), g, offs, n_valid, batch, n, P, sums);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_universal_reduce_host(const float* g, const int* offs, const int* n_valid, int batch, int n, int P, double* sums) {
  const char* fn = "lipasr_universal_reduce_host";
  if (int rc = universal_shape(fn, batch, n, P)) return rc;
  if (batch == 0 || n == 0 || P == 0) return LIPASR_OK;
  if (int rc = universal_reduce_check(fn, g, batch, n, P, sums)) return rc;
  for (int b0 = 0; b0 < batch; b0 += LIPASR_UNIVERSAL_GROUP) {
    double* out = sums + (size_t)(b0 / LIPASR_UNIVERSAL_GROUP) * P;
    const int rows = std::min(LIPASR_UNIVERSAL_GROUP, batch - b0);
    for (int p = 0; p < P; ++p) {
      double acc = 0.0;
      for (int r = 0; r < rows; ++r) {
        const int nv = row_valid(n_valid, b0 + r, n);
        const float* row = g + (size_t)(b0 + r) * n;
        for (int k = universal_first(p, universal_off(offs, b0 + r, P), P); k < nv; k += P) acc = universal_add(acc, row[k]);
      }
      out[p] = acc;
    }
  }
  return LIPASR_OK;
}

int lipasr_universal_step(lipasr_handle_t h, float* noise, const double* sums, int groups, int P, float norm, float alpha, float eps,
                          lipasr_stream_t stream) {
  const char* fn = "lipasr_universal_step";
  if (int rc = universal_step_check(fn, groups, P, norm, alpha, eps)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (groups == 0 || P == 0) return LIPASR_OK;
  if (int rc = universal_step_pointers(fn, noise, sums, groups, P)) return rc;
  if (norm == 2.0f)
    hipLaunchKernelGGL(universal_step2_kernel, dim3(1), dim3(kUnStep2Threads), 0, S(stream), noise, sums, groups, P, alpha, eps);
  else
    hipLaunchKernelGGL(universal_step_kernel, dim3((unsigned)((P + kUnThreads - 1) / kUnThreads)), dim3(kUnThreads), 0, S(stream), noise,
                       sums, groups, P, alpha, eps);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_universal_step_host(float* noise, const double* sums, int groups, int P, float norm, float alpha, float eps) {
  const char* fn = "lipasr_universal_step_host";
  if (int rc = universal_step_check(fn, groups, P, norm, alpha, eps)) return rc;
  if (groups == 0 || P == 0) return LIPASR_OK;
  if (int rc = universal_step_pointers(fn, noise, sums, groups, P)) return rc;
  if (norm != 2.0f) {
    for (int p = 0; p < P; ++p) noise[p] = universal_step_inf(noise[p], universal_total(sums, groups, P, p), alpha, eps);
    return LIPASR_OK;
  }
  double acc = 0.0;
  for (int p = 0; p < P; ++p) {
    const double G = universal_total(sums, groups, P, p);
    acc += G * G;
  }
  const double N = std::sqrt(acc);
  const bool step = universal_finite(N);
  acc = 0.0;
  for (int p = 0; p < P; ++p) {
    const double d = universal_step2_d(noise[p], universal_total(sums, groups, P, p), alpha, N, step);
    acc += d * d;
  }
  const double scale = universal_scale(std::sqrt(acc), eps);
  for (int p = 0; p < P; ++p)
    noise[p] = (float)(universal_step2_d(noise[p], universal_total(sums, groups, P, p), alpha, N, step) * scale);
  return LIPASR_OK;
}

}  // extern "C"
