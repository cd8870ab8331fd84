// DeepFool (Moosavi-Dezfooli et al. 2016): one iteration of the minimal-perturbation attack for a batch, in place on x.  Per row b
// the class gradients J_b[c][k] (jac[b * stride_b + c * stride_c + k], the layouts of lipasr_jacobian_sigma), the outputs out[b][.]
// at x_b and the class c = label[b] the row started in give, for every other class k the mask allows,
//     w_k = J_k - J_c,   f_k = out_k - out_c,   rho_k = |f_k| / (||w_k||_q + tol)      (q = 2 for norm 2, q = 1 for norm inf)
// the distance to the linearised boundary of class k; l = argmin rho_k, and x_b moves by (1 + overshoot) r with
//     norm 2: r = |f_l| / (||w_l||_2^2 + tol) w_l        norm inf: r = |f_l| / (||w_l||_1 + tol) sign(w_l)
// (include/lipasr.h, lipasr_deepfool_step, fixes the conventions; tol = 1e-7 is ART's 10e-8, kLpTol of lp_attack.hip).
//
// deepfool_step_kernel<VEC, NORM>: ONE workgroup of 256 threads per row, one launch per call, no workspace, no atomics.
//   out     every thread reads the row's C <= 32 outputs (the same addresses in every lane): a NaN or inf ends the row (state -1),
//           an argmax that is no longer c ends it too (state 0, x untouched).
//   norms   a lane takes columns tid, tid + 256, ... (VEC = 4: four adjacent columns, one 16-byte load per row), holds row c of
//           them and reads the other rows four at a time, so J is read once and consecutive lanes read consecutive addresses.
//           w = J_k - J_c and the terms w^2 (or |w|) are formed in fp64 and summed lane-serially in fp64 (n / 256 <= 87 terms
//           each): the squares of a saturated softmax's ~1e-30 Jacobian are not fp32 numbers, and fp64 holds the square of every
//           finite fp32 difference, so no scaling pass over J is needed.  Then wave_sum_d and the four waves in a fixed order
//           through LDS, as jacobian.hip sums its Gram matrix: the same bits on every run.
//   argmin  thread k forms rho_k; every thread scans the C values in LDS (lowest index on a tie).  A class whose norm is not finite
//           (a NaN or inf in J_k or J_c) is never chosen; no class left: state -1.
//   step    rows l and c and x are read once more; the step's factor is fp64, each x is rounded once.  A column with w_l = 0 (a
//           ragged clip's padding) keeps the bits of x.
// VEC = 4 needs n, both strides and the bases of jac and x multiples of 16 bytes; anything else takes VEC = 1.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kDfMaxC = 32;
constexpr int kDfThreads = 256;
constexpr int kDfWaves = kDfThreads / 64;
constexpr int kDfGroup = 4;       // rows of J in flight per lane
constexpr double kDfTol = 1e-7;   // ART's tol = 10e-8 (deepfool.py)

struct DeepfoolArgs {
  const float* jac;
  long stride_b, stride_c;
  const float* out;
  const int* label;
  const uint32_t* allowed;  // or null
  int C, n;
  float overshoot, lo, hi;
  float* x;
  float* dist;  // or null
  int* target;  // or null
  int* state;   // or null
};

__device__ __forceinline__ void df_result(const DeepfoolArgs& a, size_t b, float dist, int target, int state) {
  if (a.dist) a.dist[b] = dist;
  if (a.target) a.target[b] = target;
  if (a.state) a.state[b] = state;
}

// NORM: 2, or 0 for inf
template <int VEC, int NORM>
__global__ __launch_bounds__(kDfThreads) void deepfool_step_kernel(DeepfoolArgs a) {
  __shared__ double part[kDfWaves][kDfMaxC];
  __shared__ double nrm[kDfMaxC];  // ||w_k||_2^2 or ||w_k||_1
  __shared__ double rho[kDfMaxC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, n = a.n, nv = n / VEC;
  const size_t b = blockIdx.x;
  const float* __restrict__ out = a.out + b * (size_t)C;

  // ---- the outputs: finite?  still in class c?  (identical in every thread)
  const int c = a.label[b];
  bool bad = c < 0 || c >= C;
  int am = 0;
  float top = out[0];
  for (int k = 0; k < C; ++k) {
    const float v = out[k];
    bad |= !(fabsf(v) < INFINITY);
    if (v > top) { top = v; am = k; }
  }
  if (bad) {
    if (tid == 0) df_result(a, b, NAN, -1, -1);
    return;
  }
  if (am != c) {
    if (tid == 0) df_result(a, b, 0.0f, am, 0);
    return;
  }
  const uint32_t mask = a.allowed ? a.allowed[b] : 0xffffffffu;
  const float* __restrict__ J = a.jac + b * (size_t)a.stride_b;
  const float* __restrict__ Jc = J + (size_t)c * a.stride_c;

  // ---- sum_k' w_k[k']^2 (or |w_k[k']|) for every class at once.  Rows past C - 1 re-read row C - 1 (their sums are not used), so
  // that the kDfGroup loads of a group need no test of their own and are in flight together.
  double acc[kDfMaxC];
#pragma unroll
  for (int k = 0; k < kDfMaxC; ++k) acc[k] = 0.0;
  for (int i = tid; i < nv; i += kDfThreads) {
    float jc[VEC];
    ldv<VEC>(Jc, i, jc);
#pragma unroll
    for (int g = 0; g < kDfMaxC; g += kDfGroup) {
      if (g < C) {  // uniform
        float jk[kDfGroup][VEC];
#pragma unroll
        for (int r = 0; r < kDfGroup; ++r) ldv<VEC>(J + (size_t)min(g + r, C - 1) * a.stride_c, i, jk[r]);
#pragma unroll
        for (int r = 0; r < kDfGroup; ++r)
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const double w = (double)jk[r][e] - (double)jc[e];
            acc[g + r] = (NORM == 2) ? fma(w, w, acc[g + r]) : acc[g + r] + fabs(w);
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kDfMaxC; ++k) {
    if (k < C) {  // uniform
      const double d = wave_sum_d(acc[k]);
      if (lane == 0) part[wave][k] = d;
    }
  }
  __syncthreads();

  // ---- rho_k, then its smallest (lowest index on a tie)
  if (tid < C) {
    const double s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const bool cand = tid != c && ((mask >> tid) & 1u) && s < (double)INFINITY;  // (a NaN sum fails the comparison)
    const double f = fabs((double)out[tid] - (double)out[c]);
    nrm[tid] = s;
    rho[tid] = cand ? f / ((NORM == 2 ? sqrt(s) : s) + kDfTol) : (double)INFINITY;
  }
  __syncthreads();
  int l = -1;
  double best = (double)INFINITY;
  for (int k = 0; k < C; ++k)
    if (rho[k] < best) { best = rho[k]; l = k; }
  if (l < 0) {  // the same in every thread
    if (tid == 0) df_result(a, b, NAN, -1, -1);
    return;
  }
  if (tid == 0) df_result(a, b, (float)best, l, 1);

  // ---- x <- clamp(x + (1 + overshoot) r)
  const double step = (1.0 + (double)a.overshoot) * fabs((double)out[l] - (double)out[c]) / (nrm[l] + kDfTol);
  const float stepf = (float)step;
  const float* __restrict__ Jl = J + (size_t)l * a.stride_c;
  float* __restrict__ xr = a.x + b * (size_t)n;
  const float lo = a.lo, hi = a.hi;
  for (int i = tid; i < nv; i += kDfThreads) {
    float jl[VEC], jc[VEC], x[VEC];
    ldv<VEC>(Jl, i, jl);
    ldv<VEC>(Jc, i, jc);
    ldv<VEC>(xr, i, x);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double w = (double)jl[e] - (double)jc[e];
      const float d = (NORM == 2) ? (float)(step * w) : (w > 0.0 ? stepf : (w < 0.0 ? -stepf : 0.0f));
      x[e] = clampf((d == 0.0f) ? x[e] : x[e] + d, lo, hi);  // (x + 0 would turn a -0 into +0)
    }
    stv<VEC>(xr, i, x);
  }
}

template <int NORM>
static void launch_deepfool(bool vec, int batch, const DeepfoolArgs& a, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((deepfool_step_kernel<4, NORM>), dim3((unsigned)batch), dim3(kDfThreads), 0, st, a);
  else hipLaunchKernelGGL((deepfool_step_kernel<1, NORM>), dim3((unsigned)batch), dim3(kDfThreads), 0, st, a);
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_deepfool_step(lipasr_handle_t h, const float* jac, long stride_b, long stride_c, const float* out, const int* label,
                         const uint32_t* allowed, int batch, int classes, int n, float norm, float overshoot, float clip_lo,
                         float clip_hi, float* x, float* dist, int* target, int* state, lipasr_stream_t stream) {
  LP_CHECK_ARG(norm == 2.0f || (norm > 0.0f && std::isinf(norm)), "lipasr_deepfool_step: norm %g; 2 or inf are supported", (double)norm);
  LP_CHECK_ARG(batch >= 0 && n >= 0, "lipasr_deepfool_step: bad shape %d x %d x %d", batch, classes, n);
  LP_CHECK_ARG(classes >= 1 && classes <= kDfMaxC, "lipasr_deepfool_step: %d classes; 1 to %d are supported", classes, kDfMaxC);
  LP_CHECK_ARG(stride_b >= 0 && stride_c >= 0, "lipasr_deepfool_step: negative stride (%ld, %ld)", stride_b, stride_c);
  LP_CHECK_ARG(overshoot >= 0.0f && overshoot < INFINITY, "lipasr_deepfool_step: overshoot %g", (double)overshoot);
  LP_CHECK_ARG(clip_lo <= clip_hi, "lipasr_deepfool_step: clip range [%g, %g]", (double)clip_lo, (double)clip_hi);
  LP_CHECK_ARG(h != nullptr, "lipasr_deepfool_step: null handle");
  if (batch == 0) return LIPASR_OK;
  LP_CHECK_ARG(out != nullptr && label != nullptr, "lipasr_deepfool_step: out or label is null");
  LP_CHECK_ARG(n == 0 || (jac != nullptr && x != nullptr), "lipasr_deepfool_step: jac or x is null");
  DeepfoolArgs a;
  a.jac = jac; a.stride_b = stride_b; a.stride_c = stride_c; a.out = out; a.label = label; a.allowed = allowed;
  a.C = classes; a.n = n; a.overshoot = overshoot; a.lo = clip_lo; a.hi = clip_hi;
  a.x = x; a.dist = dist; a.target = target; a.state = state;
  const bool vec = (n % 4 == 0) && (stride_b % 4 == 0) && (stride_c % 4 == 0) &&
                   ((reinterpret_cast<uintptr_t>(jac) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  hipStream_t st = S(stream);
  if (norm == 2.0f) launch_deepfool<2>(vec, batch, a, st);
  else launch_deepfool<0>(vec, batch, a, st);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // extern "C"
