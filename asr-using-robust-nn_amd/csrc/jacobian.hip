// Local Lipschitz read-out: the spectral norm of a stack of class gradients.  J_b is the C x n Jacobian of one sample (C <= 32
// classes, n = 880 / 2 020 features or 16 000 / 22 050 samples), jac[b * stride_b + c * stride_c + k]; sigma_b = ||J_b||_2, u_b and
// v_b its left and right singular vectors (include/lipasr.h, lipasr_jacobian_sigma, fixes the conventions).
//
// jacobian_sigma_kernel<RB, MULTI, VEC>: ONE workgroup of 256 threads per sample, one launch per call, in four steps.
//   max     max |J| and "is anything not finite", lane-serial then a wave maximum then the four waves through LDS.  A sample with a
//           NaN or inf ends here (sigma = NaN); an all-zero one too (sigma = 0, u = v = 0).  Everything after works on
//           J 2^ex with ex chosen so that the largest entry lies in [1, 2): the Jacobian of a saturated softmax is ~1e-30, its
//           squares are not fp32 numbers.  ldexpf is exact, so J 2^k gives sigma 2^k and the same u, v.
//   Gram    G = J J^T, C (C + 1) / 2 numbers.  A lane holds the C values of column k (VEC = 4: of four adjacent columns, one
//           16-byte load per row) and does the products in registers, so a row is read once and consecutive lanes read consecutive
//           addresses.  The accumulators are fp32 and lane-serial (n / 256 <= 87 terms each), then widened: wave_sum_d, then the four
//           waves in a fixed order through LDS -- as the project's other norms are summed; no atomics, the same bits on every run.
//           RB is the row block held in registers, 12 or 20: RB >= C is the single pass (C = 10: 78 accumulators, C = 20: 210).
//           C > 20 would need 528, more than a lane has, and takes RB = 12 over block pairs (MULTI: rows re-read from L2, 3.4 x at
//           C = 32; no model of the project has more than 20 classes).
//   eigen   cyclic Jacobi on G in fp64 in LDS, round-robin (tournament) ordering so that C / 2 disjoint rotations run at once -- the
//           scheme of sv_clip_kernel (spectral_clip.hip), restated here because that one is written into its kernel's LDS carving.
//           lambda_max -> sigma = sqrt(lambda_max) 2^-ex, its eigenvector -> u (largest component positive).
//   v       only when asked: v[k] = (sum_c u[c] J[c][k]) / sigma on the scaled values, a third read.  A column of zeros gives
//           fmaf(u, 0, +0) = +0 whatever u is: v stays exactly zero past the end of a ragged clip.
// The kernel reads J up to three times (the second and third mostly from L2: a sample is 35 KB to 1.8 MB) and does <= 528 FMAs per
// column, so the arithmetic is not what it waits for.  Measured ("Local Lipschitz read-out"): 256 samples of 10 x 880, 9 MB,
// take 107 us -- far from the read's cost: with one workgroup per sample the time is the latency of three dependent passes and of
// the barriers of the Jacobi sweeps.  VEC = 4 needs n, both strides and the bases multiples of 16 bytes; anything else takes VEC = 1.
#include "common.h"
#include "row.h"

namespace lipasr {

constexpr int kJacMaxC = 32;
constexpr int kJacLd = kJacMaxC + 1;
constexpr int kJacThreads = 256;
constexpr int kJacWaves = kJacThreads / 64;
constexpr int kJacMaxSweeps = 30;

struct JacSigmaArgs {
  const float* jac;
  int C, n;
  long stride_b, stride_c;
  float* sigma;  // [batch]
  float* u;      // [batch][C] or null
  float* v;      // [batch][n] or null
};

// rows [a0, a0 + RB) against rows [b0, b0 + RB) (DIAG: the same rows, upper triangle) of J 2^ex; rows >= C count as zero and are
// not read.  Wave w leaves its sums in part[w][a][b].
template <int RB, bool DIAG, int VEC>
__device__ __forceinline__ void gram_block(const float* __restrict__ J, long stride_c, int n, int C, int ex, int a0, int b0,
                                           double* __restrict__ part) {
  constexpr int NP = DIAG ? RB * (RB + 1) / 2 : RB * RB;
  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0f;
  const int nv = n / VEC;
  for (int i = threadIdx.x; i < nv; i += kJacThreads) {
    float xa[RB][VEC], xb[DIAG ? 1 : RB][VEC];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (a0 + r < C) {  // uniform
        ldv<VEC>(J + (size_t)(a0 + r) * stride_c, i, xa[r]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) xa[r][e] = ldexpf(xa[r][e], ex);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) xa[r][e] = 0.0f;
      }
    }
    if constexpr (!DIAG) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        if (b0 + r < C) {
          ldv<VEC>(J + (size_t)(b0 + r) * stride_c, i, xb[r]);
#pragma unroll
          for (int e = 0; e < VEC; ++e) xb[r][e] = ldexpf(xb[r][e], ex);
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) xb[r][e] = 0.0f;
        }
      }
    }
    int p = 0;
#pragma unroll
    for (int a = 0; a < RB; ++a)
#pragma unroll
      for (int b = DIAG ? a : 0; b < RB; ++b) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[p] = fmaf(xa[a][e], DIAG ? xa[b][e] : xb[b][e], acc[p]);
        ++p;
      }
  }
  const int lane = threadIdx.x & 63;
  double* mine = part + (threadIdx.x >> 6) * (kJacMaxC * kJacLd);
  int p = 0;
#pragma unroll
  for (int a = 0; a < RB; ++a)
#pragma unroll
    for (int b = DIAG ? a : 0; b < RB; ++b) {
      const double d = wave_sum_d((double)acc[p]);
      if (lane == 0 && a0 + a < C && b0 + b < C) mine[(a0 + a) * kJacLd + b0 + b] = d;
      ++p;
    }
}

template <int RB, bool MULTI, int VEC>
__global__ __launch_bounds__(kJacThreads) void jacobian_sigma_kernel(JacSigmaArgs a) {
  __shared__ double part[kJacWaves * kJacMaxC * kJacLd];
  __shared__ double G[kJacMaxC * kJacLd];
  __shared__ double V[kJacMaxC * kJacLd];
  __shared__ double cs[kJacMaxC];  // (c, s) per pair
  __shared__ int pq[kJacMaxC];     // (p, q) per pair, p < q; -1 when the pair holds the bye
  __shared__ double red[kJacMaxC];
  __shared__ float wmax[kJacWaves];
  __shared__ int wbad[kJacWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, n = a.n, nv = n / VEC;
  const size_t b = blockIdx.x;
  const float* __restrict__ J = a.jac + b * (size_t)a.stride_b;
  float* __restrict__ vout = a.v ? a.v + b * (size_t)n : nullptr;

  // ---- max |J|, and whether every entry is finite
  float mx = 0.0f;
  int bad = 0;
  for (int c = 0; c < C; ++c) {
    const float* row = J + (size_t)c * a.stride_c;
    for (int i = tid; i < nv; i += kJacThreads) {
      float x[VEC];
      ldv<VEC>(row, i, x);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float m = fabsf(x[e]);
        bad |= !(m < INFINITY);  // inf or NaN
        mx = fmaxf(mx, m);
      }
    }
  }
  mx = wave_max(mx);
  bad = __any(bad);
  if (lane == 0) { wmax[wave] = mx; wbad[wave] = bad; }
  __syncthreads();
  mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  bad = wbad[0] | wbad[1] | wbad[2] | wbad[3];
  if (bad || mx == 0.0f) {  // the same in every thread
    if (tid == 0) a.sigma[b] = bad ? NAN : 0.0f;
    if (a.u && tid < C) a.u[b * C + tid] = 0.0f;
    if (vout)
      for (int k = tid; k < n; k += kJacThreads) vout[k] = 0.0f;
    return;
  }
  int ex = 0;
  (void)frexpf(mx, &ex);  // mx = f 2^ex, f in [0.5, 1)
  ex = 1 - ex;            // mx 2^ex in [1, 2)

  // ---- Gram matrix of the scaled rows
  if constexpr (MULTI) {
    for (int a0 = 0; a0 < C; a0 += RB) {
      gram_block<RB, true, VEC>(J, a.stride_c, n, C, ex, a0, a0, part);
      for (int b0 = a0 + RB; b0 < C; b0 += RB) gram_block<RB, false, VEC>(J, a.stride_c, n, C, ex, a0, b0, part);
    }
  } else {
    gram_block<RB, true, VEC>(J, a.stride_c, n, C, ex, 0, 0, part);
  }
  __syncthreads();
  for (int e = tid; e < C * C; e += kJacThreads) {
    const int i = e / C, j = e - i * C;
    const int lo = (i < j ? i : j) * kJacLd + (i < j ? j : i);
    constexpr int W = kJacMaxC * kJacLd;
    G[i * kJacLd + j] = ((part[lo] + part[W + lo]) + part[2 * W + lo]) + part[3 * W + lo];
    V[i * kJacLd + j] = (i == j) ? 1.0 : 0.0;
  }
  __syncthreads();

  // ---- Jacobi: G <- R^T G R, V <- V R
  const int Ce = (C + 1) & ~1;  // players in the tournament (one bye when C is odd)
  const int n_pairs = Ce / 2;
  for (int sweep = 0; sweep < kJacMaxSweeps; ++sweep) {
    if (tid < C) {
      double o = 0.0;
      for (int j = 0; j < C; ++j)
        if (j != tid) o = fma(G[tid * kJacLd + j], G[tid * kJacLd + j], o);
      red[tid] = o;
    }
    __syncthreads();
    double off = 0.0, dg = 0.0;
    for (int i = 0; i < C; ++i) {
      off += red[i];
      dg = fma(G[i * kJacLd + i], G[i * kJacLd + i], dg);
    }
    __syncthreads();
    if (!(off > 1e-30 * dg)) break;  // identical in every thread
    for (int round = 0; round < Ce - 1; ++round) {
      if (tid < n_pairs) {
        int p, q;
        if (tid == 0) {
          p = Ce - 1;
          q = round;
        } else {
          p = (round + tid) % (Ce - 1);
          q = (round - tid + (Ce - 1)) % (Ce - 1);
        }
        if (p > q) { const int t = p; p = q; q = t; }
        double c = 1.0, sn = 0.0;
        if (q >= C) {
          p = -1;
        } else {
          const double gpp = G[p * kJacLd + p], gqq = G[q * kJacLd + q], gpq = G[p * kJacLd + q];
          if (fabs(gpq) > 1e-300 && fabs(gpq) > 1e-18 * sqrt(fabs(gpp * gqq))) {
            const double tau = (gqq - gpp) / (2.0 * gpq);
            const double t = ((tau >= 0.0) ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            sn = t * c;
          }
        }
        pq[2 * tid] = p;
        pq[2 * tid + 1] = q;
        cs[2 * tid] = c;
        cs[2 * tid + 1] = sn;
      }
      __syncthreads();
      for (int e = tid; e < n_pairs * C; e += kJacThreads) {  // columns p, q of G and of V
        const int k = e / C, i = e - k * C;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        if (p < 0) continue;
        const double c = cs[2 * k], sn = cs[2 * k + 1];
        const double gip = G[i * kJacLd + p], giq = G[i * kJacLd + q];
        G[i * kJacLd + p] = c * gip - sn * giq;
        G[i * kJacLd + q] = sn * gip + c * giq;
        const double vip = V[i * kJacLd + p], viq = V[i * kJacLd + q];
        V[i * kJacLd + p] = c * vip - sn * viq;
        V[i * kJacLd + q] = sn * vip + c * viq;
      }
      __syncthreads();
      for (int e = tid; e < n_pairs * C; e += kJacThreads) {  // rows p, q of G
        const int k = e / C, j = e - k * C;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        if (p < 0) continue;
        const double c = cs[2 * k], sn = cs[2 * k + 1];
        const double gpj = G[p * kJacLd + j], gqj = G[q * kJacLd + j];
        G[p * kJacLd + j] = c * gpj - sn * gqj;
        G[q * kJacLd + j] = sn * gpj + c * gqj;
      }
      __syncthreads();
    }
  }

  // ---- the largest eigenvalue (lowest index on a tie) and its vector, every thread for itself from LDS
  int km = 0;
  double lam = G[0];
  for (int i = 1; i < C; ++i)
    if (G[i * kJacLd + i] > lam) { lam = G[i * kJacLd + i]; km = i; }
  const double sig = sqrt(lam > 0.0 ? lam : 0.0);  // of the scaled matrix: >= 1, its largest entry is
  int im = 0;
  double um = fabs(V[km]);
  for (int i = 1; i < C; ++i)
    if (fabs(V[i * kJacLd + km]) > um) { um = fabs(V[i * kJacLd + km]); im = i; }
  const double sgn = V[im * kJacLd + km] < 0.0 ? -1.0 : 1.0;
  if (tid == 0) a.sigma[b] = (float)ldexp(sig, -ex);
  if (a.u && tid < C) a.u[b * C + tid] = (float)(sgn * V[tid * kJacLd + km]);
  if (!vout) return;

  // ---- v = J^T u / sigma
  float* uf = reinterpret_cast<float*>(part);  // (the partials were consumed before the Jacobi sweeps)
  if (tid < C) uf[tid] = (float)(sgn * V[tid * kJacLd + km]);
  __syncthreads();
  const float sigf = (float)sig;
  for (int i = tid; i < nv; i += kJacThreads) {
    float s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.0f;
    for (int c = 0; c < C; ++c) {
      float x[VEC];
      ldv<VEC>(J + (size_t)c * a.stride_c, i, x);
      const float uc = uf[c];
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] = fmaf(uc, ldexpf(x[e], ex), s[e]);
    }
    if constexpr (VEC == 4) {
      reinterpret_cast<float4*>(vout)[i] = make_float4(s[0] / sigf, s[1] / sigf, s[2] / sigf, s[3] / sigf);
    } else {
      vout[i] = s[0] / sigf;
    }
  }
}

template <int RB, bool MULTI>
static void launch_jac(bool vec, int batch, const JacSigmaArgs& a, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((jacobian_sigma_kernel<RB, MULTI, 4>), dim3((unsigned)batch), dim3(kJacThreads), 0, st, a);
  else hipLaunchKernelGGL((jacobian_sigma_kernel<RB, MULTI, 1>), dim3((unsigned)batch), dim3(kJacThreads), 0, st, a);
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_jacobian_sigma(lipasr_handle_t h, const float* jac, int batch, int classes, int n, long stride_b, long stride_c,
                          float* sigma, float* u, float* v, lipasr_stream_t stream) {
  LP_CHECK_ARG(h != nullptr, "lipasr_jacobian_sigma: null handle");
  LP_CHECK_ARG(batch >= 0 && n >= 0, "lipasr_jacobian_sigma: bad shape %d x %d x %d", batch, classes, n);
  LP_CHECK_ARG(classes >= 1 && classes <= kJacMaxC, "lipasr_jacobian_sigma: %d classes; 1 to %d are supported", classes, kJacMaxC);
  LP_CHECK_ARG(stride_b >= 0 && stride_c >= 0, "lipasr_jacobian_sigma: negative stride (%ld, %ld)", stride_b, stride_c);
  if (batch == 0) return LIPASR_OK;
  LP_CHECK_ARG(sigma != nullptr, "lipasr_jacobian_sigma: sigma is null");
  hipStream_t st = S(stream);
  if (n == 0) {  // an empty Jacobian: sigma = 0, u = 0
    LP_HIP(hipMemsetAsync(sigma, 0, (size_t)batch * sizeof(float), st));
    if (u) LP_HIP(hipMemsetAsync(u, 0, (size_t)batch * classes * sizeof(float), st));
    return LIPASR_OK;
  }
  LP_CHECK_ARG(jac != nullptr, "lipasr_jacobian_sigma: jac is null");
  JacSigmaArgs a;
  a.jac = jac; a.C = classes; a.n = n; a.stride_b = stride_b; a.stride_c = stride_c; a.sigma = sigma; a.u = u; a.v = v;
  const bool vec = (n % 4 == 0) && (stride_b % 4 == 0) && (stride_c % 4 == 0) &&
                   ((reinterpret_cast<uintptr_t>(jac) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  if (classes <= 12) launch_jac<12, false>(vec, batch, a, st);       // 10: the digits
  else if (classes <= 20) launch_jac<20, false>(vec, batch, a, st);  // 20: the speakers
  else launch_jac<12, true>(vec, batch, a, st);                      // block pairs
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // extern "C"
