// K3, the single-matrix projections: singular-value clipping (the FISTA surface), the Frobenius projection (customConstraint) and
// the BatchNorm correction factor.
#include "spectral.h"

namespace lipasr {

// ---------------------------------------------------------------------------------------------
// Singular-value clipping of an R x n matrix, R <= 32 (norm_constraint_FISTA, Constraints.py:78-91).
// X = U S V^T  =>  U min(S, hi) V^T = M X  with  M = U diag(min(s, hi) / s) U^T, and U, S^2 are the
// eigen-pairs of the R x R Gram matrix X X^T.  One workgroup: Gram in fp64 through an LDS tile,
// cyclic Jacobi with the round-robin (tournament) ordering so that R/2 disjoint rotations run at
// once, then M X column by column.  Fixed summation order; no atomics.
// ---------------------------------------------------------------------------------------------
constexpr int kSvTile = 256;
constexpr int kSvLd = kMaxR + 1;
constexpr int kSvMaxSweeps = 30;

__global__ __launch_bounds__(256) void sv_clip_kernel(const float* __restrict__ X, int R, int n, double hi,
                                                       float* out, float* __restrict__ svals_out) {
  __shared__ double G[kMaxR * kSvLd];
  __shared__ double V[kMaxR * kSvLd];
  __shared__ double cs[kMaxR];  // (c, s) per pair
  __shared__ int pq[kMaxR];     // (p, q) per pair, p < q; -1 when the pair holds the bye
  __shared__ double red[kMaxR + 1];
  __shared__ float tile[kMaxR * (kSvTile + 1)];
  const int tid = threadIdx.x;
  const int RR = R * R;
  // ---- Gram
  double acc[(kMaxR * kMaxR) / 256] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < n; j0 += kSvTile) {
    __syncthreads();
    for (int r = 0; r < R; ++r) tile[r * (kSvTile + 1) + tid] = (j0 + tid < n) ? X[(size_t)r * n + j0 + tid] : 0.0f;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < (kMaxR * kMaxR) / 256; ++u) {
      const int e = tid + 256 * u;
      if (e < RR) {
        const int a = e / R, b = e - a * R;
        const float* ta = tile + a * (kSvTile + 1);
        const float* tb = tile + b * (kSvTile + 1);
        double s = 0.0;
        for (int c = 0; c < kSvTile; ++c) s = fma((double)ta[c], (double)tb[c], s);
        acc[u] += s;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < (kMaxR * kMaxR) / 256; ++u) {
    const int e = tid + 256 * u;
    if (e < RR) {
      const int a = e / R, b = e - a * R;
      G[a * kSvLd + b] = acc[u];
      V[a * kSvLd + b] = (a == b) ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  // ---- Jacobi: G <- J^T G J, V <- V J
  const int Re = (R + 1) & ~1;  // players in the tournament (one bye when R is odd)
  const int n_pairs = Re / 2;
  for (int sweep = 0; sweep < kSvMaxSweeps; ++sweep) {
    // convergence: sum of squared off-diagonal entries against the squared diagonal
    if (tid < R) {
      double o = 0.0;
      for (int j = 0; j < R; ++j)
        if (j != tid) o = fma(G[tid * kSvLd + j], G[tid * kSvLd + j], o);
      red[tid] = o;
    }
    __syncthreads();
    double off = 0.0, dg = 0.0;
    for (int i = 0; i < R; ++i) {
      off += red[i];
      dg = fma(G[i * kSvLd + i], G[i * kSvLd + i], dg);
    }
    __syncthreads();
    if (!(off > 1e-30 * dg)) break;  // identical in every thread
    for (int round = 0; round < Re - 1; ++round) {
      if (tid < n_pairs) {
        int p, q;
        if (tid == 0) {
          p = Re - 1;
          q = round;
        } else {
          p = (round + tid) % (Re - 1);
          q = (round - tid + (Re - 1)) % (Re - 1);
        }
        if (p > q) { const int t = p; p = q; q = t; }
        double c = 1.0, sn = 0.0;
        if (q >= R) {
          p = -1;
        } else {
          const double gpp = G[p * kSvLd + p], gqq = G[q * kSvLd + q], gpq = G[p * kSvLd + q];
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
      // columns p, q of G and of V
      for (int e = tid; e < n_pairs * R; e += 256) {
        const int k = e / R, i = e - k * R;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        if (p < 0) continue;
        const double c = cs[2 * k], sn = cs[2 * k + 1];
        const double gip = G[i * kSvLd + p], giq = G[i * kSvLd + q];
        G[i * kSvLd + p] = c * gip - sn * giq;
        G[i * kSvLd + q] = sn * gip + c * giq;
        const double vip = V[i * kSvLd + p], viq = V[i * kSvLd + q];
        V[i * kSvLd + p] = c * vip - sn * viq;
        V[i * kSvLd + q] = sn * vip + c * viq;
      }
      __syncthreads();
      // rows p, q of G
      for (int e = tid; e < n_pairs * R; e += 256) {
        const int k = e / R, j = e - k * R;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        if (p < 0) continue;
        const double c = cs[2 * k], sn = cs[2 * k + 1];
        const double gpj = G[p * kSvLd + j], gqj = G[q * kSvLd + j];
        G[p * kSvLd + j] = c * gpj - sn * gqj;
        G[q * kSvLd + j] = sn * gpj + c * gqj;
      }
      __syncthreads();
    }
  }
  // ---- singular values (descending) and the clipping factors
  if (tid < R) {
    const double lam = G[tid * kSvLd + tid];
    const double sv = (lam > 0.0) ? sqrt(lam) : 0.0;
    red[tid] = sv;
    cs[tid] = (sv > hi) ? hi / sv : 1.0;
  }
  __syncthreads();
  if (svals_out && tid < R) {
    const double mine = red[tid];
    int rank = 0;
    for (int k = 0; k < R; ++k) rank += (red[k] > mine || (red[k] == mine && k < tid)) ? 1 : 0;
    svals_out[rank] = (float)mine;
  }
  if (!out) return;
  // M = V diag(f) V^T, kept in G
  double mloc[(kMaxR * kMaxR) / 256];
#pragma unroll
  for (int u = 0; u < (kMaxR * kMaxR) / 256; ++u) {
    const int e = tid + 256 * u;
    mloc[u] = 0.0;
    if (e < RR) {
      const int a = e / R, b = e - a * R;
      double s = 0.0;
      for (int k = 0; k < R; ++k) s = fma(cs[k] * V[a * kSvLd + k], V[b * kSvLd + k], s);
      mloc[u] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < (kMaxR * kMaxR) / 256; ++u) {
    const int e = tid + 256 * u;
    if (e < RR) G[(e / R) * kSvLd + (e % R)] = mloc[u];
  }
  __syncthreads();
  // ---- out = M X, one column per thread (in place allowed: a tile is read before it is written)
  for (int j0 = 0; j0 < n; j0 += kSvTile) {
    const int j = j0 + tid;
    if (j < n) {
      float xcol[kMaxR];
#pragma unroll
      for (int b = 0; b < kMaxR; ++b) xcol[b] = (b < R) ? X[(size_t)b * n + j] : 0.0f;
      for (int a = 0; a < R; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < kMaxR; ++b)
          if (b < R) s = fma(G[a * kSvLd + b], (double)xcol[b], s);
        out[(size_t)a * n + j] = (float)s;
      }
    }
  }
}

int launch_sv_clip(const float* X, int R, int n, double hi, float* out, float* svals_out, hipStream_t st) {
  hipLaunchKernelGGL(sv_clip_kernel, dim3(1), dim3(256), 0, st, X, R, n, hi, out, svals_out);
  k3_count(K3_SV_CLIP);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

// ---------------------------------------------------------------------------------------------
// Frobenius projection (customConstraint) and BN correction factor
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumsq_clamped_kernel(const float* __restrict__ w, size_t n, double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float x = fmaxf(w[i], 0.0f);
    s += (double)x * (double)x;
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void frob_scale_kernel(float* __restrict__ w, size_t n, const double* __restrict__ part,
                                                          int n_part, double rho) {
  __shared__ double tot;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int p = 0; p < n_part; ++p) s += part[p];
    tot = s;
  }
  __syncthreads();
  const float f = (float)(rho / (sqrt(tot) + kEps));
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) w[i] = fmaxf(w[i], 0.0f) * f;
}

int launch_frobenius(lipasr_ctx* h, float* W, size_t n, double rho, hipStream_t st) {
  const int nb = 256;
  double* part = carve_frobenius_partials(h, nb);
  if (!part) return LIPASR_EUNSUPPORTED;
  hipLaunchKernelGGL(sumsq_clamped_kernel, dim3(nb), dim3(256), 0, st, W, n, part);
  LP_LAUNCH_CHECK();
  hipLaunchKernelGGL(frob_scale_kernel, dim3(nb), dim3(256), 0, st, W, n, part, nb, rho);
  k3_count(K3_FROBENIUS);  // the pair counts once
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

__global__ __launch_bounds__(256) void bn_correction_kernel(const float* __restrict__ gamma, const float* __restrict__ var,
                                                             int n, float* __restrict__ out) {
  __shared__ float red[4];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, sqrtf(var[i]) / gamma[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *out = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

int launch_bn_correction(const float* gamma, const float* var, int n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(bn_correction_kernel, dim3(1), dim3(256), 0, st, gamma, var, n, out);
  k3_count(K3_BN_CORRECTION);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr
