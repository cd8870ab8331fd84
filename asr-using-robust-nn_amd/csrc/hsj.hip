// HopSkipJump (Chen, Jordan, Wainwright 2020), the decision-based minimum-norm attack: the four kernels around the classifier, and
// their host restatements.  (include/lipasr.h, lipasr_hsj_expand / _accumulate / _direction / _search, fixes the conventions.)
//
// hsj_expand_kernel<NQ, T>: ONE workgroup of T threads per output row b * draws + j.  A thread owns the quads q = tid, tid + T, ...
//   of the row; quad q of draw j is one Philox block.  The draw is generated once, held in NQ x 4 registers per thread while its
//   squared length is added up (L-inf: 64-bit integers, exact and order-free; L2: fp64, lane-serial, butterfly, one double per
//   wavefront in LDS), and written as clamp(fmaf(delta / ||r||, r, x)).  T = 256 with NQ = 1, 2, 4, 8: n <= 1 024 (880), 2 048
//   (2 020), 4 096, 8 192; T = 1 024 with NQ = 4, 6: n <= 16 384 (16 000), 24 576 (22 050) -- over audio there are few rows, so a
//   row is spread over 16 wavefronts, and the unrolled body stays short; NQ = 0 (T = 256), anything wider, generates the draw a
//   second time.  hsj_expand_instance() is the one selector.  The loops over a thread's quads are unrolled in full, so the draw
//   is indexed by constants only and no instance uses scratch memory.
// hsj_accumulate_kernel: 64 threads, grid (quads / 64, batch).  phi_j of the row's draws into LDS (one byte each), then a thread
//   walks j = 0 .. draws - 1 over its own element quad and adds (p_j - x) and phi_j (p_j - x) in fp64 to the workspace: ascending
//   j, carried through memory, so chunks of draws give the bits of one call.
// hsj_direction_kernel: ONE workgroup per row: g from the two sums and the two counts, u = sign(g) or g / ||g||_2 (fp64).
// hsj_search_kernel: ONE workgroup per row, one launch per query: the row's scalars (8 floats, 8 ints) are read by every thread,
//   hsj_decide() -- shared with the host twin -- says what moves, and the threads move it quad by quad.
//   The quads move as row.h says; `vec` is its `whole`: n a multiple of 4 and every base of the call on 16 bytes.
//   No atomics, nothing waits on another workgroup, two runs give the same bits.  Every a * b + c that a comparison of bits depends
//   on is an explicit fmaf / fma, and contraction is off for the whole file, so host and device round alike.
#include "common.h"
#include "row.h"

#pragma clang fp contract(off)

namespace lipasr {

constexpr int kHsjThreads = 256;
constexpr int kHsjWideThreads = 1024, kHsjWide = 32;  // expand over rows of more than 8 192 elements
constexpr int kHsjMaxC = 32;
constexpr int kHsjAccThreads = 64;
constexpr int kHsjMaxDraws = 16384;  // phi in LDS, one byte per draw
constexpr uint32_t kHsjTagStart = 1u << 28, kHsjTagL2 = 2u << 28, kHsjTagLinf = 3u << 28;

__host__ __device__ __forceinline__ bool hsj_finite(float v) { return fabsf(v) < INFINITY; }

// argmax != y (targeted: == y), the lowest index on a tie; a NaN anywhere or a label outside [0, classes): not adversarial
__host__ __device__ __forceinline__ bool hsj_adv(const float* __restrict__ z, int classes, int y, int targeted) {
  if (y < 0 || y >= classes) return false;
  float m = -INFINITY;
  int p = 0;
  bool nan = false;
  for (int c = 0; c < classes; ++c) {
    const float v = z[c];
    nan |= v != v;
    if (v > m) { m = v; p = c; }
  }
  if (nan) return false;
  return targeted ? p == y : p != y;
}

// quad q of draw `draw` of iteration `it` of clip `clip`: four elements of r (before scaling)
__host__ __device__ __forceinline__ void hsj_draw4(int l2, uint64_t seed, uint32_t clip, uint32_t it, uint32_t draw, int q, float (&r)[4]) {
  const uint64_t ctr = (uint64_t)(uint32_t)q | ((uint64_t)draw << 32);
  if (l2) {
    normal4(seed, ctr, clip, kHsjTagL2 | it, r);
  } else {
    uint32_t o[4];
    Philox::gen(seed, ctr, clip, kHsjTagLinf | it, o);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)((int)(o[e] >> 8) + 1 - (1 << 23)) * (1.0f / 8388608.0f);  // (k - 2^23) / 2^23, exact
  }
}
__host__ __device__ __forceinline__ uint64_t hsj_sq_int(float r) {  // (r 2^23)^2 as an integer, exact
  const long long m = (long long)(r * 8388608.0f);
  return (uint64_t)(m * m);
}
// delta / ||r||_2 in fp32, rounded once from fp64; 0 where the draw is empty or delta is not finite
__host__ __device__ __forceinline__ float hsj_scale(int l2, double ss, uint64_t si, float delta) {
  const double nrm = l2 ? sqrt(ss) : sqrt((double)si) * (1.0 / 8388608.0);
  if (!(nrm > 0.0) || !(nrm < (double)INFINITY) || !hsj_finite(delta)) return 0.0f;
  return (float)((double)delta / nrm);
}
__host__ __device__ __forceinline__ float hsj_point(float s, float r, float x, float lo, float hi) { return clampf(fmaf(s, r, x), lo, hi); }

// the start draws: uniform in [sl, sh]
__host__ __device__ __forceinline__ void hsj_start4(uint64_t seed, uint32_t clip, uint32_t draw, int q, float (&u)[4]) {
  uint32_t o[4];
  Philox::gen(seed, (uint64_t)(uint32_t)q | ((uint64_t)draw << 32), clip, kHsjTagStart, o);
#pragma unroll
  for (int e = 0; e < 4; ++e) u[e] = Philox::u01(o[e]);
}
__host__ __device__ __forceinline__ float hsj_start_value(float u, float sl, float sh) { return clampf(fmaf(u, sh - sl, sl), sl, sh); }

// the two projections of the bisection: the blend (L2) and the box (L-inf) between x0 and the far point
__host__ __device__ __forceinline__ float hsj_proj(int l2, float a, float x0, float xf, float lo, float hi) {
  float v;
  if (l2) {
    v = fmaf(a, xf, fmaf(-a, x0, x0));
  } else {
    const float l = x0 - a, h = x0 + a;
    v = xf < l ? l : (xf > h ? h : xf);
  }
  return clampf(v, lo, hi);
}

// g_k from the two sums: sum_j (phi_j - m)(p_j - x) = s1 - m s0
__host__ __device__ __forceinline__ double hsj_g(double s0, double s1, int total, int pos) {
  if (total <= 0) return 0.0;
  if (pos >= total) return s0;
  if (pos <= 0) return -s0;
  const double m = (double)(2 * (long long)pos - total) / (double)total;
  return fma(-m, s0, s1);
}
__host__ __device__ __forceinline__ float hsj_sign(double g) { return g > 0.0 ? 1.0f : (g < 0.0 ? -1.0f : 0.0f); }
__host__ __device__ __forceinline__ float hsj_unit(double g, double nrm) {
  return (nrm > 0.0 && nrm < (double)INFINITY && g == g) ? (float)(g / nrm) : 0.0f;
}

// ---- the search: a row's scalars and what one call decides for it
struct HsjRow {
  float lo, hi, mid, thresh, eps, dist, dist_best, dist_far;
  int active, found, ok, moved, halvings, queries, spare0, spare1;
};
struct HsjOps {
  int init_rows;      // x_adv, x_best <- x0
  int far_from_cand;  // x_far <- x_cand
  int cand;           // 0: keep, 1: start draw `draw`, 2: clamp(x_adv + eps u), 3: proj(mid), 4: x0
  int finish;         // x_adv <- proj(hi) (or x_far), dist, x_best
  uint32_t draw;
};

__host__ __device__ __forceinline__ void hsj_load_row(const float* __restrict__ f, const int* __restrict__ i, HsjRow& r) {
  r.lo = f[0]; r.hi = f[1]; r.mid = f[2]; r.thresh = f[3]; r.eps = f[4]; r.dist = f[5]; r.dist_best = f[6]; r.dist_far = f[7];
  r.active = i[0]; r.found = i[1]; r.ok = i[2]; r.moved = i[3]; r.halvings = i[4]; r.queries = i[5]; r.spare0 = i[6]; r.spare1 = i[7];
}
__host__ __device__ __forceinline__ void hsj_store_row(float* __restrict__ f, int* __restrict__ i, const HsjRow& r) {
  f[0] = r.lo; f[1] = r.hi; f[2] = r.mid; f[3] = r.thresh; f[4] = r.eps; f[5] = r.dist; f[6] = r.dist_best; f[7] = r.dist_far;
  i[0] = r.active; i[1] = r.found; i[2] = r.ok; i[3] = r.moved; i[4] = r.halvings; i[5] = r.queries; i[6] = r.spare0; i[7] = r.spare1;
}

// does BISECT | FIRST need ||x_far - x0||_inf of this row before it decides?
__host__ __device__ __forceinline__ bool hsj_needs_far(const HsjRow& r, int mode, int flags, int l2, int nv) {
  return mode == LIPASR_HSJ_BISECT && (flags & LIPASR_HSJ_FIRST) && !l2 && r.ok != 0 && nv > 0;
}

__host__ __device__ __forceinline__ HsjOps hsj_decide(HsjRow& r, int mode, int flags, bool adv, int nv, int l2, float theta,
                                                      float step_scale, int max_halvings, uint32_t draw, float dist_far) {
  HsjOps o = {0, 0, 0, 0, 0u};
  const bool first = (flags & LIPASR_HSJ_FIRST) != 0, last = (flags & LIPASR_HSJ_LAST) != 0;
  if (mode == LIPASR_HSJ_START) {
    if (first) {
      const int act = r.active != 0 && nv > 0;
      r.lo = r.hi = r.mid = r.thresh = r.eps = 0.0f;
      r.dist = r.dist_best = r.dist_far = INFINITY;
      r.active = act;
      r.found = r.ok = r.moved = r.halvings = r.queries = r.spare0 = r.spare1 = 0;
      o.init_rows = 1;
      o.cand = act ? 1 : 4;
      o.draw = 0u;
    } else if (r.active) {
      ++r.queries;
      if (adv) { o.far_from_cand = 1; r.found = r.ok = 1; r.active = 0; }
      else if (last) r.active = 0;
      else { o.cand = 1; o.draw = draw + 1u; }
    }
  } else if (mode == LIPASR_HSJ_HALVE) {
    if (first) {
      r.active = r.found != 0 && nv > 0;
      r.ok = 0;
      r.halvings = 0;
      r.eps = r.dist * step_scale;
      if (r.active) o.cand = 2;
    } else if (r.active) {
      ++r.queries;
      if (adv) { o.far_from_cand = 1; r.ok = 1; r.active = 0; }
      else if (++r.halvings >= max_halvings) r.active = 0;
      else { r.eps = r.eps * 0.5f; o.cand = 2; }
    }
  } else {
    bool advance = false;
    if (first) {
      r.active = r.ok != 0 && nv > 0;
      r.moved = 0;
      if (r.active) {
        r.dist_far = dist_far;
        r.lo = 0.0f;
        r.hi = l2 ? 1.0f : dist_far;
        const float dt = dist_far * theta;
        r.thresh = l2 ? theta : (dt < theta ? dt : theta);
        advance = true;
      }
    } else if (r.active) {
      ++r.queries;
      if (adv) { r.hi = r.mid; r.moved = 1; } else { r.lo = r.mid; }
      advance = true;
    }
    if (advance) {
      const float mid = 0.5f * (r.lo + r.hi);
      if (!(r.hi - r.lo > r.thresh) || !(mid > r.lo && mid < r.hi)) { o.finish = 1; r.active = 0; }
      else { r.mid = mid; o.cand = 3; }
    }
  }
  return o;
}

// ---- device helpers: block_sum_d (row.h) for 64-bit integers and for a maximum
template <int T>
__device__ __forceinline__ uint64_t hsj_block_sum_u(uint64_t v, uint64_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64), lo = __shfl_xor((uint32_t)v, o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) v += red[w];
  __syncthreads();
  return v;
}
__device__ __forceinline__ float hsj_block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < kHsjThreads / 64; ++w) v = fmaxf(v, red[w]);
  __syncthreads();
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------- expand
struct HsjExpandArgs {
  const float* x; const float* delta; const int* n_valid; float* out;
  int batch, n, draws, l2, vec;
  uint32_t clip0, it, draw0;
  uint64_t seed;
  float lo, hi;
};

template <int NQ, int T>
__global__ __launch_bounds__(T) void hsj_expand_kernel(HsjExpandArgs a) {
  __shared__ double red_d[T / 64];
  __shared__ uint64_t red_u[T / 64];
  const int tid = threadIdx.x, n = a.n;
  const int b = (int)(blockIdx.x / (unsigned)a.draws), j = (int)(blockIdx.x % (unsigned)a.draws);
  const uint32_t clip = a.clip0 + (uint32_t)b, draw = a.draw0 + (uint32_t)j;
  const int nv = row_valid(a.n_valid, b, n);
  const int quads = (n + 3) >> 2;
  const bool vec = a.vec != 0;
  const float* __restrict__ xr = a.x + (size_t)b * n;
  float* __restrict__ outr = a.out + (size_t)blockIdx.x * n;
  constexpr int R = NQ > 0 ? NQ : 1;
  float D[R][4];
  auto gen = [&](int q, float (&r)[4]) {
    if (4 * q < nv) {
      hsj_draw4(a.l2, a.seed, clip, a.it, draw, q, r);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (4 * q + e < nv) ? r[e] : 0.0f;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = 0.0f;
    }
  };
  const int nj = NQ > 0 ? NQ : (quads + T - 1) / T;
  double ss = 0.0;
  uint64_t si = 0;
  // both loops over s are unrolled in full where NQ > 0: D is indexed by constants only and stays in registers
#pragma unroll(R)
  for (int s = 0; s < nj; ++s) {
    float r[4];
    gen(tid + T * s, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (a.l2) ss += (double)r[e] * (double)r[e]; else si += hsj_sq_int(r[e]);
      if constexpr (NQ > 0) D[s][e] = r[e];
    }
  }
  if (a.l2) ss = block_sum_d<T>(ss, red_d); else si = hsj_block_sum_u<T>(si, red_u);
  const float sc = hsj_scale(a.l2, ss, si, a.delta[b]);
#pragma unroll(R)
  for (int s = 0; s < nj; ++s) {
    const int q = tid + T * s;
    if (q >= quads) break;
    float r[4], xv[4], o[4];
    if constexpr (NQ > 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = D[s][e];
    } else {
      gen(q, r);
    }
    ld4(xr, 4 * q, n, vec, xv);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (4 * q + e < nv) ? hsj_point(sc, r[e], xv[e], a.lo, a.hi) : xv[e];
    st4(outr, 4 * q, n, vec, o);
  }
}

// quads per thread, | kHsjWide where the workgroup has kHsjWideThreads threads; 0: the draw is generated twice
static int hsj_expand_instance(int n) {
  const int per = 4 * kHsjThreads, wide = 4 * kHsjWideThreads;
  if (n <= per) return 1;
  if (n <= 2 * per) return 2;
  if (n <= 4 * per) return 4;
  if (n <= 8 * per) return 8;
  if (n <= 4 * wide) return 4 | kHsjWide;
  if (n <= 6 * wide) return 6 | kHsjWide;
  return 0;
}

// -------------------------------------------------------------------------------------------------------------------- accumulate
__global__ __launch_bounds__(kHsjAccThreads) void hsj_accumulate_kernel(const float* __restrict__ logits, const int* __restrict__ labels,
                                                                        const float* __restrict__ p, const float* __restrict__ x,
                                                                        const int* __restrict__ n_valid, int C, int n, int draws,
                                                                        int targeted, int vec_, double* __restrict__ sums,
                                                                        int* __restrict__ counts) {
  __shared__ unsigned char phi[kHsjMaxDraws];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int y = labels[b];
  const bool vec = vec_ != 0;
  int pos = 0;
  for (int j = tid; j < draws; j += kHsjAccThreads) {
    const bool adv = hsj_adv(logits + ((size_t)b * draws + j) * C, C, y, targeted);
    phi[j] = adv ? 1 : 0;
    pos += adv ? 1 : 0;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pos += __shfl_xor(pos, o, 64);
    if (tid == 0) {
      counts[(size_t)b * 2] += draws;
      counts[(size_t)b * 2 + 1] += pos;
    }
  }
  const int quads = (n + 3) >> 2;
  const int q = blockIdx.x * kHsjAccThreads + tid;
  if (q >= quads) return;
  const int k0 = 4 * q;
  const int nv = row_valid(n_valid, b, n);
  double* __restrict__ s0 = sums + ((size_t)b * 2) * n;
  double* __restrict__ s1 = s0 + n;
  float xv[4];
  ld4(x + (size_t)b * n, k0, n, vec, xv);
  double a0[4], a1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a0[e] = (k0 + e < n) ? s0[k0 + e] : 0.0;
    a1[e] = (k0 + e < n) ? s1[k0 + e] : 0.0;
  }
  const float* __restrict__ pr = p + (size_t)b * draws * n;
#pragma unroll 4
  for (int j = 0; j < draws; ++j) {
    float pv[4];
    ld4(pr + (size_t)j * n, k0, n, vec, pv);
    const bool plus = phi[j] != 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (k0 + e < nv) ? (double)pv[e] - (double)xv[e] : 0.0;
      a0[e] += d;
      a1[e] += plus ? d : -d;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (k0 + e < n) { s0[k0 + e] = a0[e]; s1[k0 + e] = a1[e]; }
}

// --------------------------------------------------------------------------------------------------------------------- direction
__global__ __launch_bounds__(kHsjThreads) void hsj_direction_kernel(const double* __restrict__ sums, const int* __restrict__ counts,
                                                                    const int* __restrict__ n_valid, int n, int l2, int vec_,
                                                                    float* __restrict__ u) {
  __shared__ double red[kHsjThreads / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const bool vec = vec_ != 0;
  const int nv = row_valid(n_valid, b, n);
  const int total = counts[(size_t)b * 2], pos = counts[(size_t)b * 2 + 1];
  const double* __restrict__ s0 = sums + ((size_t)b * 2) * n;
  const double* __restrict__ s1 = s0 + n;
  const int quads = (n + 3) >> 2;
  double nrm = 0.0;
  if (l2) {
    double ss = 0.0;
    for (int q = tid; q < quads; q += kHsjThreads)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 4 * q + e;
        if (k < nv) { const double g = hsj_g(s0[k], s1[k], total, pos); ss += g * g; }
      }
    nrm = sqrt(block_sum_d<kHsjThreads>(ss, red));
  }
  for (int q = tid; q < quads; q += kHsjThreads) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * q + e;
      o[e] = 0.0f;
      if (k < nv) { const double g = hsj_g(s0[k], s1[k], total, pos); o[e] = l2 ? hsj_unit(g, nrm) : hsj_sign(g); }
    }
    st4(u + (size_t)b * n, 4 * q, n, vec, o);
  }
}

// ------------------------------------------------------------------------------------------------------------------------ search
struct HsjSearchArgs {
  const float* logits; const int* labels; const float* x0; const int* n_valid; const float* u;
  const float* start_lo; const float* start_hi; const float* theta;
  float* x_cand; float* x_far; float* x_adv; float* x_best; float* fstate; int* istate;
  int batch, C, n, mode, flags, targeted, l2, max_halvings, vec;
  uint32_t clip0, draw;
  uint64_t seed;
  float step_scale, lo, hi;
};

__global__ __launch_bounds__(kHsjThreads) void hsj_search_kernel(HsjSearchArgs a) {
  __shared__ double red_d[kHsjThreads / 64];
  __shared__ float red_f[kHsjThreads / 64];
  const int tid = threadIdx.x, b = blockIdx.x, n = a.n;
  const bool vec = a.vec != 0;
  const int l2 = a.l2;
  const size_t base = (size_t)b * n;
  const int nv = row_valid(a.n_valid, b, n);
  const int quads = (n + 3) >> 2;
  HsjRow r;
  hsj_load_row(a.fstate + (size_t)b * 8, a.istate + (size_t)b * 8, r);
  const bool first = (a.flags & LIPASR_HSJ_FIRST) != 0;
  const bool adv = first ? false : hsj_adv(a.logits + (size_t)b * a.C, a.C, a.labels[b], a.targeted);
  const float* __restrict__ x0 = a.x0 + base;
  float dist_far = 0.0f;
  if (hsj_needs_far(r, a.mode, a.flags, l2, nv)) {  // uniform over the row
    float m = 0.0f;
    for (int q = tid; q < quads; q += kHsjThreads) {
      float c[4], f[4];
      ld4(x0, 4 * q, n, vec, c);
      ld4(a.x_far + base, 4 * q, n, vec, f);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < nv) m = fmaxf(m, fabsf(f[e] - c[e]));
    }
    dist_far = hsj_block_max(m, red_f);
  }
  const float theta = a.theta[b];
  const HsjOps op = hsj_decide(r, a.mode, a.flags, adv, nv, l2, theta, a.step_scale, a.max_halvings, a.draw, dist_far);
  __syncthreads();  // every thread has read the row's scalars
  const uint32_t clip = a.clip0 + (uint32_t)b;
  if (op.init_rows | op.far_from_cand | (op.cand != 0)) {
    const float sl = a.start_lo[b], sh = a.start_hi[b];
    for (int q = tid; q < quads; q += kHsjThreads) {
      const int k0 = 4 * q;
      float c[4];
      ld4(x0, k0, n, vec, c);
      if (op.init_rows) {
        st4(a.x_adv + base, k0, n, vec, c);
        st4(a.x_best + base, k0, n, vec, c);
      }
      if (op.far_from_cand) {
        float t[4];
        ld4(a.x_cand + base, k0, n, vec, t);
        st4(a.x_far + base, k0, n, vec, t);
      }
      float o[4];
      if (op.cand == 1) {
        float uu[4];
        hsj_start4(a.seed, clip, op.draw, q, uu);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (k0 + e < nv) ? hsj_start_value(uu[e], sl, sh) : c[e];
      } else if (op.cand == 2) {
        float xa[4], uu[4];
        ld4(a.x_adv + base, k0, n, vec, xa);
        ld4(a.u + base, k0, n, vec, uu);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (k0 + e < nv) ? hsj_point(r.eps, uu[e], xa[e], a.lo, a.hi) : c[e];
      } else if (op.cand == 3) {
        float f[4];
        ld4(a.x_far + base, k0, n, vec, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (k0 + e < nv) ? hsj_proj(l2, r.mid, c[e], f[e], a.lo, a.hi) : c[e];
      } else if (op.cand == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = c[e];
      }
      if (op.cand != 0) st4(a.x_cand + base, k0, n, vec, o);
    }
  }
  if (op.finish) {  // uniform over the row
    double ss = 0.0;
    float mx = 0.0f;
    auto value = [&](int k0, const float (&c)[4], float (&o)[4]) {
      float f[4];
      ld4(a.x_far + base, k0, n, vec, f);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (k0 + e < nv) ? (r.moved ? hsj_proj(l2, r.hi, c[e], f[e], a.lo, a.hi) : f[e]) : c[e];
    };
    for (int q = tid; q < quads; q += kHsjThreads) {
      const int k0 = 4 * q;
      float c[4], o[4];
      ld4(x0, k0, n, vec, c);
      value(k0, c, o);
      st4(a.x_adv + base, k0, n, vec, o);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k0 + e < nv) {
          if (l2) { const double d = (double)o[e] - (double)c[e]; ss += d * d; }
          else mx = fmaxf(mx, fabsf(o[e] - c[e]));
        }
    }
    r.dist = l2 ? (float)sqrt(block_sum_d<kHsjThreads>(ss, red_d)) : hsj_block_max(mx, red_f);
    if (r.dist < r.dist_best) {
      r.dist_best = r.dist;
      for (int q = tid; q < quads; q += kHsjThreads) {
        const int k0 = 4 * q;
        float c[4], o[4];
        ld4(x0, k0, n, vec, c);
        value(k0, c, o);
        st4(a.x_best + base, k0, n, vec, o);
      }
    }
  }
  if (tid == 0) hsj_store_row(a.fstate + (size_t)b * 8, a.istate + (size_t)b * 8, r);
}

// ------------------------------------------------------------------------------------------------------------------------ checks
static int hsj_norm(const char* fn, float norm, int* l2) {
  LP_CHECK_ARG(norm == 2.0f || (std::isinf(norm) && norm > 0.0f), "%s: norm=%g; 2 and inf are supported", fn, (double)norm);
  *l2 = norm == 2.0f ? 1 : 0;
  return LIPASR_OK;
}

static int hsj_expand_check(const char* fn, const float* x, const float* delta, int batch, int n, int draws, uint32_t it, float norm,
                            float lo, float hi, const float* out, int* l2) {
  if (int rc = hsj_norm(fn, norm, l2)) return rc;
  LP_CHECK_ARG(batch >= 0 && n >= 0 && draws >= 0, "%s: bad shape %d x %d x %d", fn, batch, draws, n);
  LP_CHECK_ARG((long long)batch * draws <= 0x7fffffffLL, "%s: %d x %d rows", fn, batch, draws);
  LP_CHECK_ARG(*l2 || n <= (1 << 17), "%s: rows of %d elements; the L-inf draw's integer norm takes at most 2^17", fn, n);
  LP_CHECK_ARG(it < (1u << 24), "%s: it %u; below 2^24 is required", fn, it);
  LP_CHECK_ARG(lo <= hi, "%s: clip range [%g, %g]", fn, (double)lo, (double)hi);
  if (batch == 0 || n == 0 || draws == 0) return LIPASR_OK;
  LP_CHECK_ARG(x != nullptr && delta != nullptr && out != nullptr, "%s: a null pointer", fn);
  LP_CHECK_ARG(!spans_overlap(x, (size_t)batch * n * 4, out, (size_t)batch * draws * n * 4), "%s: out overlaps x", fn);
  return LIPASR_OK;
}

static int hsj_acc_check(const char* fn, const float* logits, const int* labels, const float* p, const float* x, int batch, int classes,
                         int n, int draws, const double* sums, const int* counts) {
  LP_CHECK_ARG(batch >= 0 && n >= 0 && draws >= 0, "%s: bad shape %d x %d x %d", fn, batch, draws, n);
  LP_CHECK_ARG(batch <= 65535, "%s: %d rows; at most 65535 per call", fn, batch);
  LP_CHECK_ARG((long long)batch * draws <= 0x7fffffffLL, "%s: %d x %d rows", fn, batch, draws);
  LP_CHECK_ARG(draws <= kHsjMaxDraws, "%s: %d draws; at most %d per call", fn, draws, kHsjMaxDraws);
  LP_CHECK_ARG(classes >= 1 && classes <= kHsjMaxC, "%s: %d classes; 1 to %d are supported", fn, classes, kHsjMaxC);
  if (batch == 0 || n == 0 || draws == 0) return LIPASR_OK;
  LP_CHECK_ARG(logits && labels && p && x && sums && counts, "%s: a null pointer", fn);
  const size_t sb = (size_t)batch * 2 * n * sizeof(double);
  LP_CHECK_ARG(!spans_overlap(sums, sb, p, (size_t)batch * draws * n * 4) && !spans_overlap(sums, sb, x, (size_t)batch * n * 4),
               "%s: sums overlaps an input", fn);
  return LIPASR_OK;
}

static int hsj_dir_check(const char* fn, const double* sums, const int* counts, int batch, int n, float norm, const float* u, int* l2) {
  if (int rc = hsj_norm(fn, norm, l2)) return rc;
  LP_CHECK_ARG(batch >= 0 && n >= 0, "%s: bad shape %d x %d", fn, batch, n);
  if (batch == 0 || n == 0) return LIPASR_OK;
  LP_CHECK_ARG(sums && counts && u, "%s: a null pointer", fn);
  LP_CHECK_ARG(!spans_overlap(sums, (size_t)batch * 2 * n * 8, u, (size_t)batch * n * 4), "%s: u overlaps sums", fn);
  return LIPASR_OK;
}

static int hsj_search_check(const char* fn, const HsjSearchArgs& a, float norm, int* l2) {
  if (int rc = hsj_norm(fn, norm, l2)) return rc;
  LP_CHECK_ARG(a.batch >= 0 && a.n >= 0, "%s: bad shape %d x %d", fn, a.batch, a.n);
  LP_CHECK_ARG(a.mode == LIPASR_HSJ_START || a.mode == LIPASR_HSJ_HALVE || a.mode == LIPASR_HSJ_BISECT, "%s: mode %d", fn, a.mode);
  LP_CHECK_ARG((a.flags & ~(LIPASR_HSJ_FIRST | LIPASR_HSJ_LAST)) == 0, "%s: flags %d", fn, a.flags);
  LP_CHECK_ARG(a.C >= 1 && a.C <= kHsjMaxC, "%s: %d classes; 1 to %d are supported", fn, a.C, kHsjMaxC);
  LP_CHECK_ARG(a.max_halvings >= 1, "%s: max_halvings %d", fn, a.max_halvings);
  LP_CHECK_ARG(a.step_scale >= 0.0f && a.step_scale < INFINITY, "%s: step_scale %g", fn, (double)a.step_scale);
  LP_CHECK_ARG(a.lo <= a.hi, "%s: clip range [%g, %g]", fn, (double)a.lo, (double)a.hi);
  if (a.batch == 0 || a.n == 0) return LIPASR_OK;
  LP_CHECK_ARG(a.x0 && a.x_cand && a.x_far && a.x_adv && a.x_best && a.fstate && a.istate && a.start_lo && a.start_hi && a.theta && a.labels,
               "%s: a null pointer", fn);
  LP_CHECK_ARG((a.flags & LIPASR_HSJ_FIRST) || a.logits != nullptr, "%s: logits are required without LIPASR_HSJ_FIRST", fn);
  LP_CHECK_ARG(a.mode != LIPASR_HSJ_HALVE || a.u != nullptr, "%s: the step needs u", fn);
  const size_t rb = (size_t)a.batch * a.n * 4;
  const void* rows[6] = {a.x0, a.x_cand, a.x_far, a.x_adv, a.x_best, a.u};
  const char* names[6] = {"x0", "x_cand", "x_far", "x_adv", "x_best", "u"};
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      LP_CHECK_ARG(rows[i] == nullptr || rows[j] == nullptr || !spans_overlap(rows[i], rb, rows[j], rb), "%s: %s overlaps %s", fn, names[i],
                   names[j]);
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_debug_hsj_path(int n, int aligned) {
  if (n <= 0) return -1;
  return hsj_expand_instance(n) | ((aligned && n % 4 == 0) ? 64 : 0);  // quads per thread | 32 (1 024 threads) | 64 (float4)
}

int lipasr_hsj_expand(lipasr_handle_t h, const float* x, const float* delta, const int* n_valid, int batch, int n, int draws,
                      uint32_t clip0, uint32_t it, uint32_t draw0, uint64_t seed, float norm, float clip_lo, float clip_hi, float* out,
                      lipasr_stream_t stream) {
  const char* fn = "lipasr_hsj_expand";
  int l2 = 0;
  if (int rc = hsj_expand_check(fn, x, delta, batch, n, draws, it, norm, clip_lo, clip_hi, out, &l2)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0 || draws == 0) return LIPASR_OK;
  HsjExpandArgs a;
  a.x = x; a.delta = delta; a.n_valid = n_valid; a.out = out;
  a.batch = batch; a.n = n; a.draws = draws; a.l2 = l2;
  a.vec = (n % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) ? 1 : 0;
  a.clip0 = clip0; a.it = it; a.draw0 = draw0; a.seed = seed; a.lo = clip_lo; a.hi = clip_hi;
  const dim3 grid((unsigned)(batch * draws)), block(kHsjThreads), wide(kHsjWideThreads);
  const hipStream_t st = S(stream);
  switch (hsj_expand_instance(n)) {
    case 1: hipLaunchKernelGGL((hsj_expand_kernel<1, kHsjThreads>), grid, block, 0, st, a); break;  // 880
    case 2: hipLaunchKernelGGL((hsj_expand_kernel<2, kHsjThreads>), grid, block, 0, st, a); break;  // 2 020
    case 4: hipLaunchKernelGGL((hsj_expand_kernel<4, kHsjThreads>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((hsj_expand_kernel<8, kHsjThreads>), grid, block, 0, st, a); break;
    case 4 | kHsjWide: hipLaunchKernelGGL((hsj_expand_kernel<4, kHsjWideThreads>), grid, wide, 0, st, a); break;  // 16 000
    case 6 | kHsjWide: hipLaunchKernelGGL((hsj_expand_kernel<6, kHsjWideThreads>), grid, wide, 0, st, a); break;  // 22 050
    default: hipLaunchKernelGGL((hsj_expand_kernel<0, kHsjThreads>), grid, block, 0, st, a); break;
  }
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_hsj_expand_host(const float* x, const float* delta, const int* n_valid, int batch, int n, int draws, uint32_t clip0,
                           uint32_t it, uint32_t draw0, uint64_t seed, float norm, float clip_lo, float clip_hi, float* out) {
  const char* fn = "lipasr_hsj_expand_host";
  int l2 = 0;
  if (int rc = hsj_expand_check(fn, x, delta, batch, n, draws, it, norm, clip_lo, clip_hi, out, &l2)) return rc;
  if (batch == 0 || n == 0 || draws == 0) return LIPASR_OK;
  const int quads = (n + 3) >> 2;
  std::vector<float> r((size_t)quads * 4);
  for (int b = 0; b < batch; ++b) {
    const int nv = row_valid(n_valid, b, n);
    for (int j = 0; j < draws; ++j) {
      double ss = 0.0;
      uint64_t si = 0;
      for (int q = 0; q < quads; ++q) {
        float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (4 * q < nv) hsj_draw4(l2, seed, clip0 + (uint32_t)b, it, draw0 + (uint32_t)j, q, t);
        for (int e = 0; e < 4; ++e) {
          const float v = (4 * q + e < nv) ? t[e] : 0.0f;
          r[(size_t)4 * q + e] = v;
          if (l2) ss += (double)v * (double)v; else si += hsj_sq_int(v);
        }
      }
      const float sc = hsj_scale(l2, ss, si, delta[b]);
      float* o = out + ((size_t)b * draws + j) * n;
      const float* xr = x + (size_t)b * n;
      for (int k = 0; k < n; ++k) o[k] = k < nv ? hsj_point(sc, r[k], xr[k], clip_lo, clip_hi) : xr[k];
    }
  }
  return LIPASR_OK;
}

int lipasr_hsj_accumulate(lipasr_handle_t h, const float* logits, const int* labels, const float* p, const float* x, const int* n_valid,
                          int batch, int classes, int n, int draws, int targeted, double* sums, int* counts, lipasr_stream_t stream) {
  const char* fn = "lipasr_hsj_accumulate";
  if (int rc = hsj_acc_check(fn, logits, labels, p, x, batch, classes, n, draws, sums, counts)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0 || draws == 0) return LIPASR_OK;
  const int vec = (n % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(p)) & 15) == 0) ? 1 : 0;
  const int quads = (n + 3) >> 2;
  hipLaunchKernelGGL(hsj_accumulate_kernel, dim3((unsigned)((quads + kHsjAccThreads - 1) / kHsjAccThreads), (unsigned)batch),
                     dim3(kHsjAccThreads), 0, S(stream), logits, labels, p, x, n_valid, classes, n, draws, targeted ? 1 : 0, vec, sums,
                     counts);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_hsj_accumulate_host(const float* logits, const int* labels, const float* p, const float* x, const int* n_valid, int batch,
                               int classes, int n, int draws, int targeted, double* sums, int* counts) {
  const char* fn = "lipasr_hsj_accumulate_host";
  if (int rc = hsj_acc_check(fn, logits, labels, p, x, batch, classes, n, draws, sums, counts)) return rc;
  if (batch == 0 || n == 0 || draws == 0) return LIPASR_OK;
  for (int b = 0; b < batch; ++b) {
    const int nv = row_valid(n_valid, b, n);
    double* s0 = sums + ((size_t)b * 2) * n;
    double* s1 = s0 + n;
    int pos = 0;
    for (int j = 0; j < draws; ++j) {
      const bool plus = hsj_adv(logits + ((size_t)b * draws + j) * classes, classes, labels[b], targeted ? 1 : 0);
      pos += plus ? 1 : 0;
      const float* pr = p + ((size_t)b * draws + j) * n;
      for (int k = 0; k < n; ++k) {
        const double d = k < nv ? (double)pr[k] - (double)x[(size_t)b * n + k] : 0.0;
        s0[k] += d;
        s1[k] += plus ? d : -d;
      }
    }
    counts[(size_t)b * 2] += draws;
    counts[(size_t)b * 2 + 1] += pos;
  }
  return LIPASR_OK;
}

int lipasr_hsj_direction(lipasr_handle_t h, const double* sums, const int* counts, const int* n_valid, int batch, int n, float norm,
                         float* u, lipasr_stream_t stream) {
  const char* fn = "lipasr_hsj_direction";
  int l2 = 0;
  if (int rc = hsj_dir_check(fn, sums, counts, batch, n, norm, u, &l2)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0) return LIPASR_OK;
  const int vec = (n % 4 == 0 && (reinterpret_cast<uintptr_t>(u) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(hsj_direction_kernel, dim3((unsigned)batch), dim3(kHsjThreads), 0, S(stream), sums, counts, n_valid, n, l2, vec, u);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_hsj_direction_host(const double* sums, const int* counts, const int* n_valid, int batch, int n, float norm, float* u) {
  const char* fn = "lipasr_hsj_direction_host";
  int l2 = 0;
  if (int rc = hsj_dir_check(fn, sums, counts, batch, n, norm, u, &l2)) return rc;
  if (batch == 0 || n == 0) return LIPASR_OK;
  for (int b = 0; b < batch; ++b) {
    const int nv = row_valid(n_valid, b, n);
    const int total = counts[(size_t)b * 2], pos = counts[(size_t)b * 2 + 1];
    const double* s0 = sums + ((size_t)b * 2) * n;
    const double* s1 = s0 + n;
    double ss = 0.0;
    if (l2)
      for (int k = 0; k < nv; ++k) { const double g = hsj_g(s0[k], s1[k], total, pos); ss += g * g; }
    const double nrm = sqrt(ss);
    for (int k = 0; k < n; ++k) {
      float o = 0.0f;
      if (k < nv) { const double g = hsj_g(s0[k], s1[k], total, pos); o = l2 ? hsj_unit(g, nrm) : hsj_sign(g); }
      u[(size_t)b * n + k] = o;
    }
  }
  return LIPASR_OK;
}

static void hsj_fill_search(HsjSearchArgs& a, const float* logits, const int* labels, const float* x0, const int* n_valid, const float* u,
                            const float* start_lo, const float* start_hi, const float* theta, int batch, int classes, int n, int mode,
                            int flags, int targeted, uint32_t clip0, uint32_t draw, uint64_t seed, float step_scale, int max_halvings,
                            float clip_lo, float clip_hi, float* x_cand, float* x_far, float* x_adv, float* x_best, float* fstate,
                            int* istate) {
  a.logits = logits; a.labels = labels; a.x0 = x0; a.n_valid = n_valid; a.u = u;
  a.start_lo = start_lo; a.start_hi = start_hi; a.theta = theta;
  a.x_cand = x_cand; a.x_far = x_far; a.x_adv = x_adv; a.x_best = x_best; a.fstate = fstate; a.istate = istate;
  a.batch = batch; a.C = classes; a.n = n; a.mode = mode; a.flags = flags; a.targeted = targeted ? 1 : 0; a.l2 = 0;
  a.max_halvings = max_halvings; a.vec = 0;
  a.clip0 = clip0; a.draw = draw; a.seed = seed; a.step_scale = step_scale; a.lo = clip_lo; a.hi = clip_hi;
}

int lipasr_hsj_search(lipasr_handle_t h, const float* logits, const int* labels, const float* x0, const int* n_valid, const float* u,
                      const float* start_lo, const float* start_hi, const float* theta, int batch, int classes, int n, int mode,
                      int flags, int targeted, uint32_t clip0, uint32_t draw, uint64_t seed, float norm, float step_scale,
                      int max_halvings, float clip_lo, float clip_hi, float* x_cand, float* x_far, float* x_adv, float* x_best,
                      float* fstate, int* istate, lipasr_stream_t stream) {
  const char* fn = "lipasr_hsj_search";
  HsjSearchArgs a;
  hsj_fill_search(a, logits, labels, x0, n_valid, u, start_lo, start_hi, theta, batch, classes, n, mode, flags, targeted, clip0, draw,
                  seed, step_scale, max_halvings, clip_lo, clip_hi, x_cand, x_far, x_adv, x_best, fstate, istate);
  if (int rc = hsj_search_check(fn, a, norm, &a.l2)) return rc;
  LP_CHECK_ARG(h != nullptr, "%s: null handle", fn);
  if (batch == 0 || n == 0) return LIPASR_OK;
  uintptr_t bits = 0;
  for (const void* p : {(const void*)x0, (const void*)x_cand, (const void*)x_far, (const void*)x_adv, (const void*)x_best, (const void*)u})
    bits |= reinterpret_cast<uintptr_t>(p);
  a.vec = (n % 4 == 0 && (bits & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(hsj_search_kernel, dim3((unsigned)batch), dim3(kHsjThreads), 0, S(stream), a);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_hsj_search_host(const float* logits, const int* labels, const float* x0, const int* n_valid, const float* u,
                           const float* start_lo, const float* start_hi, const float* theta, int batch, int classes, int n, int mode,
                           int flags, int targeted, uint32_t clip0, uint32_t draw, uint64_t seed, float norm, float step_scale,
                           int max_halvings, float clip_lo, float clip_hi, float* x_cand, float* x_far, float* x_adv, float* x_best,
                           float* fstate, int* istate) {
  const char* fn = "lipasr_hsj_search_host";
  HsjSearchArgs a;
  hsj_fill_search(a, logits, labels, x0, n_valid, u, start_lo, start_hi, theta, batch, classes, n, mode, flags, targeted, clip0, draw,
                  seed, step_scale, max_halvings, clip_lo, clip_hi, x_cand, x_far, x_adv, x_best, fstate, istate);
  if (int rc = hsj_search_check(fn, a, norm, &a.l2)) return rc;
  if (batch == 0 || n == 0) return LIPASR_OK;
  const int l2 = a.l2;
  const bool first = (flags & LIPASR_HSJ_FIRST) != 0;
  for (int b = 0; b < batch; ++b) {
    const size_t base = (size_t)b * n;
    const int nv = row_valid(n_valid, b, n);
    HsjRow r;
    hsj_load_row(fstate + (size_t)b * 8, istate + (size_t)b * 8, r);
    const bool adv = first ? false : hsj_adv(logits + (size_t)b * classes, classes, labels[b], targeted ? 1 : 0);
    const float* c = x0 + base;
    float dist_far = 0.0f;
    if (hsj_needs_far(r, mode, flags, l2, nv))
      for (int k = 0; k < nv; ++k) dist_far = fmaxf(dist_far, fabsf(x_far[base + k] - c[k]));
    const HsjOps op = hsj_decide(r, mode, flags, adv, nv, l2, theta[b], step_scale, max_halvings, draw, dist_far);
    const uint32_t clip = clip0 + (uint32_t)b;
    if (op.init_rows)
      for (int k = 0; k < n; ++k) x_adv[base + k] = x_best[base + k] = c[k];
    if (op.far_from_cand)
      for (int k = 0; k < n; ++k) x_far[base + k] = x_cand[base + k];
    if (op.cand == 1) {
      for (int q = 0; 4 * q < n; ++q) {
        float uu[4];
        hsj_start4(seed, clip, op.draw, q, uu);
        for (int e = 0; e < 4 && 4 * q + e < n; ++e) {
          const int k = 4 * q + e;
          x_cand[base + k] = k < nv ? hsj_start_value(uu[e], start_lo[b], start_hi[b]) : c[k];
        }
      }
    } else if (op.cand == 2) {
      for (int k = 0; k < n; ++k) x_cand[base + k] = k < nv ? hsj_point(r.eps, u[base + k], x_adv[base + k], clip_lo, clip_hi) : c[k];
    } else if (op.cand == 3) {
      for (int k = 0; k < n; ++k) x_cand[base + k] = k < nv ? hsj_proj(l2, r.mid, c[k], x_far[base + k], clip_lo, clip_hi) : c[k];
    } else if (op.cand == 4) {
      for (int k = 0; k < n; ++k) x_cand[base + k] = c[k];
    }
    if (op.finish) {
      double ss = 0.0;
      float mx = 0.0f;
      for (int k = 0; k < n; ++k) {
        const float v = k < nv ? (r.moved ? hsj_proj(l2, r.hi, c[k], x_far[base + k], clip_lo, clip_hi) : x_far[base + k]) : c[k];
        x_adv[base + k] = v;
        if (k < nv) {
          if (l2) { const double d = (double)v - (double)c[k]; ss += d * d; }
          else mx = fmaxf(mx, fabsf(v - c[k]));
        }
      }
      r.dist = l2 ? (float)sqrt(ss) : mx;
      if (r.dist < r.dist_best) {
        r.dist_best = r.dist;
        for (int k = 0; k < n; ++k) x_best[base + k] = x_adv[base + k];
      }
    }
    hsj_store_row(fstate + (size_t)b * 8, istate + (size_t)b * 8, r);
  }
  return LIPASR_OK;
}

}  // extern "C"
