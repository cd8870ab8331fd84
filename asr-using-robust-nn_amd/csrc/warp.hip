// The time-warp operator (lipasr/warp.py, attacks.TimeWarp): every clip resampled under K triples (shift, rate, gain) in one launch,
// and the derivative of the result with respect to the three parameters.  (include/lipasr.h, lipasr_warp_apply, fixes the formula.)
//
//   lipasr_warp_apply      out[b * K + j][t] = gain * sum_k w_k(u) x[b][n0 + k],  u = c + rate (t - c) - shift, c = (nv_b - 1) / 2
//   lipasr_warp_param_vjp  gp[b * K + j] = (d/dshift, d/drate, d/dgain) of sum_t g[b * K + j][t] out[b * K + j][t]
//
// The interpolation kernel is a Kaiser-windowed sinc with its cutoff at Nyquist, tabulated at kWarpP steps per zero crossing over
// kWarpZ crossings (win) with the first differences next to it (delta); a tap weight is fmaf(eta, delta[j], win[j]), the table read
// linearly, and d weight / du is +-delta[j] kWarpP, so one table serves the value and the slope.
//
// warp_kernel<VJP>: 512 threads own (a row's source clip, a span of 1 024 output positions).  LDS holds the table as (win, delta)
//   pairs (65.5 kB: one ds_read_b64 per tap) and the source window of the span under the current triple, zero outside [0, nv)
//   (at most 2 * 1 024 + 2 Z + 4 samples, 8.4 kB): 74 kB, two workgroups and 16 wavefronts per CU.  The table reads are gathers at
//   j0 + i kWarpP; kWarpP is a multiple of the 32 eight-byte banks, so the 2 Z taps of a position meet one bank each and lanes
//   conflict only through j0 (2 to 4 ways at rates 0.9 to 1.07, none at rate 1 where j0 is nearly one value: a broadcast).
//   VJP = false: grid clips x spans; the workgroup walks the K triples of its clip, staging the window of each, so the table
//   is loaded once for K spans of output.  VJP = true: grid clips * K; the workgroup walks the spans of its row, thread t mod 512
//   adds the three fp64 terms of its positions in ascending t, and the partials meet in block_sum_d's order: no atomics, no
//   workspace.  Every output position is its own chain, so neither the grid nor the batch can change a bit.
//   There is no rate == 1 fast path: t - shift rounds at t's own exponent in fp64, so f, and with it eta, differs in its last bits
//   from one t to the next, and weights formed once per row would not be the bits of the general path.
// A wavefront never reads outside its window: the window is sized from u at the span's two ends (u is monotone in t: every step
// of it is), and a position whose n0 falls outside it -- which no finite triple produces -- is written as 0.
// Every a * b + c that the bits depend on is an explicit fmaf, and contraction is off for the whole file (as in hsj.hip), so the
// host twins and the device round alike.
#include "common.h"
#include "row.h"

#pragma clang fp contract(off)

namespace lipasr {

constexpr int kWarpZ = 16;                        // zero crossings per wing
constexpr int kWarpP = 512;                       // table steps per crossing
constexpr int kWarpTab = kWarpZ * kWarpP + 1;     // entries of win and of delta
constexpr double kWarpBeta = 8.6;
constexpr int kWarpThreads = 512;
constexpr int kWarpSpan = 1024;                   // output positions of a workgroup per step
constexpr int kWarpEach = kWarpSpan / kWarpThreads;
constexpr int kWarpReach = 2 * kWarpSpan + 4;     // floor(u) over a span moves by at most rate (span - 1) + 2 <= this
constexpr int kWarpWin = kWarpReach + 2 * kWarpZ + 4;  // staged source samples
constexpr int kWarpMaxN = 1 << 24;
constexpr size_t kWarpLds = (size_t)(2 * kWarpTab + kWarpWin) * sizeof(float) + (kWarpThreads / 64) * sizeof(double);
static_assert((2 * kWarpTab + kWarpWin) % 2 == 0, "the fp64 slots of block_sum_d sit on 8 bytes");

long g_warp_launches[2] = {};

// a triple that is written as NaN: something not finite, or a rate outside [0.5, 2]
__host__ __device__ __forceinline__ bool warp_bad(float shift, float rate, float gain) {
  return !(fabsf(shift) < INFINITY && fabsf(gain) < INFINITY && rate >= 0.5f && rate <= 2.0f);
}

__host__ __device__ __forceinline__ double warp_u(double c, double rate, double shift, int t) {
  const double d = (double)t - c;
  const double r = rate * d;
  const double a = c + r;
  return a - shift;
}

// where output position t reads: n0 = floor(u) and, per wing, the table index and the fp32 fraction of a table step.  false: u
// is so far outside the clip that no tap has a sample (and n0 need not fit an int).
__host__ __device__ __forceinline__ bool warp_pos(double u, int nv, int& n0, int& jl, float& el, int& jr, float& er) {
  const double u0 = floor(u);
  if (!(u0 >= -(double)(kWarpZ + 1) && u0 <= (double)(nv + kWarpZ))) return false;
  n0 = (int)u0;
  const double f = u - u0;
  const double il = f * (double)kWarpP;
  jl = (int)il;
  el = (float)(il - (double)jl);
  const double fr = 1.0 - f;
  const double ir = fr * (double)kWarpP;
  jr = (int)ir;
  er = (float)(ir - (double)jr);
  return true;
}

// one tap: the weight's own fma, then the chain's; the slope chain next to it
template <bool VJP>
__host__ __device__ __forceinline__ void warp_tap(float win, float delta, float eta, float sign_p, float xv, float& acc, float& dxu) {
  acc = fmaf(fmaf(eta, delta, win), xv, acc);
  if (VJP) dxu = fmaf(delta * sign_p, xv, dxu);
}

// the three fp64 terms of position t
__host__ __device__ __forceinline__ void warp_terms(float gv, float gain, float acc, float dxu, int t, double c, double (&s)[3]) {
  const double gd = (double)gv;
  const double a = gd * (double)gain;
  const double p0 = a * (-(double)dxu);
  const double q = a * (double)dxu;
  const double p1 = q * ((double)t - c);
  const double p2 = gd * (double)acc;
  s[0] = s[0] + p0;
  s[1] = s[1] + p1;
  s[2] = s[2] + p2;
}

// acc (and dxu) of the positions s0 + tid + e * 512 of one row under one triple; xr is the row's clip.  The same barriers in every
// thread: what decides them is the same in all.
template <bool VJP>
__device__ __forceinline__ void warp_span(const float* __restrict__ xr, int nv, double c, double rate, double shift, int s0,
                                          const float2* tab, float* xs, float (&acc)[kWarpEach], float (&dxu)[kWarpEach]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < kWarpEach; ++e) acc[e] = dxu[e] = 0.0f;
  const int tl = min(s0 + kWarpSpan, nv) - 1;
  const double lo_d = fmax(floor(warp_u(c, rate, shift, s0)), -(double)(kWarpZ + 1));
  const double hi_d = fmin(floor(warp_u(c, rate, shift, tl)), (double)(nv + kWarpZ));
  if (!(lo_d <= hi_d)) return;  // the whole span reads outside the clip
  const int lo = (int)lo_d;
  const int reach = min((int)hi_d - lo, kWarpReach);
  const int len = reach + 2 * kWarpZ;  // source positions lo - (Z - 1) .. lo + reach + Z
  __syncthreads();                     // the previous window is read (and the table is written)
  for (int k = tid; k < len; k += kWarpThreads) {
    const int p = lo - (kWarpZ - 1) + k;
    xs[k] = (p >= 0 && p < nv) ? xr[p] : 0.0f;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kWarpEach; ++e) {
    const int t = s0 + tid + e * kWarpThreads;
    int n0 = 0, jl = 0, jr = 0;
    float el = 0.0f, er = 0.0f;
    if (t >= nv || !warp_pos(warp_u(c, rate, shift, t), nv, n0, jl, el, jr, er)) continue;
    const int rel = n0 - lo;
    if (rel < 0 || rel > reach) continue;
    const float* xl = xs + rel + (kWarpZ - 1);
    float a = 0.0f, d = 0.0f;
#pragma unroll
    for (int i = 0; i < kWarpZ; ++i) {
      const float2 w = tab[jl + i * kWarpP];
      warp_tap<VJP>(w.x, w.y, el, (float)kWarpP, xl[-i], a, d);
    }
#pragma unroll
    for (int k = 0; k < kWarpZ; ++k) {
      const float2 w = tab[jr + k * kWarpP];
      warp_tap<VJP>(w.x, w.y, er, -(float)kWarpP, xl[1 + k], a, d);
    }
    acc[e] = a;
    dxu[e] = d;
  }
}

// gp is written as dwords so that it may sit on any 4-byte boundary
__device__ __forceinline__ void warp_store_d(double* p, double v) {
  unsigned* q = reinterpret_cast<unsigned*>(p);
  q[0] = (unsigned)__double2loint(v);
  q[1] = (unsigned)__double2hiint(v);
}

template <bool VJP>
__global__ __launch_bounds__(kWarpThreads) void warp_kernel(const float* __restrict__ x, const int* __restrict__ n_valid,
                                                            const float* __restrict__ params, const float* __restrict__ table,
                                                            const float* __restrict__ g, int K, int n, int spans,
                                                            float* __restrict__ out, double* __restrict__ gp) {
  extern __shared__ __attribute__((aligned(16))) float warp_lds[];
  float2* tab = reinterpret_cast<float2*>(warp_lds);
  float* xs = warp_lds + 2 * kWarpTab;
  const int tid = threadIdx.x;
  const int b = VJP ? (int)(blockIdx.x / (unsigned)K) : (int)(blockIdx.x / (unsigned)spans);
  const int nv = row_valid(n_valid, b, n);
  const double c = ((double)nv - 1.0) / 2.0;
  const float* xr = x + (size_t)b * n;
  auto load_table = [&]() {
    for (int i = tid; i < kWarpTab; i += kWarpThreads) tab[i] = make_float2(table[2 * i], table[2 * i + 1]);
  };
  float acc[kWarpEach] = {}, dxu[kWarpEach] = {};
  if constexpr (!VJP) {
    const int s0 = (int)(blockIdx.x % (unsigned)spans) * kWarpSpan;
    const bool live = s0 < nv;
    if (live) load_table();
    for (int j = 0; j < K; ++j) {
      const size_t row = (size_t)b * K + j;
      const float shift = params[3 * row], rate = params[3 * row + 1], gain = params[3 * row + 2];
      const bool bad = warp_bad(shift, rate, gain);
      if (live && !bad) warp_span<false>(xr, nv, c, (double)rate, (double)shift, s0, tab, xs, acc, dxu);
#pragma unroll
      for (int e = 0; e < kWarpEach; ++e) {
        const int t = s0 + tid + e * kWarpThreads;
        if (t < n) out[row * (size_t)n + t] = t < nv ? (bad ? NAN : gain * acc[e]) : 0.0f;
      }
    }
  } else {
    double* red = reinterpret_cast<double*>(xs + kWarpWin);
    const size_t row = blockIdx.x;
    const float shift = params[3 * row], rate = params[3 * row + 1], gain = params[3 * row + 2];
    double s[3] = {0.0, 0.0, 0.0};
    if (warp_bad(shift, rate, gain)) {
      s[0] = s[1] = s[2] = (double)NAN;
    } else if (nv > 0) {
      load_table();
      const float* gr = g + row * (size_t)n;
      for (int s0 = 0; s0 < nv; s0 += kWarpSpan) {
        warp_span<true>(xr, nv, c, (double)rate, (double)shift, s0, tab, xs, acc, dxu);
#pragma unroll
        for (int e = 0; e < kWarpEach; ++e) {
          const int t = s0 + tid + e * kWarpThreads;
          if (t < nv) warp_terms(gr[t], gain, acc[e], dxu[e], t, c, s);
        }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) s[q] = block_sum_d<kWarpThreads>(s[q], red);
    }
    if (tid < 3) warp_store_d(gp + 3 * row + tid, tid == 0 ? s[0] : (tid == 1 ? s[1] : s[2]));
  }
}

// ------------------------------------------------------------------------------------------------------------------------ checks
static int warp_check(const char* fn, const float* x, const int* n_valid, const float* params, const float* table, const float* g,
                      int clips, int K, int n, const void* dst, bool vjp) {
  LP_CHECK_ARG(clips >= 0 && K >= 0 && n >= 0, "%s: bad shape %d x %d x %d", fn, clips, K, n);
  LP_CHECK_ARG(n <= kWarpMaxN, "%s: rows of %d elements; at most 2^24", fn, n);
  LP_CHECK_ARG((long long)clips * K <= 0x7fffffffLL / 3, "%s: %d x %d rows", fn, clips, K);
  if (clips == 0 || K == 0 || n == 0) return LIPASR_OK;
  LP_CHECK_ARG(x != nullptr && params != nullptr && table != nullptr && dst != nullptr && (!vjp || g != nullptr), "%s: a null pointer", fn);
  const size_t rows = (size_t)clips * K;
  const size_t xb = (size_t)clips * n * 4, pb = rows * 3 * 4, tb = (size_t)2 * kWarpTab * 4, rb = rows * n * 4;
  const size_t db = vjp ? rows * 3 * sizeof(double) : rb;
  LP_CHECK_ARG(!spans_overlap(dst, db, x, xb) && !spans_overlap(dst, db, params, pb) && !spans_overlap(dst, db, table, tb) &&
                   !(vjp && spans_overlap(dst, db, g, rb)) && !(n_valid && spans_overlap(dst, db, n_valid, (size_t)clips * 4)),
               "%s: the output overlaps an input", fn);
  return LIPASR_OK;
}

// I0 by its power series: every term is positive, and 64 of them leave nothing above 1e-17 of the sum at beta = 8.6
static double warp_i0(double v) {
  const double q = v * v / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 64; ++k) {
    term = term * q / ((double)k * (double)k);
    sum = sum + term;
  }
  return sum;
}

// the host twins' chain for one position: the device's order, taps without a sample or a table entry left out
template <bool VJP>
static inline bool warp_point_host(const float* xr, int nv, const float* table, double c, double rate, double shift, int t, float& acc,
                                   float& dxu) {
  acc = dxu = 0.0f;
  int n0 = 0, jl = 0, jr = 0;
  float el = 0.0f, er = 0.0f;
  if (!warp_pos(warp_u(c, rate, shift, t), nv, n0, jl, el, jr, er)) return false;
  for (int i = 0; i < kWarpZ; ++i) {
    const int p = n0 - i, j = jl + i * kWarpP;
    if (p < 0 || p >= nv || j >= kWarpTab) continue;
    warp_tap<VJP>(table[2 * j], table[2 * j + 1], el, (float)kWarpP, xr[p], acc, dxu);
  }
  for (int k = 0; k < kWarpZ; ++k) {
    const int p = n0 + 1 + k, j = jr + k * kWarpP;
    if (p < 0 || p >= nv || j >= kWarpTab) continue;
    warp_tap<VJP>(table[2 * j], table[2 * j + 1], er, -(float)kWarpP, xr[p], acc, dxu);
  }
  return true;
}

// block_sum_d<kWarpThreads> restated: v[lane] + v[lane ^ o] for o = 32 .. 1 in every wavefront, then the wavefronts in index order
static double warp_block_sum_host(double* v) {
  double tmp[64];
  double sum = 0.0;
  for (int w = 0; w < kWarpThreads / 64; ++w) {
    double* l = v + 64 * w;
    for (int o = 32; o > 0; o >>= 1) {
      for (int i = 0; i < 64; ++i) tmp[i] = l[i] + l[i ^ o];
      for (int i = 0; i < 64; ++i) l[i] = tmp[i];
    }
    sum = sum + l[0];
  }
  return sum;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

int lipasr_warp_table_host(float* win, float* delta) {
  LP_CHECK_ARG(win != nullptr && delta != nullptr, "lipasr_warp_table_host: a null pointer");
  const double pi = 3.14159265358979323846;
  const double i0b = warp_i0(kWarpBeta);
  for (int i = 0; i < kWarpTab; ++i) {
    const double v = (double)i / (double)kWarpP;
    const double r = (double)i / (double)(kWarpTab - 1);
    const double kaiser = warp_i0(kWarpBeta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    double w = i == 0 ? 1.0 : std::sin(pi * v) / (pi * v) * kaiser;
    if (i != 0 && i % kWarpP == 0) w = 0.0;  // sin(pi k) is not 0 in floating point; the kernel is
    win[i] = (float)w;
  }
  for (int i = 0; i + 1 < kWarpTab; ++i) delta[i] = win[i + 1] - win[i];
  delta[kWarpTab - 1] = 0.0f;
  return LIPASR_OK;
}

int lipasr_warp_apply(const float* x, const int* n_valid, const float* params, const float* table, int clips, int K, int n, float* out,
                      lipasr_stream_t stream) {
  const char* fn = "lipasr_warp_apply";
  if (int rc = warp_check(fn, x, n_valid, params, table, nullptr, clips, K, n, out, false)) return rc;
  if (clips == 0 || K == 0 || n == 0) return LIPASR_OK;
  const long long spans = ((long long)n + kWarpSpan - 1) / kWarpSpan;
  LP_CHECK_ARG(spans * clips <= 0x7fffffffLL, "%s: %lld workgroups; split the batch", fn, spans * clips);
  LP_DYN_LDS(warp_kernel<false>, kWarpLds);
  hipLaunchKernelGGL(warp_kernel<false>, dim3((unsigned)(spans * clips)), dim3(kWarpThreads), kWarpLds, S(stream), x, n_valid, params,
                     table, (const float*)nullptr, K, n, (int)spans, out, (double*)nullptr);
  ++g_warp_launches[0];
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_warp_param_vjp(const float* x, const float* g, const int* n_valid, const float* params, const float* table, int clips, int K,
                          int n, double* gp, lipasr_stream_t stream) {
  const char* fn = "lipasr_warp_param_vjp";
  if (int rc = warp_check(fn, x, n_valid, params, table, g, clips, K, n, gp, true)) return rc;
  if (clips == 0 || K == 0 || n == 0) return LIPASR_OK;
  LP_DYN_LDS(warp_kernel<true>, kWarpLds);
  hipLaunchKernelGGL(warp_kernel<true>, dim3((unsigned)((size_t)clips * K)), dim3(kWarpThreads), kWarpLds, S(stream), x, n_valid, params,
                     table, g, K, n, 0, (float*)nullptr, gp);
  ++g_warp_launches[1];
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_warp_apply_host(const float* x, const int* n_valid, const float* params, const float* table, int clips, int K, int n,
                           float* out) {
  const char* fn = "lipasr_warp_apply_host";
  if (int rc = warp_check(fn, x, n_valid, params, table, nullptr, clips, K, n, out, false)) return rc;
  if (clips == 0 || K == 0 || n == 0) return LIPASR_OK;
  for (int b = 0; b < clips; ++b) {
    const int nv = row_valid(n_valid, b, n);
    const double c = ((double)nv - 1.0) / 2.0;
    const float* xr = x + (size_t)b * n;
    for (int j = 0; j < K; ++j) {
      const size_t row = (size_t)b * K + j;
      const float shift = params[3 * row], rate = params[3 * row + 1], gain = params[3 * row + 2];
      const bool bad = warp_bad(shift, rate, gain);
      float* o = out + row * (size_t)n;
      for (int t = 0; t < n; ++t) {
        float acc = 0.0f, dxu = 0.0f;
        if (t < nv && !bad) warp_point_host<false>(xr, nv, table, c, (double)rate, (double)shift, t, acc, dxu);
        o[t] = t < nv ? (bad ? NAN : gain * acc) : 0.0f;
      }
    }
  }
  return LIPASR_OK;
}

int lipasr_warp_param_vjp_host(const float* x, const float* g, const int* n_valid, const float* params, const float* table, int clips,
                               int K, int n, double* gp) {
  const char* fn = "lipasr_warp_param_vjp_host";
  if (int rc = warp_check(fn, x, n_valid, params, table, g, clips, K, n, gp, true)) return rc;
  if (clips == 0 || K == 0 || n == 0) return LIPASR_OK;
  std::vector<double> part(3 * (size_t)kWarpThreads);
  for (int b = 0; b < clips; ++b) {
    const int nv = row_valid(n_valid, b, n);
    const double c = ((double)nv - 1.0) / 2.0;
    const float* xr = x + (size_t)b * n;
    for (int j = 0; j < K; ++j) {
      const size_t row = (size_t)b * K + j;
      const float shift = params[3 * row], rate = params[3 * row + 1], gain = params[3 * row + 2];
      double res[3] = {0.0, 0.0, 0.0};
      if (warp_bad(shift, rate, gain)) {
        res[0] = res[1] = res[2] = (double)NAN;
      } else if (nv > 0) {
        const float* gr = g + row * (size_t)n;
        std::fill(part.begin(), part.end(), 0.0);
        for (int t = 0; t < nv; ++t) {  // thread t mod 512 takes position t, in ascending t
          const int th = t % kWarpThreads;
          float acc = 0.0f, dxu = 0.0f;
          warp_point_host<true>(xr, nv, table, c, (double)rate, (double)shift, t, acc, dxu);
          double s[3] = {part[th], part[kWarpThreads + th], part[2 * kWarpThreads + th]};
          warp_terms(gr[t], gain, acc, dxu, t, c, s);
          for (int q = 0; q < 3; ++q) part[q * kWarpThreads + th] = s[q];
        }
        for (int q = 0; q < 3; ++q) res[q] = warp_block_sum_host(part.data() + q * kWarpThreads);
      }
      std::memcpy(reinterpret_cast<char*>(gp) + (3 * row) * sizeof(double), res, sizeof(res));
    }
  }
  return LIPASR_OK;
}

long lipasr_debug_warp_launches(int kernel) { return (kernel == 0 || kernel == 1) ? g_warp_launches[kernel] : -1; }

}  // extern "C"
