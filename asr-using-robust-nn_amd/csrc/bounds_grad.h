// What bounds_grad.hip and bounds_crown_grad.hip share: the sliced column sum (device and host), exp and log written out in + * /,
// the scale-and-mix of a gradient entry, the label guard, and the stores of a head entry and of a hidden column.
#pragma once
#include "bounds.h"

// host and device must round alike
#pragma clang fp contract(off)

namespace lipasr {

// a column sum over the batch: a block takes kBgCols columns, thread slice s of a column the rows s, s + kBgSlices, ...  (8 x 32
// and not 32 x 8: at batch 1024 a slice is 32 dependent loads, not 128, and a 1024-wide layer is 128 blocks, not 32)
constexpr int kBgCols = 8;
constexpr int kBgSlices = kBdThreads / kBgCols;

// NS (1 or 3) such sums of the block's column threadIdx.x % kBgCols over the rows [begin, end).  term(r, acc) adds row r's terms to
// acc[0 .. NS): slice sl takes the rows begin + sl, begin + sl + 32, ... in ascending order, the partials go to LDS, and slice 0
// adds the 32 partials in index order and hands the totals to store(tot).  on: the column exists.  Every thread of the block calls.
template <int NS, class Term, class Store>
__device__ __forceinline__ void bg_sliced_sum(bool on, int begin, int end, const Term& term, const Store& store) {
  __shared__ double parts[NS][kBgSlices][kBgCols];
  const int cl = threadIdx.x % kBgCols, sl = threadIdx.x / kBgCols;
  double acc[NS] = {};
  if (on)
    for (int r = begin + sl; r < end; r += kBgSlices) term(r, acc);
#pragma unroll
  for (int n = 0; n < NS; ++n) parts[n][sl][cl] = acc[n];
  __syncthreads();
  if (sl == 0 && on) {
#pragma unroll
    for (int n = 0; n < NS; ++n) acc[n] = parts[n][0][cl];
    for (int q = 1; q < kBgSlices; ++q)
#pragma unroll
      for (int n = 0; n < NS; ++n) acc[n] = acc[n] + parts[n][q][cl];
    store(acc);
  }
}
// the same order on the host, one sum: term(r) is row r's term
template <class Term>
inline double bg_sliced_sum_host(int begin, int end, const Term& term) {
  double part[kBgSlices] = {};
  for (int r = begin; r < end; ++r) part[(r - begin) % kBgSlices] = part[(r - begin) % kBgSlices] + term(r);
  for (int q = 1; q < kBgSlices; ++q) part[0] = part[0] + part[q];
  return part[0];
}

// exp and log in plain arithmetic: the same bits on the host and on the device.  |error| < 2^-50 relative on the ranges used
// (exp: x <= 0 after the row's maximum is taken off; log: a sum in [1, 32]).
BD_HD double bg_pow2(int n) { return __builtin_bit_cast(double, (unsigned long long)(n + 1023) << 52); }
BD_HD double bg_exp(double x) {
  if (x != x) return x;
  if (x < -745.0) return 0.0;
  if (x > 709.0) return INFINITY;
  const double kf = x * 1.4426950408889634;
  const int n = (int)(kf + (kf < 0.0 ? -0.5 : 0.5));
  const double r = (x - n * 0.693147180369123816490e+00) - n * 1.90821492927058770002e-10;
  double p = 1.0;
  for (int k = 13; k >= 1; --k) p = 1.0 + r * p / (double)k;
  return n < -1000 ? p * bg_pow2(n + 100) * bg_pow2(-100) : p * bg_pow2(n);
}
BD_HD double bg_log(double s) {
  if (!(s > 0.0) || s == INFINITY) return s != s ? s : (s == INFINITY ? s : (s == 0.0 ? -INFINITY : NAN));
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, s);
  int e = (int)((bits >> 52) & 0x7ff) - 1023;
  double m = __builtin_bit_cast(double, (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
  if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
  const double f = (m - 1.0) / (m + 1.0), f2 = f * f;
  double q = 1.0 / 23.0;
  for (int k = 21; k >= 1; k -= 2) q = q * f2 + 1.0 / (double)k;
  return e * 0.693147180369123816490e+00 + (2.0 * f * q + e * 1.90821492927058770002e-10);
}

BD_HD float bg_mix(float old, float v, float scale_old, float scale_new) {
  return scale_old == 0.0f ? scale_new * v : scale_old * old + scale_new * v;
}
BD_HD int bg_label(int y, int C) { return (y >= 0 && y < C) ? y : 0; }
// the sum of entry e of [dW_L | db_L] into its place
BD_HD void bg_head_store(int e, int nh, int C, double tot, float scale_old, float scale_new, float* dW, float* db) {
  float* out = e < nh * C ? dW + e : db + (e - nh * C);
  *out = bg_mix(*out, (float)tot, scale_old, scale_new);
}

// dgamma and dbeta of a column from the sums of es and et
BD_HD void bg_bn_grads(double sum_s, double sum_t, float mmean, float mvar, double& dgamma, double& dbeta) {
  const double rstd = 1.0 / sqrt((double)mvar + (double)kBnEps);
  dgamma = (sum_s - (double)mmean * sum_t) * rstd;
  dbeta = sum_t;
}
// column j of a hidden layer from its three sums: db, and (dgamma != null) dgamma and dbeta
BD_HD void bg_column_store(int j, double sum_b, double sum_s, double sum_t, const float* mmean, const float* mvar, float scale_old,
                           float scale_new, float* db, float* dgamma, float* dbeta) {
  db[j] = bg_mix(db[j], (float)sum_b, scale_old, scale_new);
  if (dgamma) {
    double dg, dbe;
    bg_bn_grads(sum_s, sum_t, mmean[j], mvar[j], dg, dbe);
    dgamma[j] = bg_mix(dgamma[j], (float)dg, scale_old, scale_new);
    dbeta[j] = bg_mix(dbeta[j], (float)dbe, scale_old, scale_new);
  }
}

// the u of a row's class from its margins; margin2 (CROWN-IBP training): the mixed margin (1 - beta) margin + beta margin2
BD_HD double bg_u(const float* margin, const float* margin2, float beta, size_t at) {
  if (!margin2) return -(double)margin[at];
  return -((1.0 - (double)beta) * (double)margin[at] + (double)beta * (double)margin2[at]);
}

}  // namespace lipasr
