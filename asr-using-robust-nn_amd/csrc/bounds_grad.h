// What bounds_grad.hip and bounds_crown_grad.hip share: the column-sum slices, exp and log written out in + * /, the scale-and-mix
// of a gradient entry, the label guard and the BatchNorm gradients of a column.
#pragma once
#include "bounds.h"

// host and device must round alike
#pragma clang fp contract(off)

namespace lipasr {

// a column sum over the batch: a block takes kBgCols columns, thread slice s of a column the rows s, s + kBgSlices, ...  (8 x 32
// and not 32 x 8: at batch 1024 a slice is 32 dependent loads, not 128, and a 1024-wide layer is 128 blocks, not 32)
constexpr int kBgCols = 8;
constexpr int kBgSlices = kBdThreads / kBgCols;

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

// dgamma and dbeta of a column from the sums of es and et
BD_HD void bg_bn_grads(double sum_s, double sum_t, float mmean, float mvar, double& dgamma, double& dbeta) {
  const double rstd = 1.0 / sqrt((double)mvar + (double)kBnEps);
  dgamma = (sum_s - (double)mmean * sum_t) * rstd;
  dbeta = sum_t;
}


// the u of a row's class from its margins; margin2 (CROWN-IBP training): the mixed margin (1 - beta) margin + beta margin2
BD_HD double bg_u(const float* margin, const float* margin2, float beta, size_t at) {
  if (!margin2) return -(double)margin[at];
  return -((1.0 - (double)beta) * (double)margin[at] + (double)beta * (double)margin2[at]);
}

}  // namespace lipasr
