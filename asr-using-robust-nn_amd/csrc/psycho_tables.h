// Host tables of the psychoacoustic masker (psycho.hip), float64: bin frequencies, their Bark values, the absolute threshold of
// hearing in dB and the per-masker level shift, for a 2048-point window at any sample rate (include/lipasr.h has the equations).
#pragma once
#include <cmath>
#include <limits>
#include <vector>

namespace lipasr {
namespace psycho {

constexpr int kWin = 2048, kHopP = 512, kBins = 1025;
constexpr int kMaxMaskers = 512;  // strict local maxima among bins 1 .. 1023 (every odd bin at the most)

inline double bin_hz(int k, int sr) { return (double)k * (double)sr / (double)kWin; }

inline double bark_of(double f) {
  const double r = f / 7500.0;
  return 13.0 * std::atan(0.00076 * f) + 3.5 * std::atan(r * r);
}

// -inf outside [20 Hz, 20 kHz]
inline double ath_db(double f) {
  if (!(f >= 20.0 && f <= 20000.0)) return -std::numeric_limits<double>::infinity();
  const double q = f / 1000.0, d = q - 3.3;
  return 3.64 * std::pow(q, -0.8) - 6.5 * std::exp(-0.6 * (d * d)) + 0.001 * (q * q * q * q) - 12.0;
}

// which: 0 f, 1 bark, 2 ATH (dB), 3 shift
inline std::vector<double> table(int which, int sr) {
  std::vector<double> v(kBins);
  for (int k = 0; k < kBins; ++k) {
    const double f = bin_hz(k, sr);
    switch (which) {
      case 0: v[k] = f; break;
      case 1: v[k] = bark_of(f); break;
      case 2: v[k] = ath_db(f); break;
      default: v[k] = -6.025 - 0.275 * bark_of(f); break;
    }
  }
  return v;
}

}  // namespace psycho
}  // namespace lipasr
