// Host-side constant tables of the DolphinAttack chain (dolphin.hip), built in fp64 like mfcc_tables.h and fetched by the
// suite through lipasr_dolphin_table():
//   * the 100 Hz - 7 kHz Butterworth band-pass of order 10 as ten second-order sections (analogue prototype, band-pass
//     transform, bilinear transform; poles paired by conjugates, the gain spread evenly over the sections), with each
//     section's state-transition matrix to the power of the scan's chunk length;
//   * MATLAB resample's default anti-aliasing filter for a ratio of 12 (firls by its normal equations, times a Kaiser window),
//     scaled once for the interpolator (sum 12) and once for the decimator (sum 1), and both as polyphase fragments.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

namespace lipasr {
namespace dolphin {

constexpr int kSections = 10;     // Butterworth order 10, band-pass: 20 poles
constexpr int kChunk = 64;        // samples per chunk of the band-pass scan
constexpr int kRatio = 12;        // 192 kHz / 16 kHz
constexpr int kHalf = 10 * kRatio;        // MATLAB resample, n = 10: the filter reaches 10 slow samples to each side
constexpr int kTaps = 2 * kHalf + 1;      // 241
constexpr int kPhaseTaps = 21;            // taps of one polyphase branch: t = -10 .. 10
constexpr int kPhaseStride = 24;          // ... padded
constexpr int kSrIn = 16000, kSrOut = kSrIn * kRatio;
constexpr double kPi = 3.14159265358979323846;

struct Sos {
  double b[kSections][3];   // g, 0, -g
  double a[kSections][3];   // 1, a1, a2
  double mp[kSections][4];  // M^kChunk, M = [[-a1, 1], [-a2, 0]]: the zero-input map of the transposed direct form II state
  double pole_max = 0.0;
};

// scipy.signal.butter(10, [2 f_lo / fs, 2 f_hi / fs], "bandpass", output="sos") up to section order and gain split
inline Sos butter_bandpass(double f_lo = 100.0, double f_hi = 7000.0, double fs = 16000.0) {
  typedef std::complex<double> cd;
  const int N = kSections;
  // pre-warped edges for a bilinear transform at sampling rate 2 (fs2 = 4)
  const double w1 = 4.0 * std::tan(kPi * (2.0 * f_lo / fs) / 2.0), w2 = 4.0 * std::tan(kPi * (2.0 * f_hi / fs) / 2.0);
  const double bw = w2 - w1, wo = std::sqrt(w1 * w2);
  std::vector<cd> pz;  // digital poles with positive imaginary part: one per section
  cd den(1.0, 0.0);    // prod (fs2 - p) over all 20 analogue poles
  for (int k = 0; k < N; ++k) {
    const double th = kPi * (2.0 * k + N + 1) / (2.0 * N);
    const cd p_lp = cd(std::cos(th), std::sin(th)) * (bw / 2.0);
    const cd root = std::sqrt(p_lp * p_lp - wo * wo);
    for (int s = 0; s < 2; ++s) {
      const cd p = s ? p_lp - root : p_lp + root;
      den *= (4.0 - p);
      const cd z = (4.0 + p) / (4.0 - p);
      if (z.imag() > 0.0) pz.push_back(z);
    }
  }
  // gain: k_bp = bw^N; k_z = k_bp Re(prod(fs2 - zero) / prod(fs2 - pole)) with N analogue zeros at 0
  const double kz = std::pow(bw, N) * (std::pow(4.0, N) / den).real();
  const double g = std::pow(kz, 1.0 / N);
  // Section order.  The poles fall into a cluster at the lower band edge (near z = +1) and one at the upper edge (near z = -1),
  // five pairs each.  With a zero at +1 and one at -1 per section, a run of sections from ONE cluster is a chain of resonators
  // at nearly the same frequency whose gains multiply before the other cluster's sections take them back: measured in float64,
  // all-low-then-all-high (or any order by radius alone) loses nine digits on the impulse response (1e-6 of its peak).  So the
  // clusters alternate, low then high, each from its mildest pole to its sharpest: 2e-15 in float64, 1.3e-5 in float32.
  std::vector<cd> lo, hi;
  for (const cd& p : pz) (p.real() >= 0.0 ? lo : hi).push_back(p);
  const auto by_radius = [](const cd& x, const cd& y) { return std::abs(x) < std::abs(y); };
  std::sort(lo.begin(), lo.end(), by_radius);
  std::sort(hi.begin(), hi.end(), by_radius);
  for (size_t i = 0, k = 0; k < pz.size(); ++i) {
    if (i < lo.size()) pz[k++] = lo[i];
    if (i < hi.size()) pz[k++] = hi[i];
  }
  Sos s;
  for (int i = 0; i < N; ++i) {
    const cd p = pz[(size_t)i];
    s.b[i][0] = g; s.b[i][1] = 0.0; s.b[i][2] = -g;
    s.a[i][0] = 1.0; s.a[i][1] = -2.0 * p.real(); s.a[i][2] = std::norm(p);
    s.pole_max = std::max(s.pole_max, std::abs(p));
    double m[4] = {-s.a[i][1], 1.0, -s.a[i][2], 0.0};
    for (int sq = 1; sq < kChunk; sq *= 2) {
      const double r[4] = {m[0] * m[0] + m[1] * m[2], m[0] * m[1] + m[1] * m[3], m[2] * m[0] + m[3] * m[2], m[2] * m[1] + m[3] * m[3]};
      for (int e = 0; e < 4; ++e) m[e] = r[e];
    }
    for (int e = 0; e < 4; ++e) s.mp[i][e] = m[e];
  }
  return s;
}

inline double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x); }

// dense solve by Gaussian elimination with partial pivoting (A is n x n row-major, overwritten)
inline std::vector<double> solve_dense(std::vector<double> A, std::vector<double> b) {
  const int n = (int)b.size();
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(A[(size_t)r * n + c]) > std::fabs(A[(size_t)piv * n + c])) piv = r;
    if (piv != c) {
      for (int k = 0; k < n; ++k) std::swap(A[(size_t)c * n + k], A[(size_t)piv * n + k]);
      std::swap(b[c], b[piv]);
    }
    for (int r = c + 1; r < n; ++r) {
      const double f = A[(size_t)r * n + c] / A[(size_t)c * n + c];
      if (f == 0.0) continue;
      for (int k = c; k < n; ++k) A[(size_t)r * n + k] -= f * A[(size_t)c * n + k];
      b[r] -= f * b[c];
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double acc = b[r];
    for (int k = r + 1; k < n; ++k) acc -= A[(size_t)r * n + k] * b[k];
    b[r] = acc / A[(size_t)r * n + r];
  }
  return b;
}

// firls(numtaps - 1, [0 f1 f1 1], [1 1 0 0]) (type I, unit weights): minimise the integral of (A(f) - D(f))^2 over both bands
// for A(f) = sum_n a[n] cos(pi n f) through the normal equations Q a = b, Q = toeplitz(q) + hankel(q),
// q[n] = sum over bands of f sinc(f n) between the band's edges, b[n] = the same over the bands where D = 1.
inline std::vector<double> firls_lowpass(int numtaps, double f1) {
  const int M = (numtaps - 1) / 2;
  const double band[2][2] = {{0.0, f1}, {f1, 1.0}}, desired[2] = {1.0, 0.0};
  std::vector<double> q((size_t)numtaps), b((size_t)M + 1, 0.0);
  for (int n = 0; n < numtaps; ++n) {
    double acc = 0.0;
    for (int k = 0; k < 2; ++k) acc += band[k][1] * sinc(band[k][1] * n) - band[k][0] * sinc(band[k][0] * n);
    q[(size_t)n] = acc;
  }
  for (int n = 0; n <= M; ++n)
    for (int k = 0; k < 2; ++k) b[(size_t)n] += desired[k] * (band[k][1] * sinc(band[k][1] * n) - band[k][0] * sinc(band[k][0] * n));
  std::vector<double> Q((size_t)(M + 1) * (M + 1));
  for (int i = 0; i <= M; ++i)
    for (int j = 0; j <= M; ++j) Q[(size_t)i * (M + 1) + j] = q[(size_t)std::abs(i - j)] + q[(size_t)(i + j)];
  const std::vector<double> a = solve_dense(Q, b);
  std::vector<double> h((size_t)numtaps);
  for (int n = 1; n <= M; ++n) h[(size_t)(M + n)] = h[(size_t)(M - n)] = a[(size_t)n];
  h[(size_t)M] = 2.0 * a[0];
  return h;
}

// modified Bessel function I0 by its power series (x <= 5 here: 25 terms reach 1e-17)
inline double bessel_i0(double x) {
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 60; ++k) {
    term *= (x / (2.0 * k)) * (x / (2.0 * k));
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// MATLAB resample(x, P, Q) default filter for max(P, Q) = 12 (n = 10, beta = 5), scaled to sum `gain` (P)
inline std::vector<double> resample_filter(double gain) {
  const double fc = 1.0 / (2.0 * kRatio);
  std::vector<double> h = firls_lowpass(kTaps, 2.0 * fc);
  double sum = 0.0;
  for (int n = 0; n < kTaps; ++n) {
    const double r = (double)(n - kHalf) / kHalf;
    h[(size_t)n] *= bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(5.0);
    sum += h[(size_t)n];
  }
  for (double& v : h) v *= gain / sum;
  return h;
}

// polyphase fragments [12][kPhaseStride] (0 outside the filter), t = -10 .. 10:
//   interpolator (mirror = false): entry [p][t + 10] = h[120 + 12 t + p],  u[12 q + p] = sum_t frag[p][t + 10] v[q - t]
//   decimator    (mirror = true):  entry [p][t + 10] = h[120 - 12 t - p],  r[i] = sum_p sum_t frag[p][t + 10] w[12 (i + t) + p]
inline std::vector<float> phase_fragments(const std::vector<double>& h, bool mirror) {
  std::vector<float> f((size_t)kRatio * kPhaseStride, 0.0f);
  for (int p = 0; p < kRatio; ++p)
    for (int t = -10; t <= 10; ++t) {
      const int idx = mirror ? kHalf - kRatio * t - p : kHalf + kRatio * t + p;
      if (idx >= 0 && idx < kTaps) f[(size_t)p * kPhaseStride + t + 10] = (float)h[(size_t)idx];
    }
  return f;
}

}  // namespace dolphin
}  // namespace lipasr
