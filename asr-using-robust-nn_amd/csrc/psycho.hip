// Psychoacoustic masking threshold of a clip and the hinge loss of a perturbation against it, with its gradient to the samples
// (the imperceptible audio attack's second stage).  Window 2048, hop 512, periodic Hann, no padding: frame t is
// x[512 t .. 512 t + 2048), T = 1 + (n - 2048) / 512, 1025 bins.  include/lipasr.h has the equations.
// Kernels:
//   psy_psd_kernel         one workgroup per (clip, group of 8 frames).  Frames go in pairs through ONE complex FFT (fft_pass of
//                          stft.h: frame a + i frame b, separated by conjugate symmetry); un-normalised dB [B][T][1025] and the
//                          group's maximum.
//   psy_psd_finish_kernel  one workgroup per (clip, frame): the clip maximum from the group maxima, psd = 96 - max + p in place.
//   psy_threshold_kernel   one workgroup per (clip, frame): strict local maxima, their three-bin levels and the comparison with the
//                          absolute threshold of hearing in parallel (an ordered compaction through a prefix sum), the greedy merge
//                          within half a Bark on ONE lane in the order the rule is stated in, then for every bin the sum over the
//                          surviving maskers, ascending.  Every list holds 512 entries, the most there can be.
//   psy_loss_grad_kernel   one workgroup per (clip, group of 8 frames), built like stft_vjp_kernel without the reflection: forward
//                          FFT of w . delta for a frame pair, P = c |X|^2, the hinge against theta, Z = G X sent through the same
//                          four passes on conjugated data, windowed overlap-add into the group's LDS image (11 hops).  A pair with
//                          no bin over theta skips the inverse transform; a frame with none stays out of the image.
//   psy_fold_kernel        adds the (at most two) images that cover a sample, and the loss partials of a clip in ascending order.
//   psy_step_kernel        delta <- clamp(delta - lr s(g_net + alpha_u g_theta), +-eps_u), x_adv = clamp(x0 + delta), delta = x_adv - x0.
// Every sum runs in a fixed order, there are no atomics, and a clip's result does not depend on the batch it is launched in.
#include "common.h"
#include "psycho_tables.h"
#include "stft.h"
#include <memory>

namespace lipasr {

using namespace psycho;

constexpr int kPsFrames = 8;                       // frames per workgroup (even: they go through the FFT in pairs)
constexpr int kPsSpan = kPsFrames * kHopP;         // samples between two groups
constexpr int kPsSeg = (kPsFrames + 3) * kHopP;    // samples the frames of one group cover

struct PsyPlan {
  lipasr_ctx* ctx = nullptr;
  int sample_rate = 0, n_max = 0, batch_max = 0, frames_max = 0, groups_max = 0, by_position = 0;
  float* d_hann = nullptr;     // [2048]
  float* d_tw = nullptr;       // float2 [2048]
  double* d_bark = nullptr;    // [1025]
  float* d_ath_db = nullptr;   // [1025] (-inf outside 20 Hz .. 20 kHz)
  float* d_ath_lin = nullptr;  // [1025] 10^(ATH/10), 0 where ATH is -inf
  float* d_shift = nullptr;    // [1025]
  float* d_psd = nullptr;      // [batch_max][frames_max][1025] (lipasr_psy_prepare)
  float* d_gmax = nullptr;     // [batch_max][groups_max]
  float* d_part = nullptr;     // [batch_max][groups_max][kPsSeg]
  float* d_lpart = nullptr;    // [batch_max][groups_max]
};

void psy_plan_free(PsyPlan* p) {
  if (!p) return;
  void* ptrs[] = {p->d_hann, p->d_tw, p->d_bark, p->d_ath_db, p->d_ath_lin, p->d_shift, p->d_psd, p->d_gmax, p->d_part, p->d_lpart};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  delete p;
}

__device__ __forceinline__ float psy_block_max(float v, float* red, int tid) {
  v = wave_max(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// the windowed frame pair (f0, f0 + 1) of one row through the four Stockham passes; buf then holds FFT(frame a + i frame b)
__device__ __forceinline__ void psy_pair_fft(float2* buf, const float* __restrict__ row, int f0, bool has1, const float* __restrict__ hann,
                                             const float2* __restrict__ tw, int tid) {
  cpx x0[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int j = f0 * kHopP + tid + 256 * e;
    const float w = hann[tid + 256 * e];
    const float s0 = row[j], s1 = has1 ? row[j + kHopP] : 0.0f;
    x0[e] = {w * s0, w * s1};
  }
  fft_pass<8, 1>(buf, 1, tid, tw, x0);
  __syncthreads();
  fft_pass<8, 1>(buf, 8, tid, tw);
  __syncthreads();
  fft_pass<8, 1>(buf, 64, tid, tw);
  __syncthreads();
  fft_pass<4, 2>(buf, 512, tid, tw);
  __syncthreads();
}

// Xa[k] = (Z[k] + conj Z[N-k]) / 2, Xb[k] = (Z[k] - conj Z[N-k]) / (2 i)
__device__ __forceinline__ void psy_split(float2 z, float2 zc, float* xar, float* xai, float* xbr, float* xbi) {
  const float zr = z.x, zi = z.y, wr = zc.x, wi = -zc.y;
  *xar = 0.5f * (zr + wr); *xai = 0.5f * (zi + wi);
  *xbr = 0.5f * (zi - wi); *xbi = -0.5f * (zr - wr);
}

// ---------------------------------------------------------------------------------------------
// PSD
// ---------------------------------------------------------------------------------------------
constexpr float kPsdScale = (float)((8.0 / 3.0) / ((double)kWin * (double)kWin));  // |sqrt(8/3) X / N|^2 = kPsdScale |X|^2

__device__ __forceinline__ float psy_db(float re, float im) { return fmaxf(-200.0f, 10.0f * log10f((re * re + im * im) * kPsdScale)); }

__global__ __launch_bounds__(256) void psy_psd_kernel(const float* __restrict__ x, int n, int T, int n_groups, const float* __restrict__ hann,
                                                       const float2* __restrict__ tw, float* __restrict__ psd, float* __restrict__ gmax) {
  __shared__ __attribute__((aligned(16))) float2 buf[kFftLds];
  __shared__ float red[4];
  const int tid = threadIdx.x, g = blockIdx.x, u = blockIdx.y;
  const int f_begin = g * kPsFrames, f_end = min(f_begin + kPsFrames, T);
  const float* xu = x + (size_t)u * n;
  float mx = -200.0f;
  for (int f0 = f_begin; f0 < f_end; f0 += 2) {
    const bool has1 = f0 + 1 < f_end;
    __syncthreads();  // the previous pair's reads of buf are done
    psy_pair_fft(buf, xu, f0, has1, hann, tw, tid);
    float* pa = psd + ((size_t)u * T + f0) * kBins;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tid + 256 * i;
      if (k <= 1024) {
        float xar, xai, xbr, xbi;
        psy_split(buf[padi(k)], buf[padi((2048 - k) & 2047)], &xar, &xai, &xbr, &xbi);
        const float da = psy_db(xar, xai);
        pa[k] = da;
        mx = fmaxf(mx, da);
        if (has1) {
          const float db = psy_db(xbr, xbi);
          pa[kBins + k] = db;
          mx = fmaxf(mx, db);
        }
      }
    }
  }
  mx = psy_block_max(mx, red, tid);
  if (tid == 0) gmax[(size_t)u * n_groups + g] = mx;
}

__global__ __launch_bounds__(256) void psy_psd_finish_kernel(float* __restrict__ psd, const float* __restrict__ gmax, int T, int n_groups,
                                                              float* __restrict__ psd_max) {
  const int tid = threadIdx.x, t = blockIdx.x, u = blockIdx.y;
  float mx = gmax[(size_t)u * n_groups];
  for (int g = 1; g < n_groups; ++g) mx = fmaxf(mx, gmax[(size_t)u * n_groups + g]);
  const float off = 96.0f - mx;
  float* p = psd + ((size_t)u * T + t) * kBins;
  for (int k = tid; k < kBins; k += 256) p[k] = off + p[k];
  if (t == 0 && tid == 0) psd_max[u] = mx;
}

// ---------------------------------------------------------------------------------------------
// masking threshold of one frame
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void psy_threshold_kernel(const float* __restrict__ psd, int T, const double* __restrict__ bark,
                                                             const float* __restrict__ ath_db, const float* __restrict__ ath_lin,
                                                             const float* __restrict__ shift, int by_position, float* __restrict__ theta,
                                                             int* __restrict__ n_maskers) {
  __shared__ float v[kBins + 3];
  __shared__ int mb[kMaxMaskers];        // candidates that passed the ATH filter, ascending: bin, level
  __shared__ float ml[kMaxMaskers];
  __shared__ unsigned char dropped[kMaxMaskers];
  __shared__ double sz[kMaxMaskers];     // survivors: Bark of the bin, level + shift, upper slope
  __shared__ float sbase[kMaxMaskers];
  __shared__ float sslope[kMaxMaskers];
  __shared__ int wtot[4];
  __shared__ int counts[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = blockIdx.x, u = blockIdx.y;
  const float* pv = psd + ((size_t)u * T + t) * kBins;
  for (int k = tid; k < kBins; k += 256) v[k] = pv[k];
  for (int i = tid; i < kMaxMaskers; i += 256) dropped[i] = 0;
  __syncthreads();
  // candidates of bins 4 tid + 1 .. 4 tid + 4 (<= 1023): at most two of four neighbours are strict local maxima
  int cb[4];
  float cl[4];
  int c = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * tid + 1 + e;
    if (k <= 1023) {
      const float a = v[k - 1], b = v[k], d = v[k + 1];
      if (b > a && b > d) {
        const float level = 10.0f * log10f(exp10f(0.1f * a) + exp10f(0.1f * b) + exp10f(0.1f * d));
        if (level > ath_db[k]) { cb[c] = k; cl[c] = level; ++c; }
      }
    }
  }
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int base = incl - c;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  for (int e = 0; e < c; ++e) { mb[base + e] = cb[e]; ml[base + e] = cl[e]; }
  __syncthreads();
  if (tid == 0) {
    const int nc = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    // the greedy merge, literally: the pair closer than half a Bark loses its smaller member; when that is i_prev, i_prev moves on
    // by ONE entry (not to i).  by_position indexes the Bark table with the list position instead of the masker's bin.
    int ip = 0;
    for (int i = 1; i < nc; ++i) {
      const double bi = by_position ? bark[i] : bark[mb[i]];
      const double bp = by_position ? bark[ip] : bark[mb[ip]];
      if (bi - bp < 0.5) {
        if (ml[ip] < ml[i]) { dropped[ip] = 1; ip = ip + 1; }
        else dropped[i] = 1;
      } else {
        ip = i;
      }
    }
    int ns = 0;
    for (int i = 0; i < nc; ++i) {
      if (dropped[i]) continue;
      const int k = mb[i];
      const float level = ml[i];
      sz[ns] = bark[k];
      sbase[ns] = level + shift[k];
      sslope[ns] = -27.0f + 0.37f * fmaxf(level - 40.0f, 0.0f);
      ++ns;
    }
    counts[0] = ns;
    if (n_maskers) n_maskers[(size_t)u * T + t] = ns;
  }
  __syncthreads();
  const int ns = counts[0];
  float* th = theta + ((size_t)u * T + t) * kBins;
  for (int k = tid; k < kBins; k += 256) {
    const double bk = bark[k];
    float acc = ath_lin[k];
    for (int j = 0; j < ns; ++j) {
      const float dz = (float)(bk - sz[j]);  // the difference of two nearby Bark values, rounded once
      const float sf = dz <= 0.0f ? 27.0f * dz : sslope[j] * dz;
      acc += exp10f(0.1f * (sbase[j] + sf));
    }
    th[k] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// hinge loss against the threshold and its gradient: one frame group
// ---------------------------------------------------------------------------------------------
// (no occupancy attribute: held to three waves per SIMD as stft_vjp_kernel is, the kernel spills 86 registers; a stage-2 batch of 64
// one-second clips is 320 workgroups, one or two per CU, so the third resident workgroup would have nothing to run)
__global__ __launch_bounds__(256) void psy_loss_grad_kernel(const float* __restrict__ delta, int n, int T, int n_groups, const float* __restrict__ hann,
                          const float2* __restrict__ tw, const float* __restrict__ theta, const float* __restrict__ psd_max,
                          int need_grad, float* __restrict__ part, float* __restrict__ lpart) {
  __shared__ __attribute__((aligned(16))) float2 buf[kFftLds];
  __shared__ float ola[kPsSeg];
  __shared__ float red[4];
  const int tid = threadIdx.x, g = blockIdx.x, u = blockIdx.y;
  const int f_begin = g * kPsFrames, f_end = min(f_begin + kPsFrames, T);
  const float* du = delta + (size_t)u * n;
  // c = 10^9.6 / 10^(psd_max / 10) (8/3) / N^2, formed in double and rounded once; G = c / (K T) where P > theta
  const double cd = pow(10.0, 9.6 - 0.1 * (double)psd_max[u]) * ((8.0 / 3.0) / ((double)kWin * (double)kWin));
  const float c = (float)cd, cg = (float)(cd / ((double)kBins * (double)T));
  if (need_grad)
    for (int i = tid; i < kPsSeg; i += 256) ola[i] = 0.0f;
  float lsum = 0.0f;
  for (int f0 = f_begin; f0 < f_end; f0 += 2) {
    const bool has1 = f0 + 1 < f_end;
    __syncthreads();  // the previous pair's reads of buf (and the zeroing of ola) are done
    psy_pair_fft(buf, du, f0, has1, hann, tw, tid);
    float2 zz[5], zc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tid + 256 * i;
      if (k <= 1024) {
        zz[i] = buf[padi(k)];
        zc[i] = buf[padi((2048 - k) & 2047)];
      }
    }
    const float* tha = theta + ((size_t)u * T + f0) * kBins;
    float xr[5][2], xi[5][2];
    bool oa[5], ob[5];
    bool any_a = false, any_b = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tid + 256 * i;
      oa[i] = ob[i] = false;
      if (k <= 1024) {
        psy_split(zz[i], zc[i], &xr[i][0], &xi[i][0], &xr[i][1], &xi[i][1]);
        const float pa = c * (xr[i][0] * xr[i][0] + xi[i][0] * xi[i][0]);
        const float ta = tha[k];
        if (pa > ta) { oa[i] = true; any_a = true; lsum += pa - ta; }
        if (has1) {  // (without a second frame the imaginary half is the rounding residue of the first: not a frame)
          const float pb = c * (xr[i][1] * xr[i][1] + xi[i][1] * xi[i][1]);
          const float tb = tha[kBins + k];
          if (pb > tb) { ob[i] = true; any_b = true; lsum += pb - tb; }
        }
      }
    }
    // (both barriers also end every thread's reads of buf)
    const int nz_a = __syncthreads_or(any_a);
    const int nz_b = __syncthreads_or(any_b);
    if (!need_grad || (!nz_a && !nz_b)) continue;  // (workgroup-uniform) nothing over the threshold: the gradient is exactly 0
    // A = Ga Xa, B = Gb Xb; W[k] = A + i B, W[N-k] = conj A + i conj B; the buffer takes conj W
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tid + 256 * i;
      if (k <= 1024) {
        const float ga = oa[i] ? cg : 0.0f, gb = ob[i] ? cg : 0.0f;
        const float ar = ga * xr[i][0], ai = ga * xi[i][0], br = gb * xr[i][1], bi = gb * xi[i][1];
        if (k == 0 || k == 1024) {
          buf[padi(k)] = make_float2(2.0f * ar, -2.0f * br);  // real bins: Re Z whole
        } else {
          buf[padi(k)] = make_float2(ar - bi, -(ai + br));
          buf[padi(2048 - k)] = make_float2(ar + bi, ai - br);
        }
      }
    }
    __syncthreads();
    fft_pass<8, 1>(buf, 1, tid, tw);
    __syncthreads();
    fft_pass<8, 1>(buf, 8, tid, tw);
    __syncthreads();
    fft_pass<8, 1>(buf, 64, tid, tw);
    __syncthreads();
    fft_pass<4, 2>(buf, 512, tid, tw);
    __syncthreads();
    // DFT(conj W) = frame-a gradient - i frame-b gradient
    float2 r[8];
    float hn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      r[e] = buf[padi(tid + 256 * e)];
      hn[e] = hann[tid + 256 * e];
    }
    float* o = ola + (f0 - f_begin) * kHopP + tid;
    if (nz_a) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[256 * e] += hn[e] * r[e].x;
    }
    __syncthreads();  // frame b lands 512 samples later: other threads' positions
    if (nz_b) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[kHopP + 256 * e] -= hn[e] * r[e].y;
    }
  }
  lsum = wave_sum(lsum);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = lsum;
  __syncthreads();
  if (tid == 0) lpart[(size_t)u * n_groups + g] = (red[0] + red[1]) + (red[2] + red[3]);
  if (need_grad) {
    float* pg = part + ((size_t)u * n_groups + g) * kPsSeg;
    for (int i = tid; i < kPsSeg; i += 256) pg[i] = ola[i];
  }
}

// g_delta[i] = the images of the (at most two) groups that cover sample i, the earlier group first; samples past the last frame
// lie in the zeroed tail of the last image or past every image: exactly 0.  Workgroup 0 of a clip also sums its loss partials.
__global__ __launch_bounds__(256) void psy_fold_kernel(const float* __restrict__ part, const float* __restrict__ lpart, int n_groups, int n,
                                                        int T, float* __restrict__ gd, float* __restrict__ loss) {
  const int u = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.0f;
    for (int g = 0; g < n_groups; ++g) s += lpart[(size_t)u * n_groups + g];
    loss[u] = s / (float)(kBins * T);
  }
  if (!gd || i >= n) return;
  const float* P = part + (size_t)u * n_groups * kPsSeg;
  const int g1 = i / kPsSpan, r = i - g1 * kPsSpan;
  float s = 0.0f;
  if (g1 >= 1 && g1 - 1 < n_groups && r < kPsSeg - kPsSpan) s = P[(size_t)(g1 - 1) * kPsSeg + kPsSpan + r];
  if (g1 < n_groups) s += P[(size_t)g1 * kPsSeg + r];
  gd[(size_t)u * n + i] = s;
}

// ---------------------------------------------------------------------------------------------
// the attack's step
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void psy_step_kernel(float* __restrict__ delta, float* __restrict__ x_adv, const float* __restrict__ x0,
                                                        const float* __restrict__ g_net, const float* __restrict__ g_theta,
                                                        const float* __restrict__ alpha, const float* __restrict__ eps, int n, float lr,
                                                        int use_sign, float lo, float hi) {
  const int u = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t o = (size_t)u * n + i;
  float t = g_net[o];
  if (g_theta) t += alpha[u] * g_theta[o];
  if (use_sign) t = (t > 0.0f) ? 1.0f : ((t < 0.0f) ? -1.0f : 0.0f);
  const float e = eps[u];
  const float d = fminf(fmaxf(delta[o] - lr * t, -e), e);
  const float xa = fminf(fmaxf(x0[o] + d, lo), hi);
  x_adv[o] = xa;
  delta[o] = xa - x0[o];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <typename T>
static int psy_upload(T** dst, const std::vector<T>& src) {
  if (hipMalloc(dst, src.size() * sizeof(T)) != hipSuccess) { set_error("lipasr_psy_create: table allocation failed"); return LIPASR_ENOMEM; }
  LP_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return LIPASR_OK;
}

static int psy_frames(int n) { return 1 + (n - kWin) / kHopP; }
static int psy_groups(int T) { return (T + kPsFrames - 1) / kPsFrames; }

static int psy_check(const char* fn, const PsyPlan* p, int n, int batch) {
  LP_CHECK_ARG(p != nullptr, "%s: null plan", fn);
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "%s: batch %d outside [1, %d]", fn, batch, p->batch_max);
  LP_CHECK_ARG(n >= kWin && n <= p->n_max, "%s: n=%d outside [%d, %d] (one whole window at least, the plan's n_max at most)", fn, n, kWin,
               p->n_max);
  return LIPASR_OK;
}

static int launch_psd(const PsyPlan* p, const float* x, int n, int batch, float* psd, float* psd_max, hipStream_t st) {
  const int T = psy_frames(n), G = psy_groups(T);
  hipLaunchKernelGGL(psy_psd_kernel, dim3(G, batch), dim3(256), 0, st, x, n, T, G, p->d_hann, reinterpret_cast<const float2*>(p->d_tw), psd,
                     p->d_gmax);
  LP_LAUNCH_CHECK();
  hipLaunchKernelGGL(psy_psd_finish_kernel, dim3(T, batch), dim3(256), 0, st, psd, p->d_gmax, T, G, psd_max);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

static int launch_threshold(const PsyPlan* p, const float* psd, int T, int batch, float* theta, int* n_maskers, hipStream_t st) {
  hipLaunchKernelGGL(psy_threshold_kernel, dim3(T, batch), dim3(256), 0, st, psd, T, p->d_bark, p->d_ath_db, p->d_ath_lin, p->d_shift,
                     p->by_position, theta, n_maskers);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

// opaque plan type of the C ABI
struct lipasr_psy : lipasr::PsyPlan {};

extern "C" {

int lipasr_psy_create(lipasr_handle_t h, int sample_rate, int n_max, int batch_max, int flags, lipasr_psy_t* out) {
  LP_CHECK_ARG(out != nullptr, "lipasr_psy_create: out is null");
  LP_CHECK_ARG(sample_rate >= 1, "lipasr_psy_create: sample_rate=%d", sample_rate);
  LP_CHECK_ARG((flags & ~1) == 0, "lipasr_psy_create: flags=%d (bit 0: bark by position)", flags);
  LP_CHECK_ARG(n_max >= kWin && batch_max >= 1, "lipasr_psy_create: n_max=%d (one window of %d samples at least) batch_max=%d", n_max, kWin,
               batch_max);
  const int T = psy_frames(n_max), G = psy_groups(T);
  if ((double)batch_max * T * kBins >= 2147483647.0) {
    set_error("lipasr_psy_create: batch_max=%d x %d frames x %d bins does not fit 31 bits", batch_max, T, kBins);
    return LIPASR_EUNSUPPORTED;
  }
  LP_CHECK_ARG(h != nullptr, "lipasr_psy_create: null handle");
  DeviceGuard g(h->device);
  std::unique_ptr<PsyPlan, void (*)(PsyPlan*)> guard(new lipasr_psy(), psy_plan_free);
  PsyPlan* p = guard.get();
  p->ctx = h;
  p->sample_rate = sample_rate; p->n_max = n_max; p->batch_max = batch_max; p->frames_max = T; p->groups_max = G;
  p->by_position = flags & 1;
  const std::vector<double> bark = table(1, sample_rate), ath = table(2, sample_rate), shift = table(3, sample_rate);
  std::vector<float> ath_db(kBins), ath_lin(kBins), shift_f(shift.begin(), shift.end());
  for (int k = 0; k < kBins; ++k) {
    ath_db[k] = (float)ath[k];
    ath_lin[k] = std::isinf(ath[k]) ? 0.0f : (float)std::pow(10.0, ath[k] / 10.0);
  }
  int rc;
  if ((rc = psy_upload(&p->d_hann, tables::hann_periodic())) != LIPASR_OK || (rc = psy_upload(&p->d_tw, tables::twiddles())) != LIPASR_OK ||
      (rc = psy_upload(&p->d_bark, bark)) != LIPASR_OK || (rc = psy_upload(&p->d_ath_db, ath_db)) != LIPASR_OK ||
      (rc = psy_upload(&p->d_ath_lin, ath_lin)) != LIPASR_OK || (rc = psy_upload(&p->d_shift, shift_f)) != LIPASR_OK)
    return rc;
  if (hipMalloc(&p->d_psd, (size_t)batch_max * T * kBins * sizeof(float)) != hipSuccess ||
      hipMalloc(&p->d_gmax, (size_t)batch_max * G * sizeof(float)) != hipSuccess ||
      hipMalloc(&p->d_part, (size_t)batch_max * G * kPsSeg * sizeof(float)) != hipSuccess ||
      hipMalloc(&p->d_lpart, (size_t)batch_max * G * sizeof(float)) != hipSuccess) {
    set_error("lipasr_psy_create: workspace allocation failed");
    return LIPASR_ENOMEM;
  }
  h->psy_plans.push_back(p);
  *out = static_cast<lipasr_psy*>(guard.release());
  return LIPASR_OK;
}

int lipasr_psy_destroy(lipasr_psy_t p) {
  LP_CHECK_ARG(p != nullptr, "lipasr_psy_destroy: null plan");
  if (p->ctx) {
    DeviceGuard g(p->ctx->device);
    std::vector<PsyPlan*>& v = p->ctx->psy_plans;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == p) { v.erase(v.begin() + i); break; }
  }
  psy_plan_free(p);
  return LIPASR_OK;
}

int lipasr_psy_psd(lipasr_psy_t p, const float* x, int n, int batch, float* psd, float* psd_max, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr, "lipasr_psy_psd: null plan");
  LP_CHECK_ARG(x != nullptr && psd != nullptr && psd_max != nullptr, "lipasr_psy_psd: null array");
  int rc = psy_check("lipasr_psy_psd", p, n, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  return launch_psd(p, x, n, batch, psd, psd_max, S(stream));
}

int lipasr_psy_threshold(lipasr_psy_t p, const float* psd, int n_frames, int batch, float* theta, int* n_maskers, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr, "lipasr_psy_threshold: null plan");
  LP_CHECK_ARG(psd != nullptr && theta != nullptr, "lipasr_psy_threshold: null array");
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "lipasr_psy_threshold: batch %d outside [1, %d]", batch, p->batch_max);
  LP_CHECK_ARG(n_frames >= 1 && n_frames <= p->frames_max, "lipasr_psy_threshold: n_frames %d outside [1, %d]", n_frames, p->frames_max);
  DeviceGuard g(p->ctx->device);
  return launch_threshold(p, psd, n_frames, batch, theta, n_maskers, S(stream));
}

int lipasr_psy_prepare(lipasr_psy_t p, const float* x, int n, int batch, float* theta, float* psd_max, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr, "lipasr_psy_prepare: null plan");
  LP_CHECK_ARG(x != nullptr && theta != nullptr && psd_max != nullptr, "lipasr_psy_prepare: null array");
  int rc = psy_check("lipasr_psy_prepare", p, n, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  if ((rc = launch_psd(p, x, n, batch, p->d_psd, psd_max, S(stream))) != LIPASR_OK) return rc;
  return launch_threshold(p, p->d_psd, psy_frames(n), batch, theta, nullptr, S(stream));
}

int lipasr_psy_loss_grad(lipasr_psy_t p, const float* delta, int n, int batch, const float* theta, const float* psd_max, float* loss,
                         float* g_delta, lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr, "lipasr_psy_loss_grad: null plan");
  LP_CHECK_ARG(delta != nullptr && theta != nullptr && psd_max != nullptr && loss != nullptr, "lipasr_psy_loss_grad: null array");
  int rc = psy_check("lipasr_psy_loss_grad", p, n, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  hipStream_t st = S(stream);
  const int T = psy_frames(n), G = psy_groups(T);
  hipLaunchKernelGGL(psy_loss_grad_kernel, dim3(G, batch), dim3(256), 0, st, delta, n, T, G, p->d_hann, reinterpret_cast<const float2*>(p->d_tw),
                     theta, psd_max, g_delta ? 1 : 0, p->d_part, p->d_lpart);
  LP_LAUNCH_CHECK();
  hipLaunchKernelGGL(psy_fold_kernel, dim3(g_delta ? (n + 255) / 256 : 1, batch), dim3(256), 0, st, p->d_part, p->d_lpart, G, n, T, g_delta,
                     loss);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_psy_step(lipasr_psy_t p, float* delta, float* x_adv, const float* x0, const float* g_net, const float* g_theta,
                    const float* alpha, const float* eps, int n, int batch, float lr, int use_sign, float clip_lo, float clip_hi,
                    lipasr_stream_t stream) {
  LP_CHECK_ARG(p != nullptr, "lipasr_psy_step: null plan");
  LP_CHECK_ARG(delta != nullptr && x_adv != nullptr && x0 != nullptr && g_net != nullptr && eps != nullptr, "lipasr_psy_step: null array");
  LP_CHECK_ARG(g_theta == nullptr || alpha != nullptr, "lipasr_psy_step: g_theta without alpha");
  LP_CHECK_ARG(n >= 1 && batch >= 1, "lipasr_psy_step: n=%d batch=%d", n, batch);
  LP_CHECK_ARG(clip_lo <= clip_hi, "lipasr_psy_step: clip range [%g, %g]", clip_lo, clip_hi);
  DeviceGuard g(p->ctx->device);
  hipLaunchKernelGGL(psy_step_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, S(stream), delta, x_adv, x0, g_net, g_theta, alpha, eps, n,
                     lr, use_sign, clip_lo, clip_hi);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_psy_table(int which, int sample_rate, double* out, int cap) {
  LP_CHECK_ARG(sample_rate >= 1, "lipasr_psy_table: sample_rate=%d", sample_rate);
  LP_CHECK_ARG(which >= 0 && which <= 3, "lipasr_psy_table: unknown table %d", which);
  const std::vector<double> v = table(which, sample_rate);
  if (out) {
    LP_CHECK_ARG((size_t)cap >= v.size(), "lipasr_psy_table: capacity %d < %zu", cap, v.size());
    memcpy(out, v.data(), v.size() * sizeof(double));
  }
  return (int)v.size();
}

}  // extern "C"
