// DolphinAttack: a 16 kHz voice command as inaudible amplitude-modulated ultrasound at 192 kHz, and what a microphone with a
// quadratic non-linearity records from it.  The chain of one clip of n valid samples (include/lipasr.h has the equations):
//     band-pass (ten biquads) -> x12 interpolation -> peak 1 -> AM on the carrier -> peak 2 -> a1 s + a2 s^2 -> /12 decimation.
// Kernels:
//   dolphin_bandpass_kernel   one workgroup per clip, the sections one after the other; per section a chunked scan in fp64 over
//                             64-sample chunks held in LDS: zero-state run, serial carry of the 2-vector state with the tabulated
//                             M^64, re-run from the right state.  Clips longer than the LDS image go tile by tile with the state.
//   dolphin_peaks_kernel      one workgroup per clip: m1 = max|u| and then m2 = max|s'| with u recomputed (two passes over the
//                             clip, nothing but two floats written).  Maxima are exact in any order.
//   dolphin_generate_kernel   the ultrasound [batch][12 n_samp], one thread per slow sample (12 outputs, three 16-byte stores)
//   dolphin_record_kernel     any 192 kHz buffer -> non-linearity -> decimating FIR, the input tile in LDS by phase
//   dolphin_fused_kernel      voice tile -> ultrasound tile -> non-linearity -> decimation with the 192 kHz signal in LDS only
// generate / record / fused share gen12 and decimate4, so the fused path gives the bits of generate followed by record.
// Every sum runs in a fixed order, there are no atomics, and a clip's result does not depend on the batch it is launched in.
#include "common.h"
#include "dolphin_tables.h"
#include <memory>

namespace lipasr {

using namespace dolphin;

struct DolphinPlan {
  lipasr_ctx* ctx = nullptr;
  int n_samp = 0, batch_max = 0, carrier_hz = 0;
  float carrier_level = 0.0f;
  double* d_sos = nullptr;   // [kSections][8]: g, a1, a2, M^64 (4), 0
  float* d_hu = nullptr;     // [12][kPhaseStride] interpolator fragments
  float* d_hd = nullptr;     // [12][kPhaseStride] decimator fragments
  float* d_voice = nullptr;  // [batch_max][n_samp]
  float* d_peaks = nullptr;  // [batch_max][2]
};

void dolphin_plan_free(DolphinPlan* p) {
  if (!p) return;
  if (p->d_sos) (void)hipFree(p->d_sos);
  if (p->d_hu) (void)hipFree(p->d_hu);
  if (p->d_hd) (void)hipFree(p->d_hd);
  if (p->d_voice) (void)hipFree(p->d_voice);
  if (p->d_peaks) (void)hipFree(p->d_peaks);
  delete p;
}

// ---------------------------------------------------------------------------------------------
// band-pass
// ---------------------------------------------------------------------------------------------
constexpr int kBpThreads = 128;                  // one chunk per thread
constexpr int kBpTile = kBpThreads * kChunk;     // 8192 samples per LDS image
constexpr int kBpStride = kChunk + 1;            // doubles per chunk row: thread t's row starts 2 t banks on (ds_read_b64: no conflict)
constexpr size_t kBpLdsBytes = (size_t)(kBpThreads * kBpStride + 4 * kBpThreads + 2 * kSections) * sizeof(double);

__device__ __forceinline__ int clip_len(const int* __restrict__ nv, int u, int n_samp) {
  return nv ? min(max(nv[u], 0), n_samp) : n_samp;
}

__global__ __launch_bounds__(kBpThreads) void dolphin_bandpass_kernel(const float* __restrict__ x, const int* __restrict__ nv,
                                                                       int n_samp, const double* __restrict__ sos,
                                                                       float* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) double bp_lds[];
  double* xs = bp_lds;                                  // [kBpThreads][kBpStride] the tile, section after section in place
  double* zs = xs + kBpThreads * kBpStride;             // [kBpThreads][2] zero-state end state of every chunk
  double* is = zs + 2 * kBpThreads;                     // [kBpThreads][2] state every chunk starts from
  double* carry = is + 2 * kBpThreads;                  // [kSections][2] state at the start of the tile
  const int u = blockIdx.x, tid = threadIdx.x;
  const int n = clip_len(nv, u, n_samp);
  const float* xu = x + (size_t)u * n_samp;
  float* vu = v + (size_t)u * n_samp;
  if (tid < 2 * kSections) carry[tid] = 0.0;
  for (int t0 = 0; t0 < n_samp; t0 += kBpTile) {
    if (t0 >= n) {  // nothing of the clip is left: zeros to the end of the row
      for (int i = tid; i < kBpTile && t0 + i < n_samp; i += kBpThreads) vu[t0 + i] = 0.0f;
      continue;
    }
    for (int i = tid; i < kBpTile; i += kBpThreads) {
      const int j = t0 + i;
      xs[(i >> 6) * kBpStride + (i & 63)] = j < n ? (double)xu[j] : 0.0;
    }
    __syncthreads();
    double* row = xs + tid * kBpStride;
    const bool active = t0 + tid * kChunk < n;  // a chunk past the clip's end feeds nothing that is kept
    for (int s = 0; s < kSections; ++s) {
      const double g = sos[8 * s], na1 = -sos[8 * s + 1], na2 = -sos[8 * s + 2];
      double z0 = 0.0, z1 = 0.0;
      if (active) {
#pragma unroll 8
        for (int k = 0; k < kChunk; ++k) {
          const double xk = row[k];
          const double y = fma(g, xk, z0);
          z0 = fma(na1, y, z1);
          z1 = fma(na2, y, -g * xk);
        }
      }
      zs[2 * tid] = z0;
      zs[2 * tid + 1] = z1;
      __syncthreads();
      if (tid == 0) {
        const double m00 = sos[8 * s + 3], m01 = sos[8 * s + 4], m10 = sos[8 * s + 5], m11 = sos[8 * s + 6];
        double s0 = carry[2 * s], s1 = carry[2 * s + 1];
        for (int c = 0; c < kBpThreads; ++c) {
          is[2 * c] = s0;
          is[2 * c + 1] = s1;
          const double t0n = fma(m00, s0, fma(m01, s1, zs[2 * c]));
          const double t1n = fma(m10, s0, fma(m11, s1, zs[2 * c + 1]));
          s0 = t0n;
          s1 = t1n;
        }
        carry[2 * s] = s0;
        carry[2 * s + 1] = s1;
      }
      __syncthreads();
      if (active) {
        z0 = is[2 * tid];
        z1 = is[2 * tid + 1];
#pragma unroll 8
        for (int k = 0; k < kChunk; ++k) {
          const double xk = row[k];
          const double y = fma(g, xk, z0);
          z0 = fma(na1, y, z1);
          z1 = fma(na2, y, -g * xk);
          row[k] = y;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < kBpTile; i += kBpThreads) {
      const int j = t0 + i;
      if (j < n_samp) vu[j] = j < n ? (float)xs[(i >> 6) * kBpStride + (i & 63)] : 0.0f;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// interpolation + modulation of one slow sample; decimation of four
// ---------------------------------------------------------------------------------------------
// u[12 q + p], p < 12, from vw[0 .. 20] = v[q - 10 .. q + 10]
__device__ __forceinline__ void up12(const float* vw, const float* __restrict__ hu, float (&u)[kRatio]) {
  float w[kPhaseTaps];
#pragma unroll
  for (int i = 0; i < kPhaseTaps; ++i) w[i] = vw[i];
#pragma unroll
  for (int p = 0; p < kRatio; ++p) {
    float acc = 0.0f;
#pragma unroll
    for (int t = -10; t <= 10; ++t) acc = fmaf(hu[p * kPhaseStride + t + 10], w[10 - t], acc);
    u[p] = acc;
  }
}

// s'[12 q + p] = (u / m1 + c) cos(2 pi fc k / 192000), the phase reduced in integers
__device__ __forceinline__ void modulate12(float (&u)[kRatio], int q, int fc, float c, float m1) {
  const int base = kRatio * (int)(((unsigned long long)q * (unsigned)fc) % (unsigned)kSrIn);  // (12 q fc) mod 192000
#pragma unroll
  for (int p = 0; p < kRatio; ++p) {
    const int ph = (base + p * fc) % kSrOut;
    const float cs = cospif((float)ph * (1.0f / (float)(kSrOut / 2)));
    const float uh = m1 > 0.0f ? u[p] / m1 : 0.0f;
    u[p] = (uh + c) * cs;
  }
}

// the ultrasound s[12 q .. 12 q + 11]
__device__ __forceinline__ void gen12(const float* vw, const float* __restrict__ hu, int q, int fc, float c, float m1, float m2,
                                      float (&s)[kRatio]) {
  up12(vw, hu, s);
  modulate12(s, q, fc, c, m1);
#pragma unroll
  for (int p = 0; p < kRatio; ++p) s[p] = m2 > 0.0f ? s[p] / m2 : 0.0f;
}

__device__ __forceinline__ float mic(float s, float a1, float a2) { return s * fmaf(a2, s, a1); }

constexpr int kRecTile = 512;                   // recorded samples per workgroup
constexpr int kRecThreads = kRecTile / 4;       // four per thread
constexpr int kRecHalo = 12;                    // slow samples kept to the left of the tile (10 needed; 12 keeps 16-byte reads aligned)
constexpr int kRecW = kRecTile + 28;            // slow samples per phase row: positions 4 tid .. 4 tid + 27 are read

// r[i0 + 4 tid + j], j < 4, from ws[p][qq] = w[12 (i0 - kRecHalo + qq) + p]
__device__ __forceinline__ void decimate4(const float* ws, int tid, const float* __restrict__ hd, float (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = 0.0f;
#pragma unroll
  for (int p = 0; p < kRatio; ++p) {
    float win[28];
    const float4* src = reinterpret_cast<const float4*>(ws + p * kRecW + 4 * tid);
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      const float4 f = src[e];
      win[4 * e] = f.x; win[4 * e + 1] = f.y; win[4 * e + 2] = f.z; win[4 * e + 3] = f.w;
    }
#pragma unroll
    for (int t = -10; t <= 10; ++t) {
      const float tap = hd[p * kPhaseStride + t + 10];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(tap, win[j + t + kRecHalo], acc[j]);
    }
  }
}

__device__ __forceinline__ void store_rec(float* __restrict__ ru, int i, int n, int n_samp, const float (&acc)[4]) {
  if (i + 3 < n_samp && (n_samp & 3) == 0 && (reinterpret_cast<uintptr_t>(ru) & 15) == 0) {
    *reinterpret_cast<float4*>(ru + i) = make_float4(i < n ? acc[0] : 0.0f, i + 1 < n ? acc[1] : 0.0f, i + 2 < n ? acc[2] : 0.0f,
                                                     i + 3 < n ? acc[3] : 0.0f);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n_samp) ru[i + j] = i + j < n ? acc[j] : 0.0f;
  }
}

// ---------------------------------------------------------------------------------------------
// peaks
// ---------------------------------------------------------------------------------------------
constexpr int kPkThreads = 512, kPkTile = 2048;

__device__ __forceinline__ float block_max(float v, float* red, int tid) {
  v = wave_max(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float m = red[0];
  for (int w = 1; w < kPkThreads / 64; ++w) m = fmaxf(m, red[w]);
  return m;
}

__global__ __launch_bounds__(kPkThreads) void dolphin_peaks_kernel(const float* __restrict__ v, const int* __restrict__ nv, int n_samp,
                                                                    const float* __restrict__ hu, int fc, float c,
                                                                    float* __restrict__ peaks) {
  __shared__ float vs[kPkTile + 2 * 10 + 4];
  __shared__ float red[kPkThreads / 64];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int n = clip_len(nv, u, n_samp);
  const float* vu = v + (size_t)u * n_samp;
  float m1 = 0.0f, m2 = 0.0f;
  for (int pass = 0; pass < 2; ++pass) {
    float mx = 0.0f;
    for (int q0 = 0; q0 < n; q0 += kPkTile) {
      __syncthreads();
      for (int i = tid; i < kPkTile + 20; i += kPkThreads) {
        const int j = q0 - 10 + i;
        vs[i] = (j >= 0 && j < n) ? vu[j] : 0.0f;
      }
      __syncthreads();
      for (int qq = tid; qq < kPkTile && q0 + qq < n; qq += kPkThreads) {
        float s[kRatio];
        up12(vs + qq, hu, s);
        if (pass) modulate12(s, q0 + qq, fc, c, m1);
#pragma unroll
        for (int p = 0; p < kRatio; ++p) mx = fmaxf(mx, fabsf(s[p]));
      }
    }
    const float m = block_max(mx, red, tid);
    if (pass) m2 = m; else m1 = m;
  }
  if (tid == 0) {
    peaks[2 * u] = m1;
    peaks[2 * u + 1] = m2;
  }
}

// ---------------------------------------------------------------------------------------------
// generate
// ---------------------------------------------------------------------------------------------
constexpr int kGenThreads = 256, kGenTile = 1024;

__global__ __launch_bounds__(kGenThreads) void dolphin_generate_kernel(const float* __restrict__ v, const int* __restrict__ nv,
                                                                        int n_samp, const float* __restrict__ hu, int fc, float c,
                                                                        const float* __restrict__ peaks, float* __restrict__ out) {
  __shared__ float vs[kGenTile + 2 * 10 + 4];
  const int u = blockIdx.y, tid = threadIdx.x, q0 = blockIdx.x * kGenTile;
  const int n = clip_len(nv, u, n_samp);
  const float* vu = v + (size_t)u * n_samp;
  float* ou = out + (size_t)u * n_samp * kRatio;
  const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;  // a row is 48 n_samp bytes long
  if (q0 < n) {
    for (int i = tid; i < kGenTile + 20; i += kGenThreads) {
      const int j = q0 - 10 + i;
      vs[i] = (j >= 0 && j < n) ? vu[j] : 0.0f;
    }
  }
  __syncthreads();
  const float m1 = peaks[2 * u], m2 = peaks[2 * u + 1];
  for (int qq = tid; qq < kGenTile && q0 + qq < n_samp; qq += kGenThreads) {
    const int q = q0 + qq;
    float s[kRatio];
    if (q < n) {
      gen12(vs + qq, hu, q, fc, c, m1, m2, s);
    } else {
#pragma unroll
      for (int p = 0; p < kRatio; ++p) s[p] = 0.0f;
    }
    float* d = ou + (size_t)q * kRatio;
    if (vec) {
      float4* d4 = reinterpret_cast<float4*>(d);
      d4[0] = make_float4(s[0], s[1], s[2], s[3]);
      d4[1] = make_float4(s[4], s[5], s[6], s[7]);
      d4[2] = make_float4(s[8], s[9], s[10], s[11]);
    } else {
#pragma unroll
      for (int p = 0; p < kRatio; ++p) d[p] = s[p];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// record, and generate -> record in one kernel
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRecThreads) void dolphin_record_kernel(const float* __restrict__ ultra, const int* __restrict__ nv,
                                                                      int n_samp, const float* __restrict__ hd, float a1, float a2,
                                                                      float* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) float ws[kRatio * kRecW];
  const int u = blockIdx.y, tid = threadIdx.x, i0 = blockIdx.x * kRecTile;
  const int n = clip_len(nv, u, n_samp);
  const float* su = ultra + (size_t)u * n_samp * kRatio;
  float* ru = rec + (size_t)u * n_samp;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i0 < n) {  // (uniform over the workgroup)
    const bool vec = (reinterpret_cast<uintptr_t>(ultra) & 15) == 0;
    for (int qq = tid; qq < kRecW; qq += kRecThreads) {
      const int q = i0 - kRecHalo + qq;
      float s[kRatio];
#pragma unroll
      for (int p = 0; p < kRatio; ++p) s[p] = 0.0f;
      if (q >= 0 && q < n) {
        const float* sp = su + (size_t)q * kRatio;
        if (vec) {
          const float4* s4 = reinterpret_cast<const float4*>(sp);
          const float4 f0 = s4[0], f1 = s4[1], f2 = s4[2];
          s[0] = f0.x; s[1] = f0.y; s[2] = f0.z; s[3] = f0.w; s[4] = f1.x; s[5] = f1.y; s[6] = f1.z; s[7] = f1.w;
          s[8] = f2.x; s[9] = f2.y; s[10] = f2.z; s[11] = f2.w;
        } else {
#pragma unroll
          for (int p = 0; p < kRatio; ++p) s[p] = sp[p];
        }
      }
#pragma unroll
      for (int p = 0; p < kRatio; ++p) ws[p * kRecW + qq] = mic(s[p], a1, a2);
    }
    __syncthreads();
    decimate4(ws, tid, hd, acc);
  }
  store_rec(ru, i0 + 4 * tid, n, n_samp, acc);
}

__global__ __launch_bounds__(kRecThreads) void dolphin_fused_kernel(const float* __restrict__ v, const int* __restrict__ nv,
                                                                     int n_samp, const float* __restrict__ hu,
                                                                     const float* __restrict__ hd, int fc, float c,
                                                                     const float* __restrict__ peaks, float a1, float a2,
                                                                     float* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) float ws[kRatio * kRecW];
  __shared__ float vs[kRecW + 2 * 10 + 4];
  const int u = blockIdx.y, tid = threadIdx.x, i0 = blockIdx.x * kRecTile;
  const int n = clip_len(nv, u, n_samp);
  const float* vu = v + (size_t)u * n_samp;
  float* ru = rec + (size_t)u * n_samp;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i0 < n) {  // (uniform over the workgroup)
    const int qa = i0 - kRecHalo;
    for (int i = tid; i < kRecW + 20; i += kRecThreads) {
      const int j = qa - 10 + i;
      vs[i] = (j >= 0 && j < n) ? vu[j] : 0.0f;
    }
    __syncthreads();
    const float m1 = peaks[2 * u], m2 = peaks[2 * u + 1];
    for (int qq = tid; qq < kRecW; qq += kRecThreads) {
      const int q = qa + qq;
      float s[kRatio];
      if (q >= 0 && q < n) {
        gen12(vs + qq, hu, q, fc, c, m1, m2, s);
      } else {
#pragma unroll
        for (int p = 0; p < kRatio; ++p) s[p] = 0.0f;
      }
#pragma unroll
      for (int p = 0; p < kRatio; ++p) ws[p * kRecW + qq] = mic(s[p], a1, a2);
    }
    __syncthreads();
    decimate4(ws, tid, hd, acc);
  }
  store_rec(ru, i0 + 4 * tid, n, n_samp, acc);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <typename T>
static int dolphin_upload(T** dst, const std::vector<T>& src) {
  if (hipMalloc(dst, src.size() * sizeof(T)) != hipSuccess) { set_error("lipasr_dolphin_create: table allocation failed"); return LIPASR_ENOMEM; }
  LP_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return LIPASR_OK;
}

static int dolphin_check(const char* fn, const DolphinPlan* p, const void* in, const void* out, int batch) {
  LP_CHECK_ARG(p != nullptr, "%s: null plan", fn);
  LP_CHECK_ARG(in != nullptr && out != nullptr, "%s: null array", fn);
  LP_CHECK_ARG(batch >= 1 && batch <= p->batch_max, "%s: batch %d outside [1, %d]", fn, batch, p->batch_max);
  return LIPASR_OK;
}

static int launch_bandpass(const DolphinPlan* p, const float* wav, const int* nv, int batch, float* voice, hipStream_t st) {
  LP_DYN_LDS(dolphin_bandpass_kernel, kBpLdsBytes);
  hipLaunchKernelGGL(dolphin_bandpass_kernel, dim3(batch), dim3(kBpThreads), kBpLdsBytes, st, wav, nv, p->n_samp, p->d_sos, voice);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

static int launch_peaks(const DolphinPlan* p, const float* voice, const int* nv, int batch, hipStream_t st) {
  hipLaunchKernelGGL(dolphin_peaks_kernel, dim3(batch), dim3(kPkThreads), 0, st, voice, nv, p->n_samp, p->d_hu, p->carrier_hz,
                     p->carrier_level, p->d_peaks);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr

using namespace lipasr;

// opaque plan type of the C ABI
struct lipasr_dolphin : lipasr::DolphinPlan {};

extern "C" {

int lipasr_dolphin_create(lipasr_handle_t h, int sr_in, int n_samp_max, int batch_max, double carrier_hz, double carrier_level,
                          lipasr_dolphin_t* out) {
  LP_CHECK_ARG(out != nullptr, "lipasr_dolphin_create: out is null");
  if (sr_in != kSrIn) {
    set_error("lipasr_dolphin_create: sr_in=%d; the chain is built for %d Hz input (x%d to %d Hz)", sr_in, kSrIn, kRatio, kSrOut);
    return LIPASR_EUNSUPPORTED;
  }
  LP_CHECK_ARG(carrier_hz == std::floor(carrier_hz) && carrier_hz > 7000.0 && carrier_hz < 89000.0,
               "lipasr_dolphin_create: carrier_hz=%g is not an integer in (7000, 89000)", carrier_hz);
  LP_CHECK_ARG(carrier_level >= 0.0 && std::isfinite(carrier_level), "lipasr_dolphin_create: carrier_level=%g is negative", carrier_level);
  LP_CHECK_ARG(n_samp_max >= 1 && batch_max >= 1 && (double)n_samp_max * kRatio < 2147483647.0,
               "lipasr_dolphin_create: n_samp_max=%d batch_max=%d", n_samp_max, batch_max);
  LP_CHECK_ARG(h != nullptr, "lipasr_dolphin_create: null handle");
  DeviceGuard g(h->device);
  std::unique_ptr<DolphinPlan, void (*)(DolphinPlan*)> guard(new lipasr_dolphin(), dolphin_plan_free);
  DolphinPlan* p = guard.get();
  p->ctx = h;
  p->n_samp = n_samp_max; p->batch_max = batch_max;
  p->carrier_hz = (int)carrier_hz; p->carrier_level = (float)carrier_level;
  const Sos sos = butter_bandpass();
  std::vector<double> st((size_t)kSections * 8, 0.0);
  for (int s = 0; s < kSections; ++s) {
    st[8 * s] = sos.b[s][0]; st[8 * s + 1] = sos.a[s][1]; st[8 * s + 2] = sos.a[s][2];
    for (int e = 0; e < 4; ++e) st[8 * s + 3 + e] = sos.mp[s][e];
  }
  int rc;
  if ((rc = dolphin_upload(&p->d_sos, st)) != LIPASR_OK ||
      (rc = dolphin_upload(&p->d_hu, phase_fragments(resample_filter((double)kRatio), false))) != LIPASR_OK ||
      (rc = dolphin_upload(&p->d_hd, phase_fragments(resample_filter(1.0), true))) != LIPASR_OK)
    return rc;
  if (hipMalloc(&p->d_voice, (size_t)batch_max * n_samp_max * sizeof(float)) != hipSuccess ||
      hipMalloc(&p->d_peaks, (size_t)batch_max * 2 * sizeof(float)) != hipSuccess) {
    set_error("lipasr_dolphin_create: workspace allocation failed");
    return LIPASR_ENOMEM;
  }
  h->dolphin_plans.push_back(p);
  *out = static_cast<lipasr_dolphin*>(guard.release());
  return LIPASR_OK;
}

int lipasr_dolphin_destroy(lipasr_dolphin_t p) {
  LP_CHECK_ARG(p != nullptr, "lipasr_dolphin_destroy: null plan");
  if (p->ctx) {
    DeviceGuard g(p->ctx->device);
    std::vector<DolphinPlan*>& v = p->ctx->dolphin_plans;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i] == p) { v.erase(v.begin() + i); break; }
  }
  dolphin_plan_free(p);
  return LIPASR_OK;
}

int lipasr_dolphin_bandpass(lipasr_dolphin_t p, const float* wav, const int* n_valid, int batch, float* voice, lipasr_stream_t stream) {
  int rc = dolphin_check("lipasr_dolphin_bandpass", p, wav, voice, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  return launch_bandpass(p, wav, n_valid, batch, voice, S(stream));
}

int lipasr_dolphin_generate(lipasr_dolphin_t p, const float* wav, const int* n_valid, int batch, float* ultrasound, float* peaks,
                            lipasr_stream_t stream) {
  int rc = dolphin_check("lipasr_dolphin_generate", p, wav, ultrasound, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  hipStream_t st = S(stream);
  if ((rc = launch_bandpass(p, wav, n_valid, batch, p->d_voice, st)) != LIPASR_OK || (rc = launch_peaks(p, p->d_voice, n_valid, batch, st)) != LIPASR_OK)
    return rc;
  hipLaunchKernelGGL(dolphin_generate_kernel, dim3((p->n_samp + kGenTile - 1) / kGenTile, batch), dim3(kGenThreads), 0, st, p->d_voice,
                     n_valid, p->n_samp, p->d_hu, p->carrier_hz, p->carrier_level, p->d_peaks, ultrasound);
  LP_LAUNCH_CHECK();
  if (peaks) LP_HIP(hipMemcpyAsync(peaks, p->d_peaks, (size_t)batch * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return LIPASR_OK;
}

int lipasr_dolphin_record(lipasr_dolphin_t p, const float* ultrasound, const int* n_valid, int batch, float a1, float a2, float* rec,
                          lipasr_stream_t stream) {
  int rc = dolphin_check("lipasr_dolphin_record", p, ultrasound, rec, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  hipLaunchKernelGGL(dolphin_record_kernel, dim3((p->n_samp + kRecTile - 1) / kRecTile, batch), dim3(kRecThreads), 0, S(stream),
                     ultrasound, n_valid, p->n_samp, p->d_hd, a1, a2, rec);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_dolphin_generate_recorded(lipasr_dolphin_t p, const float* wav, const int* n_valid, int batch, float a1, float a2, float* rec,
                                     lipasr_stream_t stream) {
  int rc = dolphin_check("lipasr_dolphin_generate_recorded", p, wav, rec, batch);
  if (rc != LIPASR_OK) return rc;
  DeviceGuard g(p->ctx->device);
  hipStream_t st = S(stream);
  if ((rc = launch_bandpass(p, wav, n_valid, batch, p->d_voice, st)) != LIPASR_OK || (rc = launch_peaks(p, p->d_voice, n_valid, batch, st)) != LIPASR_OK)
    return rc;
  hipLaunchKernelGGL(dolphin_fused_kernel, dim3((p->n_samp + kRecTile - 1) / kRecTile, batch), dim3(kRecThreads), 0, st, p->d_voice,
                     n_valid, p->n_samp, p->d_hu, p->d_hd, p->carrier_hz, p->carrier_level, p->d_peaks, a1, a2, rec);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int lipasr_dolphin_table(int which, int sr_in, double* out, int cap) {
  if (sr_in != kSrIn) { set_error("lipasr_dolphin_table: sr_in=%d; the tables exist for %d Hz", sr_in, kSrIn); return LIPASR_EUNSUPPORTED; }
  std::vector<double> v;
  switch (which) {
    case 0: {
      const Sos s = butter_bandpass();
      for (int i = 0; i < kSections; ++i) {
        for (int e = 0; e < 3; ++e) v.push_back(s.b[i][e]);
        for (int e = 0; e < 3; ++e) v.push_back(s.a[i][e]);
      }
      break;
    }
    case 1: v = resample_filter((double)kRatio); break;
    case 2: v = resample_filter(1.0); break;
    case 3: {
      const Sos s = butter_bandpass();
      for (int i = 0; i < kSections; ++i)
        for (int e = 0; e < 4; ++e) v.push_back(s.mp[i][e]);
      break;
    }
    default: set_error("lipasr_dolphin_table: unknown table %d", which); return LIPASR_EINVAL;
  }
  if (out) {
    LP_CHECK_ARG((size_t)cap >= v.size(), "lipasr_dolphin_table: capacity %d < %zu", cap, v.size());
    memcpy(out, v.data(), v.size() * sizeof(double));
  }
  return (int)v.size();
}

}  // extern "C"
