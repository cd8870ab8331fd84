// K1 backward: vector-Jacobian product of the 2048/512 MFCC stage (gfx950), g_feat [20 L] -> g_y [n_y] -> g_x [n_samp].
//
// The forward (include/lipasr.h, K1) leaves the pre-floor dB tile and the per-frame maxima in the plan; the kernels here
// walk it backwards, every sum in a fixed order (no floating-point atomics: two runs give the same bits):
//   1. mfcc_vjp_db_kernel     one workgroup per clip: Gc = g / scale, Gdbc = D^T Gc, the top_db mask, the sum of the floored
//                             elements handed to the clip maximum (first maximum in (frame, mel) order), Gmel = Gdb (10/ln 10)/mel
//                             with mel = 10^(dB/10) recomputed from the stored dB.
//   2. stft_vjp_kernel        one workgroup per (clip, group of 8 frames).  Frames go in pairs through ONE complex FFT as in
//                             stft_mel_kernel (frame a + i frame b, separated by conjugate symmetry); Z = 2 GP X of both frames
//                             is made Hermitian (H[k] = Z[k]/2, H[N-k] = conj Z[k]/2, the real bins 0 and N/2 whole), packed
//                             again as Ha + i Hb and sent through the SAME four Stockham passes on conjugated data, which
//                             returns the two real frame gradients in the real and (negated) imaginary part.  They are
//                             windowed and overlap-added into an LDS image of the group's 11 hops, frames in ascending order;
//                             frames with an all-zero cotangent are skipped (their gradient is exactly 0).
//   3. stft_vjp_fold_kernel   adds the (at most two) group images that cover a padded position and folds the two reflected
//                             flanks back: g_y[i] = gyp[i + 1024] + gyp[1024 - i] (1 <= i <= 1024) + gyp[1024 + 2 (n_y - 1) - i]
//                             (n_y - 1025 <= i <= n_y - 2).  Needs n_y > 2048 (one reflection per side).
//   4. resample_vjp_kernel    R^T as a polyphase filter of its own (`down` phases of ~176 taps over the outputs that reach a sample).
#include "common.h"
#include "mfcc_tables.h"
#include "stft.h"

namespace lipasr {

using namespace tables;

// ---------------------------------------------------------------------------------------------
// 1. DCT^T, top_db floor, dB -> mel
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float vj_gdbc(const float* __restrict__ Ds, const float* __restrict__ gcs, int Tc, int t, int m) {
  float gd = 0.0f;
  if (t < Tc) {
#pragma unroll
    for (int k = 0; k < kNMfcc; ++k) gd = fmaf(Ds[k * kNMels + m], gcs[k * Tc + t], gd);
  }
  return gd;
}

// d dB / d mel = (10 / ln 10) / mel, mel = 10^(dB/10); amin = 1e-10 pins dB at -100 (no gradient)
__device__ __forceinline__ float vj_db_to_mel(float gdb, float d) {
  return (d > -100.0f) ? gdb * (4.3429448190325175f * exp10f(-0.1f * d)) : 0.0f;
}

__global__ __launch_bounds__(256) void mfcc_vjp_db_kernel(MfccVjpArgs a) {
  extern __shared__ float gcs[];  // [20][Tc]
  __shared__ float Ds[kNMfcc * kNMels];
  __shared__ float redf[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
  const int T = a.n_frames, L = a.L, Tc = min(T, L);
  for (int i = tid; i < kNMfcc * kNMels; i += 256) Ds[i] = a.dct_rows[i];
  for (int i = tid; i < kNMfcc * Tc; i += 256) {
    const int k = i / Tc, t = i - k * Tc, o = k * L + t;
    const float g = a.g_feat[(size_t)u * kNMfcc * L + o];
    gcs[i] = a.aff_scale ? (float)((double)g / a.aff_scale[o]) : g;
  }
  float mx = -INFINITY;
  for (int t = tid; t < T; t += 256) mx = fmaxf(mx, a.fmax[(size_t)u * T + t]);
  mx = wave_max(mx);
  if (lane == 0) redf[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  const float thr = mx - 80.0f;  // top_db = 80, as dct_kernel forms it
  __syncthreads();
  const float* dbu = a.db + (size_t)u * T * kNMels;
  float* gm = a.gmel + (size_t)u * T * kNMels;
  const int n = T * kNMels;
  float fsum = 0.0f;
  int amin = n;
  for (int i = tid; i < n; i += 256) {
    const int t = i >> 7, m = i & 127;
    const float d = dbu[i];
    const float gd = vj_gdbc(Ds, gcs, Tc, t, m);
    float gdb = gd;
    if (!(d > thr)) { fsum += gd; gdb = 0.0f; }
    if (d == mx) amin = min(amin, i);
    gm[i] = vj_db_to_mel(gdb, d);
  }
  fsum = wave_sum(fsum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amin = min(amin, __shfl_xor(amin, o, 64));
  if (lane == 0) { redf[wave] = fsum; redi[wave] = amin; }
  __syncthreads();
  fsum = (redf[0] + redf[1]) + (redf[2] + redf[3]);
  amin = min(min(redi[0], redi[1]), min(redi[2], redi[3]));
  // the floor moves with the clip maximum: that element also receives what the floored ones lost.  Its owner rewrites it.
  if (amin < n && (amin & 255) == tid) {
    const float d = dbu[amin];
    const float gd = vj_gdbc(Ds, gcs, Tc, amin >> 7, amin & 127);
    gm[amin] = vj_db_to_mel(gd + fsum, d);
  }
}

// ---------------------------------------------------------------------------------------------
// 2. mel^T, |X|^2, STFT^T, overlap-add of one frame group
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void stft_vjp_kernel(MfccVjpArgs a) {
  __shared__ __attribute__((aligned(16))) float2 buf[kFftLds];
  __shared__ float ola[kVjSeg];
  __shared__ float gms[2][kNMels];
  const int tid = threadIdx.x, g = blockIdx.x, u = blockIdx.y;
  const int T = a.n_frames;
  const int f_begin = g * kVjFrames, f_end = min(f_begin + kVjFrames, T);
  const float* yu = a.y + (size_t)u * a.n_y;
  for (int i = tid; i < kVjSeg; i += 256) ola[i] = 0.0f;
  // (the Hann and mel constants are re-read where they are used, from L1 / L2: held across the pairs they cost 31 registers
  // and the third workgroup of a CU)
  for (int f0 = f_begin; f0 < f_end; f0 += 2) {
    const bool has1 = f0 + 1 < f_end;
    __syncthreads();  // the previous pair's reads of buf / gms (and the zeroing of ola) are done
    // A frame whose cotangent is all zero (frames >= L away from the clip maximum) has an exactly zero gradient: it is kept out
    // of the image, so that the rounding residue of its partner in the packed transform (the imaginary part of a "real"
    // inverse is ~1e-7 of the real part, not 0) does not land on samples whose true gradient is 0 -- sign(g) would step there.
    int nz_a, nz_b;
    {
      const int sel = tid >> 7, m = tid & 127, f = f0 + sel;
      const float v = (f < f_end) ? a.gmel[((size_t)u * T + f) * kNMels + m] : 0.0f;
      gms[sel][m] = v;
      nz_a = __syncthreads_or(sel == 0 && v != 0.0f);
      nz_b = __syncthreads_or(sel == 1 && v != 0.0f);
    }
    if (!nz_a && !nz_b) continue;  // (workgroup-uniform)
    cpx x0[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j0 = f0 * 512 + tid + 256 * e - 1024;
      const float s0 = yu[reflect_index(j0, a.n_y)];
      const float s1 = has1 ? yu[reflect_index(j0 + 512, a.n_y)] : 0.0f;
      const float w = a.hann[tid + 256 * e];
      x0[e] = {w * s0, w * s1};
    }
    fft_pass<8, 1>(buf, 1, tid, a.tw, x0);
    __syncthreads();
    fft_pass<8, 1>(buf, 8, tid, a.tw);
    __syncthreads();
    fft_pass<8, 1>(buf, 64, tid, a.tw);
    __syncthreads();
    fft_pass<4, 2>(buf, 512, tid, a.tw);
    __syncthreads();
    // Z = FFT(frame a + i frame b): Xa[k] = (Z[k] + conj Z[N-k])/2, Xb[k] = (Z[k] - conj Z[N-k])/(2i)
    float2 zz[5], zc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tid + 256 * i;
      if (k <= 1024) {
        zz[i] = buf[padi(k)];
        zc[i] = buf[padi((2048 - k) & 2047)];
      }
    }
    __syncthreads();
    // A = GPa Xa, B = GPb Xb (= Z/2 of each frame); W[k] = A + i B, W[N-k] = conj A + i conj B; the buffer takes conj W
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tid + 256 * i;
      if (k <= 1024) {
        const float zr = zz[i].x, zi = zz[i].y, wr = zc[i].x, wi = -zc[i].y;
        const float xar = 0.5f * (zr + wr), xai = 0.5f * (zi + wi);
        const float xbr = 0.5f * (zi - wi), xbi = -0.5f * (zr - wr);
        const int m = a.bin_run[k], m1 = min(m + 1, kNMels - 1);
        const float l1 = a.mel_wlo[k], h1 = (m + 1 < kNMels) ? a.mel_whi[k] : 0.0f;
        const float ga = l1 * gms[0][m] + h1 * gms[0][m1];
        const float gb = l1 * gms[1][m] + h1 * gms[1][m1];
        const float ar = ga * xar, ai = ga * xai, br = gb * xbr, bi = gb * xbi;
        if (k == 0 || k == 1024) {
          buf[padi(k)] = make_float2(2.0f * ar, -2.0f * br);  // real bins: Re Z whole
        } else {
          buf[padi(k)] = make_float2(ar - bi, -(ai + br));
          buf[padi(2048 - k)] = make_float2(ar + bi, ai - br);
        }
      }
    }
    __syncthreads();
    fft_pass<8, 1>(buf, 1, tid, a.tw);
    __syncthreads();
    fft_pass<8, 1>(buf, 8, tid, a.tw);
    __syncthreads();
    fft_pass<8, 1>(buf, 64, tid, a.tw);
    __syncthreads();
    fft_pass<4, 2>(buf, 512, tid, a.tw);
    __syncthreads();
    // DFT(conj W) = conj(IDFT-sum of W) = frame-a gradient - i frame-b gradient
    float2 r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = buf[padi(tid + 256 * e)];
    float* o = ola + (f0 - f_begin) * 512 + tid;
    float hn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) hn[e] = a.hann[tid + 256 * e];
    if (nz_a) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[256 * e] += hn[e] * r[e].x;
    }
    __syncthreads();  // frame b lands 512 samples later: other threads' positions
    if (nz_b) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[512 + 256 * e] -= hn[e] * r[e].y;
    }
  }
  __syncthreads();
  float* pg = a.part + ((size_t)u * a.n_groups + g) * kVjSeg;
  for (int i = tid; i < kVjSeg; i += 256) pg[i] = ola[i];
}

// ---------------------------------------------------------------------------------------------
// 3. sum of the group images, adjoint of the reflect pad
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float vj_gyp(const float* __restrict__ P, int n_groups, int q) {
  constexpr int kSpan = 512 * kVjFrames;
  const int g1 = q / kSpan, r = q - g1 * kSpan;
  float s = 0.0f;
  if (g1 >= 1 && g1 - 1 < n_groups && r < kVjSeg - kSpan) s = P[(size_t)(g1 - 1) * kVjSeg + kSpan + r];
  if (g1 < n_groups) s += P[(size_t)g1 * kVjSeg + r];
  return s;
}

__global__ __launch_bounds__(256) void stft_vjp_fold_kernel(const float* __restrict__ part, int n_groups, int n_y, float* __restrict__ gy) {
  const int u = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_y) return;
  const float* P = part + (size_t)u * n_groups * kVjSeg;
  float s = vj_gyp(P, n_groups, i + 1024);
  if (i >= 1 && i <= 1024) s += vj_gyp(P, n_groups, 1024 - i);
  if (i >= n_y - 1025 && i <= n_y - 2) s += vj_gyp(P, n_groups, 1024 + 2 * (n_y - 1) - i);
  gy[(size_t)u * n_y + i] = s;
}

// ---------------------------------------------------------------------------------------------
// 4. resampler adjoint
// ---------------------------------------------------------------------------------------------
// Output t = up q + p reads x[down q + noff[p] - (left - 1) + k], k < taps, and down q + noff[p] = floor(t down / up): sample
// j = down q' + r is reached by the run of outputs with  j + left - taps <= floor(t down / up) <= j + left - 1, and that run,
// relative to up q', depends on r alone.  So R^T is itself a polyphase filter with `down` phases,
//     gx[down q' + r] = sum_{i < nt} HT[i][r] gy[up q' + t0[r] + i],
// its taps HT (the forward taps re-indexed, zero-padded to the longest run nt ~ taps up / down) and first offsets t0 tabulated
// by the plan.  One workgroup = Q consecutive q' of one clip, one thread per phase r: the gy window sits in LDS (zeros outside
// [0, n_valid): the appended zero sample and the clip's ends give nothing), a tap is loaded once (coalesced over r) for Q fmas,
// ascending i = ascending t: a fixed order.
template <int Q>
__global__ __launch_bounds__(1024) void resample_vjp_kernel(const float* __restrict__ gy, int n_y, int n_valid, float* __restrict__ gx,
                                                             int n_samp, int up, int down, const float* __restrict__ HT,
                                                             const int* __restrict__ t0, int nt, int t0min, int win) {
  extern __shared__ float ws[];  // [win]: gy[up Q0 + t0min ...]
  const int u = blockIdx.y, Q0 = blockIdx.x * Q, tid = threadIdx.x;
  const int r = blockIdx.z * blockDim.x + tid;
  const float* gyu = gy + (size_t)u * n_y;
  const int base = up * Q0 + t0min;
  for (int i = tid; i < win; i += blockDim.x) {
    const int t = base + i;
    ws[i] = (t >= 0 && t < n_valid) ? gyu[t] : 0.0f;
  }
  __syncthreads();
  if (r >= down) return;
  const float* wp = ws + (t0[r] - t0min);
  float acc[Q];
#pragma unroll
  for (int qq = 0; qq < Q; ++qq) acc[qq] = 0.0f;
  for (int i = 0; i < nt; ++i) {
    const float h = HT[(size_t)i * down + r];
#pragma unroll
    for (int qq = 0; qq < Q; ++qq) acc[qq] = fmaf(h, wp[qq * up + i], acc[qq]);
  }
#pragma unroll
  for (int qq = 0; qq < Q; ++qq) {
    const int j = down * (Q0 + qq) + r;
    if (j < n_samp) gx[(size_t)u * n_samp + j] = acc[qq];
  }
}

__global__ __launch_bounds__(256) void copy_cut_kernel(const float* __restrict__ gy, int n_y, float* __restrict__ gx, int n_samp) {
  const int u = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j < n_samp) gx[(size_t)u * n_samp + j] = j < n_y ? gy[(size_t)u * n_y + j] : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int launch_mfcc_vjp(const MfccVjpArgs& a, hipStream_t st) {
  const int Tc = std::min(a.n_frames, a.L);
  const size_t lds = (size_t)kNMfcc * Tc * sizeof(float);
  if (lds > 40 * 1024) {
    set_error("lipasr_mfcc_plan_vjp: utterance_length %d with %d frames needs %zu bytes of LDS", a.L, a.n_frames, lds);
    return LIPASR_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(mfcc_vjp_db_kernel, dim3(a.batch), dim3(256), lds, st, a);
  LP_LAUNCH_CHECK();
  hipLaunchKernelGGL(stft_vjp_kernel, dim3(a.n_groups, a.batch), dim3(256), 0, st, a);
  LP_LAUNCH_CHECK();
  hipLaunchKernelGGL(stft_vjp_fold_kernel, dim3((a.n_y + 255) / 256, a.batch), dim3(256), 0, st, a.part, a.n_groups, a.n_y, a.gy);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int launch_resample_vjp(const ResampleVjpArgs& a, const float* gy, float* gx, int batch, hipStream_t st) {
  if (a.identity) {
    hipLaunchKernelGGL(copy_cut_kernel, dim3((a.n_samp + 255) / 256, batch), dim3(256), 0, st, gy, a.n_y, gx, a.n_samp);
    LP_LAUNCH_CHECK();
    return LIPASR_OK;
  }
  const int threads = std::min(1024, ((a.down + 63) / 64) * 64), zs = (a.down + threads - 1) / threads;
  const int nq = (a.n_samp + a.down - 1) / a.down;
  const int span = a.t0max - a.t0min + a.nt;  // window of one q'
  constexpr int kQ = 8;
  const size_t lds8 = (size_t)((kQ - 1) * a.up + span) * sizeof(float), lds1 = (size_t)span * sizeof(float);
  if (lds8 <= 60 * 1024) {
    hipLaunchKernelGGL(resample_vjp_kernel<kQ>, dim3((nq + kQ - 1) / kQ, batch, zs), dim3(threads), lds8, st, gy, a.n_y, a.n_valid, gx,
                       a.n_samp, a.up, a.down, a.ht, a.t0, a.nt, a.t0min, (int)(lds8 / sizeof(float)));
  } else if (lds1 <= 60 * 1024) {
    hipLaunchKernelGGL(resample_vjp_kernel<1>, dim3(nq, batch, zs), dim3(threads), lds1, st, gy, a.n_y, a.n_valid, gx, a.n_samp, a.up,
                       a.down, a.ht, a.t0, a.nt, a.t0min, span);
  } else {
    set_error("lipasr_mfcc_plan_resample_vjp: ratio %d/%d needs a %zu-byte window; unsupported", a.up, a.down, lds1);
    return LIPASR_EUNSUPPORTED;
  }
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr
