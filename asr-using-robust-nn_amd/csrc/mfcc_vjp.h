// K1 backward, the kernels: vector-Jacobian product of the 2048/512 MFCC stage (gfx950), g_feat [20 L] -> g_y [n_y] -> g_x [n_samp].
//
// The forward (include/lipasr.h, K1) leaves the pre-floor dB tile and the per-frame maxima in the plan; the kernels here
// walk it backwards, every sum in a fixed order (no floating-point atomics: two runs give the same bits):
//   1. mfcc_vjp_db_kernel     one workgroup per clip: Gc = g / scale, Gdbc = D^T Gc, the top_db mask, the sum of the floored
//                             elements handed to the clip maximum (first maximum in (frame, mel) order), Gmel = Gdb (10/ln 10)/mel
//                             with mel = 10^(dB/10) recomputed from the stored dB.
//   2. stft_vjp_kernel        one workgroup per (clip, group of 8 frames).  Frames go in pairs through ONE complex FFT as in
//                             stft_mel_kernel (frame a + i frame b, separated by conjugate symmetry), each frame first brought to
//                             a peak in [1, 2) by a power of two that its cotangent takes back; Z = 2 GP X of both frames
//                             is made Hermitian (H[k] = Z[k]/2, H[N-k] = conj Z[k]/2, the real bins 0 and N/2 whole), packed
//                             again as Ha + i Hb and sent through the SAME four Stockham passes on conjugated data, which
//                             returns the two real frame gradients in the real and (negated) imaginary part.  They are
//                             windowed and overlap-added into an LDS image of the group's 11 hops, frames in ascending order;
//                             frames with an all-zero cotangent are skipped (their gradient is exactly 0).
//   3. stft_vjp_fold_kernel   adds the (at most two) group images that cover a padded position and folds the two reflected
//                             flanks back: g_y[i] = gyp[i + 1024] + gyp[1024 - i] (1 <= i <= 1024) + gyp[1024 + 2 (n_y - 1) - i]
//                             (n_y - 1025 <= i <= n_y - 2) for n_y > 2048 (one reflection per side); a shorter clip (RAGGED only)
//                             sums every padded position that reflects onto i, in ascending order.
//   4. resample_vjp_kernel    R^T as a polyphase filter of its own (`down` phases of ~176 taps over the outputs that reach a sample).
//
// Every kernel has a RAGGED instance for clips of different lengths in one launch (lipasr_mfcc_plan_vjp_ragged): clip u then
// has its own n_vy = int(n r), n_y = ceil(n r) and frame count (clip_lengths, as the forward's kernels compute them), the
// plan's n_y / n_frames / group count are only the row strides, and everything past a clip's end is written as zero.  The
// non-RAGGED instances read no length array and compile to what they were without the parameter.
//
// The kernels are templates in this header because the two sets of instances live in two translation units: mfcc_vjp.hip
// instantiates and launches the ones for one length, mfcc_vjp_ragged.hip the RAGGED ones.  In ONE device module the mere presence
// of stft_vjp_kernel<true> changes the code the compiler emits for stft_vjp_kernel<false> (LDS addresses and register numbering
// move); apart, the one-length kernels are instruction for instruction what they were before the RAGGED parameter existed.
#pragma once
#include "common.h"
#include "mfcc_tables.h"
#include "stft.h"
#include <type_traits>

namespace lipasr {

using namespace tables;

// clip u's own lengths (RAGGED), cut to what the rows hold
__device__ __forceinline__ void vj_clip(const int* __restrict__ nv, int u, int n_samp_max, int sr_in, int frames_max, int* n_vy, int* n_y,
                                        int* n_frames) {
  clip_lengths(min(max(nv[u], 0), n_samp_max), sr_in, n_vy, n_y, n_frames);
  *n_frames = min(*n_frames, frames_max);
}

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

// d dB / d mel = (10 / ln 10) / mel, mel = 10^(dB/10); amin = 1e-10 pins dB at -100 (no gradient).  The exponent -d/10 is formed
// with its rounding made good: p = fl(-0.1f d) is off by up to half a unit of a number near 10 and 0.1f by 1.5e-8 of itself, and
// exp10 magnifies both by ln 10 |d| / 10 -- 22 units of the result at d = -95 (measured against float64).  e is the exact
// remainder of the product plus (0.1f - 0.1) d, and 10^(p + e) = 10^p (1 + ln 10 e) to second order in e < 1e-6.
__device__ __forceinline__ float vj_db_to_mel(float gdb, float d) {
  if (!(d > -100.0f)) return 0.0f;
  const float p = -0.1f * d;
  const float e = fmaf(-0.1f, d, -p) + 1.4901161e-9f * d;
  return gdb * (4.3429448190325175f * (exp10f(p) * fmaf(2.3025851f, e, 1.0f)));
}

// the power of two that brings a frame of peak m into [1, 2) (1 for a zero frame; frames below 2^-60 are pinned at -100 dB anyway)
__device__ __forceinline__ int vj_peak_exp(float m) { return m > 0.0f ? min(max(ilogbf(m), -60), 60) : 0; }

template <bool RAGGED>
using VjArgs = typename std::conditional<RAGGED, MfccVjpRaggedArgs, MfccVjpArgs>::type;

template <bool RAGGED>
__global__ __launch_bounds__(256) void mfcc_vjp_db_kernel(VjArgs<RAGGED> a) {
  extern __shared__ float gcs[];  // [20][Tc]
  __shared__ float Ds[kNMfcc * kNMels];
  __shared__ float redf[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
  // Ts: frames the rows of db / fmax / gmel are laid out for; T: frames of this clip (the maximum, the floor and the cotangent
  // stop there: what the arrays hold past it is stale, and nothing is written there)
  const int Ts = a.n_frames, L = a.L;
  int T = Ts;
  if constexpr (RAGGED) {
    int n_vy, n_y;
    vj_clip(a.n_valid, u, a.n_samp_max, a.sr_in, Ts, &n_vy, &n_y, &T);
  }
  const int Tc = min(T, L);
  for (int i = tid; i < kNMfcc * kNMels; i += 256) Ds[i] = a.dct_rows[i];
  for (int i = tid; i < kNMfcc * Tc; i += 256) {
    const int k = i / Tc, t = i - k * Tc, o = k * L + t;
    const float g = a.g_feat[(size_t)u * kNMfcc * L + o];
    gcs[i] = a.aff_scale ? (float)((double)g / a.aff_scale[o]) : g;
  }
  float mx = -INFINITY;
  for (int t = tid; t < T; t += 256) mx = fmaxf(mx, a.fmax[(size_t)u * Ts + t]);
  mx = wave_max(mx);
  if (lane == 0) redf[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
  const float thr = mx - 80.0f;  // top_db = 80, as dct_kernel forms it
  __syncthreads();
  const float* dbu = a.db + (size_t)u * Ts * kNMels;
  float* gm = a.gmel + (size_t)u * Ts * kNMels;
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
template <bool RAGGED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void stft_vjp_kernel(VjArgs<RAGGED> a) {
  __shared__ __attribute__((aligned(16))) float2 buf[kFftLds];
  __shared__ float ola[kVjSeg];
  __shared__ float gms[2][kNMels];
  __shared__ float pk[2][4];
  const int tid = threadIdx.x, g = blockIdx.x, u = blockIdx.y;
  const int Ts = a.n_frames;  // row stride of gmel
  int T = Ts, n_y = a.n_y, n_vy = a.n_y;
  if constexpr (RAGGED) vj_clip(a.n_valid, u, a.n_samp_max, a.sr_in, Ts, &n_vy, &n_y, &T);
  const int f_begin = g * kVjFrames, f_end = min(f_begin + kVjFrames, T);
  if constexpr (RAGGED) if (f_begin >= T) return;  // past this clip (workgroup-uniform, before any barrier): the fold does not read the image
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
      const float v = (f < f_end) ? a.gmel[((size_t)u * Ts + f) * kNMels + m] : 0.0f;
      gms[sel][m] = v;
      nz_a = __syncthreads_or(sel == 0 && v != 0.0f);
      nz_b = __syncthreads_or(sel == 1 && v != 0.0f);
    }
    if (!nz_a && !nz_b) continue;  // (workgroup-uniform)
    cpx x0[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j0 = f0 * 512 + tid + 256 * e - 1024;
      float s0, s1;
      if constexpr (RAGGED) {  // the clip's own reflection (repeated once n_y <= 1024); [n_vy, n_y) is fix_length's zero, as the forward reads it
        const int k0 = reflect_index(j0, n_y), k1 = reflect_index(j0 + 512, n_y);
        s0 = (k0 < n_vy) ? yu[k0] : 0.0f;
        s1 = (has1 && k1 < n_vy) ? yu[k1] : 0.0f;
      } else {
        s0 = yu[reflect_index(j0, a.n_y)];
        s1 = has1 ? yu[reflect_index(j0 + 512, a.n_y)] : 0.0f;
      }
      const float w = a.hann[tid + 256 * e];
      x0[e] = {w * s0, w * s1};
    }
    // The two frames share one transform, whose rounding error is 2^-24 of the LARGER of the two spectra: a quiet frame paired with
    // a loud one (it may lie 80 dB below it and still be above the floor) would take the loud frame's noise into its X, and its
    // cotangent ~ 1 / |X|^2 magnifies it (measured: g_y 73 x further from float64 than a float32 evaluation frame by frame).  Each
    // frame is brought to a peak in [1, 2) by a power of two before the transform -- exact -- and its cotangent takes the factor
    // back.  Frames of one binade keep the bits they had.
    float sca, scb;
    {
      float ma = 0.0f, mb = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { ma = fmaxf(ma, fabsf(x0[e].re)); mb = fmaxf(mb, fabsf(x0[e].im)); }
      ma = wave_max(ma);
      mb = wave_max(mb);
      if ((tid & 63) == 0) { pk[0][tid >> 6] = ma; pk[1][tid >> 6] = mb; }
      __syncthreads();
      const int ea = vj_peak_exp(fmaxf(fmaxf(pk[0][0], pk[0][1]), fmaxf(pk[0][2], pk[0][3])));
      const int eb = vj_peak_exp(fmaxf(fmaxf(pk[1][0], pk[1][1]), fmaxf(pk[1][2], pk[1][3])));
      const float na = ldexpf(1.0f, -ea), nb = ldexpf(1.0f, -eb);
#pragma unroll
      for (int e = 0; e < 8; ++e) { x0[e].re *= na; x0[e].im *= nb; }
      sca = ldexpf(1.0f, ea);
      scb = ldexpf(1.0f, eb);
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
        const float ga = (l1 * gms[0][m] + h1 * gms[0][m1]) * sca;
        const float gb = (l1 * gms[1][m] + h1 * gms[1][m1]) * scb;
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

// one reflection per side (n_y > 2048): the position itself, its image in the left flank, its image in the right flank
__device__ __forceinline__ float vj_fold3(const float* __restrict__ P, int n_groups, int n_y, int i) {
  float s = vj_gyp(P, n_groups, i + 1024);
  if (i >= 1 && i <= 1024) s += vj_gyp(P, n_groups, 1024 - i);
  if (i >= n_y - 1025 && i <= n_y - 2) s += vj_gyp(P, n_groups, 1024 + 2 * (n_y - 1) - i);
  return s;
}

// any n_y >= 2: np.pad's reflection has period 2 (n_y - 1), and position j = q - 1024 of the padded signal reads sample i when
// j = i or j = -i modulo the period.  The images are visited period by period, the two of a period in ascending order (they
// coincide for i = 0 and i = n_y - 1), so that the sum runs over ascending q.  n_y = 2: ~1000 terms, for two threads.
__device__ __forceinline__ float vj_fold_any(const float* __restrict__ P, int n_groups, int n_y, int i) {
  const int period = 2 * (n_y - 1), i2 = period - i;
  const bool twice = i > 0 && i < n_y - 1;
  const int j_end = n_y + 1024;  // padded positions q = j + 1024 in [0, n_y + 2048)
  float s = 0.0f;
  for (int base = -(1024 / period + 1) * period; base < j_end; base += period) {
    const int ja = base + i, jb = base + i2;
    if (ja >= -1024 && ja < j_end) s += vj_gyp(P, n_groups, ja + 1024);
    if (twice && jb >= -1024 && jb < j_end) s += vj_gyp(P, n_groups, jb + 1024);
  }
  return s;
}

// n_y: the row length of gy (and, without RAGGED, every clip's length); n_groups: the stride of the images per clip
template <bool RAGGED>
__global__ __launch_bounds__(256) void stft_vjp_fold_kernel(const float* __restrict__ part, int n_groups, int n_y, float* __restrict__ gy,
                                                             const int* __restrict__ nv, int n_samp_max, int sr_in, int frames_max) {
  const int u = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_y) return;
  const float* P = part + (size_t)u * n_groups * kVjSeg;
  if constexpr (!RAGGED) {
    gy[(size_t)u * n_y + i] = vj_fold3(P, n_groups, n_y, i);
    return;
  }
  int c_vy, c_y, c_frames;
  vj_clip(nv, u, n_samp_max, sr_in, frames_max, &c_vy, &c_y, &c_frames);
  const int c_groups = (c_frames + kVjFrames - 1) / kVjFrames;  // the images past it are stale
  float s = 0.0f;  // [c_y, n_y): not the clip's
  if (i < c_y && c_frames > 0) s = (c_y > kNFft) ? vj_fold3(P, c_groups, c_y, i) : vj_fold_any(P, c_groups, c_y, i);
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
// RAGGED: clip u has nv[u] samples; its window is cut at its own int(n r), gx is 0 from nv[u] on, and a workgroup that lies
// wholly past the clip writes its zeros and leaves.
struct VjNoClip {};
struct VjClip { const int* nv; int sr_in; };
template <int Q, bool RAGGED>
__global__ __launch_bounds__(1024) void resample_vjp_kernel(const float* __restrict__ gy, int n_y, int n_valid, float* __restrict__ gx,
                                                             int n_samp, int up, int down, const float* __restrict__ HT,
                                                             const int* __restrict__ t0, int nt, int t0min, int win,
                                                             typename std::conditional<RAGGED, VjClip, VjNoClip>::type clip) {
  extern __shared__ float ws[];  // [win]: gy[up Q0 + t0min ...]
  const int u = blockIdx.y, Q0 = blockIdx.x * Q, tid = threadIdx.x;
  const int r = blockIdx.z * blockDim.x + tid;
  int n_clip = n_samp;
  if constexpr (RAGGED) {
    int c_y, c_frames;
    n_clip = min(max(clip.nv[u], 0), n_samp);
    clip_lengths(n_clip, clip.sr_in, &n_valid, &c_y, &c_frames);
    if (down * Q0 >= n_clip) {  // (workgroup-uniform, before the barrier)
      if (r < down) {
#pragma unroll
        for (int qq = 0; qq < Q; ++qq) {
          const int j = down * (Q0 + qq) + r;
          if (j < n_samp) gx[(size_t)u * n_samp + j] = 0.0f;
        }
      }
      return;
    }
  }
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
    if (j < n_samp) gx[(size_t)u * n_samp + j] = (!RAGGED || j < n_clip) ? acc[qq] : 0.0f;
  }
}

// mfcc_vjp_ragged.hip (called by the launchers of mfcc_vjp.hip when there is a length array)
constexpr int kVjResampleQ = 8;  // outputs per thread of resample_vjp_kernel's main form
int launch_mfcc_vjp_ragged(const MfccVjpArgs& a, size_t lds, const int* n_valid, int sr_in, int n_samp_max, hipStream_t st);
int launch_resample_vjp_ragged(const ResampleVjpArgs& a, const float* gy, float* gx, dim3 grid, int threads, size_t lds, int win, bool q8,
                               hipStream_t st);

}  // namespace lipasr
