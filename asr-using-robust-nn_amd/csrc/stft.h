// Shared by the STFT kernels of K1 (stft_bdft.hip: the default block-DFT kernel on the matrix pipe; stft_mel.hip and mfcc_fused.hip:
// Stockham kernels; mfcc_vjp.hip: the backward pass).
#pragma once
#include "common.h"
#include "mfcc_tables.h"

namespace lipasr {

struct StftArgs {
  const float* y;  // [B][n_y]
  int n_y, n_frames;
  const float* hann;
  const float2* tw;
  const float* mel_wlo;  // [1025]
  const float* mel_whi;  // [1025]
  const int* mel_start;  // [128] run of bins whose lower filter is m
  const int* mel_len;
  float* db;    // [B][n_frames][128]
  float* fmax;  // [B][n_frames]
  int stage_mask;  // StageMask bits (mfcc_plan.h)
  // clips of different lengths in one launch (stft_mel2_kernel, stft_bdft_kernel): samples per clip, or null; n_y / n_frames
  // above are then the longest clip's (the strides of y, db, fmax) and every clip uses its own
  const int* n_valid;
  int sr_in, n_samp_max;
};

// per-clip lengths, the expressions of tables::resampled_lengths (librosa.load -> resampy int(n ratio), fix_length ceil)
__device__ __forceinline__ void clip_lengths(int n, int sr_in, int* n_vy, int* n_y, int* n_frames) {
  const double r = (double)tables::kSr / (double)sr_in;
  const double v = (double)n * r;
  *n_vy = (int)v;
  *n_y = (int)ceil(v);
  *n_frames = (*n_y >= 2) ? 1 + *n_y / tables::kHop : 0;
}

// librosa.power_to_db(ref=1, amin=1e-10) of one mel power.  A power at or below amin is EXACTLY -100 dB, as 10 log10 of the float32
// amin is in the reference; the device's log10f(1e-10f) is one unit in the last place off (-100.00001).
__device__ __forceinline__ float power_to_db(float p) { return p > 1e-10f ? 10.0f * log10f(p) : -100.0f; }

// np.pad(y, 1024, mode='reflect') index: position j relative to y[0], any j, n >= 2
__device__ __forceinline__ int reflect_index(int j, int n) {
  if ((unsigned)j < (unsigned)n) return j;  // interior frames never reflect
  const int period = 2 * (n - 1);
  int m = j % period;
  if (m < 0) m += period;
  return m < n ? m : period - m;
}

// the same for a clip longer than the padding (n > 2048 >= any |overshoot|): one reflection, no division
__device__ __forceinline__ int reflect_once(int j, int n) {
  const int lo = j < 0 ? -j : j;
  return lo < n ? lo : 2 * (n - 1) - lo;
}

// Workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every outstanding global access of the
// wave (vmcnt(0)) -- inside the frame loop that would expose the dB stores of the previous pair (a round trip to L2) at
// the next pair's first barrier, once per pair.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ void lds_barrier2() { lds_barrier(); }  // (the name the dual-FFT, block-DFT and backward kernels use)

// ---- LDS Stockham FFT of 2048 complex points (stft_mel_kernel, mfcc_fused_kernel, stft_vjp_kernel) ----
// LDS holds complex points as float2; element e lives at e ^ ((e >> 4) & 7) (no padding).  Unit-stride
// accesses (every read, the writes of passes 3 and 4) stay a permutation inside aligned 8-element blocks, i.e.
// conflict-free for ds_read_b64's 32-lane halves, and the stride-8 scatter of pass 1 lands its 16-lane write
// groups on 16 distinct 8-byte slots (pass 2's stride-64 scatter is 2-way).
constexpr int kFftLds = 2048 + 72;  // + room for the four weighted-power arrays laid over one buffer
__device__ __forceinline__ int padi(int i) { return i ^ ((i >> 4) & 7); }

struct cpx { float re, im; };
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cpx cmul(cpx a, cpx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cpx mul_mi(cpx a) { return {a.im, -a.re}; }  // a * (-i)

__device__ __forceinline__ void dft8(cpx (&v)[8]) {
  const float s = 0.70710678118654752440f;
  cpx a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]), a2 = cadd(v[2], v[6]), a3 = mul_mi(csub(v[2], v[6]));
  cpx a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]), a6 = cadd(v[3], v[7]), a7 = mul_mi(csub(v[3], v[7]));
  cpx b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = csub(a1, a3);
  cpx b4 = cadd(a4, a6), b6 = csub(a4, a6), b5 = cadd(a5, a7), b7 = csub(a5, a7);
  // w1 = (1 - i)/sqrt2, w2 = -i, w3 = (-1 - i)/sqrt2
  cpx t5 = {(b5.re + b5.im) * s, (b5.im - b5.re) * s};
  cpx t6 = mul_mi(b6);
  cpx t7 = {(b7.im - b7.re) * s, (-b7.re - b7.im) * s};
  v[0] = cadd(b0, b4); v[4] = csub(b0, b4);
  v[1] = cadd(b1, t5); v[5] = csub(b1, t5);
  v[2] = cadd(b2, t6); v[6] = csub(b2, t6);
  v[3] = cadd(b3, t7); v[7] = csub(b3, t7);
}

__device__ __forceinline__ void dft4(cpx (&v)[4]) {
  cpx a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), a2 = cadd(v[1], v[3]), a3 = mul_mi(csub(v[1], v[3]));
  v[0] = cadd(a0, a2); v[2] = csub(a0, a2); v[1] = cadd(a1, a3); v[3] = csub(a1, a3);
}

__device__ __forceinline__ void butterfly(cpx (&v)[8]) { dft8(v); }
__device__ __forceinline__ void butterfly(cpx (&v)[4]) { dft4(v); }

// one Stockham pass of radix R over 2048 points: butterfly j reads src[j + r*2048/R], multiplies by
// w^r, w = exp(-2 pi i k/(Ns R)), k = j mod Ns, writes dst[(j/Ns) Ns R + k + r Ns].
// Twiddles: w, w^2, w^4 come from the table, the other powers are one complex product away.
// In place on one LDS buffer: every thread reads its inputs, the workgroup meets (sync_between), then writes.
template <int R, int NB>
__device__ __forceinline__ void fft_pass(float2* __restrict__ buf, int Ns, int j0_, const float2* __restrict__ tw,
                                         const cpx* __restrict__ regs = nullptr) {
  constexpr int NR = 2048 / R;
  cpx vv[NB][R];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (regs) {
        vv[b][r] = regs[r];  // pass 1: butterfly j's inputs x[j + r*256] are exactly what thread j loaded
      } else {
        const float2 t = buf[padi(j0_ + 256 * b + r * NR)];
        vv[b][r] = {t.x, t.y};
      }
    }
  }
  if (!regs) __syncthreads();  // all reads of this pass are done before anybody overwrites the buffer
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    cpx (&v)[R] = vv[b];
    const int j = j0_ + 256 * b;
    float2* dst = buf;
  const int k = j & (Ns - 1);
  if (Ns > 1) {
    const int tstep = k * (2048 / (Ns * R));
    const float2 t1 = tw[tstep & 2047], t2 = tw[(2 * tstep) & 2047];
    const cpx w1 = {t1.x, t1.y}, w2 = {t2.x, t2.y};
    const cpx w3 = cmul(w1, w2);
    v[1] = cmul(v[1], w1);
    v[2] = cmul(v[2], w2);
    v[3] = cmul(v[3], w3);
    if (R == 8) {
      const float2 t4 = tw[(4 * tstep) & 2047];
      const cpx w4 = {t4.x, t4.y};
      v[4 % R] = cmul(v[4 % R], w4);
      v[5 % R] = cmul(v[5 % R], cmul(w1, w4));
      v[6 % R] = cmul(v[6 % R], cmul(w2, w4));
      v[7 % R] = cmul(v[7 % R], cmul(w3, w4));
    }
  }
  butterfly(v);
  const int j0 = (j - k) * R + k;
#pragma unroll
  for (int r = 0; r < R; ++r) dst[padi(j0 + r * Ns)] = make_float2(v[r].re, v[r].im);
  }
}

constexpr int kTPair = 1028;    // stride of the two float2 (frame 0, frame 1) weighted-power arrays, >= 1025 bins

// one Stockham pass with the butterfly's twiddles already in registers (w[r-1] = w^r)
template <int R>
__device__ __forceinline__ void fft_pass_regs(float2* __restrict__ buf, int Ns, int j, const cpx (&w)[R - 1], const cpx* __restrict__ regs) {
  constexpr int NR = 2048 / R;
  cpx v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (regs) {
      v[r] = regs[r];
    } else {
      const float2 t = buf[padi(j + r * NR)];
      v[r] = {t.x, t.y};
    }
  }
  if (!regs) {  // LDS-only barrier (see lds_barrier above)
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_s_barrier();
  }
  if (Ns > 1) {
#pragma unroll
    for (int r = 1; r < R; ++r) v[r] = cmul(v[r], w[r - 1]);
  }
  butterfly(v);
  const int k = j & (Ns - 1);
  const int j0 = (j - k) * R + k;
#pragma unroll
  for (int r = 0; r < R; ++r) buf[padi(j0 + r * Ns)] = make_float2(v[r].re, v[r].im);
}

template <int R>
__device__ __forceinline__ void load_tw(const float2* __restrict__ tw, int j, int Ns, cpx (&w)[R - 1]) {
  const int tstep = (j & (Ns - 1)) * (2048 / (Ns * R));
#pragma unroll
  for (int r = 1; r < R; ++r) {
    const float2 t = tw[(r * tstep) & 2047];
    w[r - 1] = {t.x, t.y};
  }
}

// ---- stft_bdft.hip: constant tables of the block-DFT kernel (device pointers, owned by the MFCC plan) ----
struct BdftTables {
  uint4* cfrag = nullptr;    // [4 tiles][2 planes][64 lanes]: stage-1 matrix (cos | -sin of W64), fp16 hi / lo fragments
  uint4* efrag = nullptr;    // [4 k-steps][2 planes][64 lanes]: stage-2 matrix (W32, complex as real 64 x 32)
  float4* tw = nullptr;      // [2 tiles][8][64 lanes]: inter-stage twiddles W2048^(n2 k1) x 2^-10 in accumulator order
  float* wlo = nullptr;      // [1024] mel weights of the lower / upper filter of every bin, x 0.25 / 8192^2
  float* whi = nullptr;
  unsigned long long* smask = nullptr;  // [16]: lanes whose bin 16 lane + j opens a mel run
  int4* mpos = nullptr;      // [128][2]: staging positions summed into mel m (run m of the lower plane | run m - 1 of the upper)
};
int bdft_tables_build(BdftTables* t);
void bdft_tables_free(BdftTables* t);
// `dct`: when non-null and one workgroup covers a whole clip (seg_frames >= n_frames <= 64, L <= 64), the kernel also applies the
// top_db floor and the DCT (+ optional StandardScaler affine) and writes the features: no dct_kernel launch afterwards.
struct BdftDct {
  int L = 0;                        // utterance_length: output frames per clip
  const float4* dct_frag = nullptr; // DCT-II rows in MFMA fragment order (MfccPlan::d_dct)
  const double* aff_mean = nullptr;
  const double* aff_scale = nullptr;
  float* out = nullptr;             // [batch][20 * L]
};
bool bdft_can_fuse_dct(int n_frames, int seg_frames, int L);
int launch_stft_bdft(const StftArgs& a, const BdftTables& t, int batch, int seg_frames, const BdftDct* dct, hipStream_t st);

// ---- mfcc_vjp.hip: vector-Jacobian product of the 2048/512 MFCC stage (kernels and their launchers; the plan glue is in mfcc.hip) ----
constexpr int kVjFrames = 8;                       // frames per workgroup of stft_vjp_kernel (even: frames go through the FFT in pairs)
constexpr int kVjSeg = (kVjFrames + 3) * 512;      // padded-signal samples those frames cover
struct MfccVjpArgs {
  const float* y;          // [batch][n_y] the 22 050 Hz signal the forward read
  int n_y, n_frames, batch, L;
  const float* db;         // [batch][n_frames][128] pre-floor dB of the forward
  const float* fmax;       // [batch][n_frames]
  const float* g_feat;     // [batch][20 L] cotangent
  const double* aff_scale; // [20 L] or null
  const float* dct_rows;   // [20][128]
  const float* hann;
  const float2* tw;
  const float* mel_wlo;    // [1025]
  const float* mel_whi;
  const int* bin_run;      // [1025]: the mel filter bin k feeds with weight wlo[k] (and bin_run + 1 with whi[k])
  float* gmel;             // [batch][n_frames][128] scratch: d loss / d mel
  float* part;             // [batch][n_groups][kVjSeg] scratch: overlap-added frame gradients of each frame group
  int n_groups;
  float* gy;               // [batch][n_y] out
};
// clips of different lengths in one launch (the RAGGED kernel instances): n_y / n_frames / n_groups above are then the row
// strides and every clip uses its own lengths (clip_lengths), as the forward does.  A type of its own, so that the kernels
// for one length keep the argument block they had.
struct MfccVjpRaggedArgs : MfccVjpArgs {
  const int* n_valid;      // [batch] samples per clip at sr_in
  int sr_in, n_samp_max;
};
// n_valid: null = one length for all
int launch_mfcc_vjp(const MfccVjpArgs& a, hipStream_t st, const int* n_valid = nullptr, int sr_in = 0, int n_samp_max = 0);
// gx = R^T gy for the polyphase resampler y[up q + p] = sum_k H[p][k] x[down q + noff[p] - (left - 1) + k], t < n_valid, in its own
// polyphase form gx[down q' + r] = sum_i HT[i][r] gy[up q' + t0[r] + i] (tables built by the plan, see resample_vjp_kernel)
struct ResampleVjpArgs {
  int n_y = 0, n_valid = 0, n_samp = 0, up = 1, down = 1;
  bool identity = false;
  const float* ht = nullptr;  // [nt][down]
  const int* t0 = nullptr;    // [down]
  int nt = 0, t0min = 0, t0max = 0;
  const int* nv = nullptr;    // [batch] samples per clip (device) or null: the RAGGED instance cuts every clip at its own length
  int sr_in = 0;
};
int launch_resample_vjp(const ResampleVjpArgs& a, const float* gy, float* gx, int batch, hipStream_t st);

}  // namespace lipasr
