// K1 stages 2 and 3 outside the default STFT kernel: launch_from_22k runs the STFT kind pick_mfcc_path (mfcc.hip) chose, then the DCT.
//   (stft_bdft_kernel   the default 2048/512 STFT -> power -> mel -> dB, a block DFT on the matrix pipe: stft_bdft.hip)
//   dct_kernel          stage 3 of every path: per clip the global maximum -> top_db floor, DCT-II (ortho) 128 -> 20, frame axis cut /
//                       zero-padded to utterance_length, coefficient-major layout, optional fused StandardScaler affine
//   stft_mel2_kernel    ST_STOCKHAM4 (SM_STOCKHAM), the parity reference of the block DFT and the forward that the backward pass runs
//                       for its own tile (plan_vjp in mfcc.hip; every frame scaled by its own power of two): one workgroup = four reflect-padded
//                       Hann-windowed frames as two complex 2048-point Stockham FFTs in packed lock step
//   stft_mel_kernel     ST_STOCKHAM2 (SM_ROUND2_STFT): two frames packed into ONE complex FFT (radix 8-8-8-4 in registers, LDS
//                       ping-pong), separated by conjugate symmetry, sparse Slaney mel bank (<= 2 filters per bin), 10 log10
//   dft_mel_kernel      ST_DFT, short windows of any length: the windowed real DFT as an fp32 MFMA contraction
#include "mfcc_plan.h"

namespace lipasr {

using namespace tables;

// ---------------------------------------------------------------------------------------------
// stage 2: STFT -> power -> mel -> dB
// ---------------------------------------------------------------------------------------------
// (padi, cpx, dft8 / dft4 and fft_pass live in stft.h: the backward kernels of mfcc_vjp.hip run the same passes)

__global__ __launch_bounds__(256) void stft_mel_kernel(StftArgs a) {
  __shared__ __attribute__((aligned(16))) float2 buf[kFftLds];  // ONE buffer: 17 kB per workgroup
  __shared__ float wmax[4];
  __shared__ float2 rsum[2][128];  // run sums (frame 0, frame 1): [weight array][run]
  const int tid = threadIdx.x;
  // XCD-aware block -> (clip, frame pair) map (speed only): workgroups are dealt round-robin over the 8 XCDs, so
  // blocks L, L+8, L+16, ... share an L2.  Giving those to consecutive frame pairs of ONE clip lets the 75 %
  // overlap between neighbouring frames hit in that L2 instead of being re-fetched by four different XCDs.
  int u, fp;
  {
    const int npairs = gridDim.x, L = blockIdx.y * gridDim.x + blockIdx.x;
    const int nb = gridDim.y;
    const int full = (nb / 8) * 8 * npairs;  // blocks covered by complete groups of 8 clips
    if (L < full) {
      const int xcd = L & 7, chunk = L >> 3;
      u = (chunk / npairs) * 8 + xcd;
      fp = chunk % npairs;
    } else {
      u = blockIdx.y;
      fp = blockIdx.x;
    }
  }
  const int f0 = fp * 2, f1 = f0 + 1;
  const bool has1 = f1 < a.n_frames;
  const float* yu = a.y + (size_t)u * a.n_y;
  // per-thread constants of the mel stage (L2-resident tables) start their trip now, not after the FFT's last barrier.
  // Wavefront w sums weight array w&1 (lower / upper filter of each bin) over run (w>>1)*64 + lane, both frames at once.
  const int mel_part = (tid >> 6) & 1, mel_run = ((tid >> 7) << 6) + (tid & 63);
  const int mst = a.mel_start[mel_run], mln = a.mel_len[mel_run];
  float mwl[5], mwh[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int k = tid + 256 * i;
    mwl[i] = (k <= 1024) ? a.mel_wlo[k] : 0.0f;
    mwh[i] = (k <= 1024) ? a.mel_whi[k] : 0.0f;
  }
  // frame f covers padded positions [512 f, 512 f + 2048) = y positions [512 f - 1024, ...)
  cpx x0[8];
  if (has1 && f0 >= 2 && f1 * 512 + 1024 <= a.n_y) {
    // both frames lie inside the clip (20 of the 22 pairs of a 1-s clip): no reflection, and frame 1 is frame 0 moved
    // by 512 samples = two of this thread's 256-sample steps, so ten loads feed both (workgroup-uniform branch)
    const float* p = yu + (f0 * 512 - 1024) + tid;
    float sm[10];
#pragma unroll
    for (int e = 0; e < 10; ++e) sm[e] = p[256 * e];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float w = a.hann[tid + 256 * e];
      x0[e] = {w * sm[e], w * sm[e + 2]};
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int n = tid + 256 * e;
      const float w = a.hann[n];
      const int j0 = f0 * 512 + n - 1024;
      const float s0 = yu[reflect_index(j0, a.n_y)];
      const float s1 = has1 ? yu[reflect_index(j0 + 512, a.n_y)] : 0.0f;
      x0[e] = {w * s0, w * s1};
    }
  }
  if (a.stage_mask & SM_SKIP_FFT) {
#pragma unroll
    for (int e = 0; e < 8; ++e) buf[padi(tid + 256 * e)] = make_float2(x0[e].re, x0[e].im);
    __syncthreads();
  } else {
    fft_pass<8, 1>(buf, 1, tid, a.tw, x0);  // straight from registers: no staging write
    __syncthreads();
    fft_pass<8, 1>(buf, 8, tid, a.tw);
    __syncthreads();
    fft_pass<8, 1>(buf, 64, tid, a.tw);
    __syncthreads();
    fft_pass<4, 2>(buf, 512, tid, a.tw);  // radix 4: two butterflies per thread
    __syncthreads();
  }
  // Z = FFT(frame0 + i frame1).  X0[k] = (Z[k] + conj Z[N-k])/2, X1[k] = (Z[k] - conj Z[N-k])/(2i).
  // The powers of bin k (frame 0, frame 1) are multiplied straight away by the bin's two mel weights and stored as
  // PAIRS: Tlo[k] = wlo[k] (P0[k], P1[k]), Thi[k] = whi[k] (P0[k], P1[k]) -- two float2 arrays laid over the same buffer
  // once Z has been read, so that the mel sums below move both frames with one ds_read_b64 + one packed add.
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
  float2* T = buf;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int k = tid + 256 * i;
    if (k <= 1024) {
      const float zr = zz[i].x, zi = zz[i].y, wr = zc[i].x, wi = -zc[i].y;
      const float x0r = 0.5f * (zr + wr), x0i = 0.5f * (zi + wi);
      const float x1r = 0.5f * (zi - wi), x1i = -0.5f * (zr - wr);
      const float p0 = x0r * x0r + x0i * x0i, p1 = x1r * x1r + x1i * x1i;
      const float wl = mwl[i], wh = mwh[i];
      T[k] = make_float2(wl * p0, wl * p1);
      T[kTPair + k] = make_float2(wh * p0, wh * p1);
    }
  }
  __syncthreads();
  // mel[m] = sum over run(m) of Tlo + sum over run(m-1) of Thi.  The kernel is VALU-issue bound, so the sums are
  // arranged for few instructions: one lane per (weight array, run) adds BOTH frames with packed adds, four loads in
  // flight off one address; the (frame, m) threads then pick their two run sums up from a 2 kB exchange array.
  const int sel = tid >> 7, m = tid & 127;
  float s = 0.0f;
  if (!(a.stage_mask & SM_SKIP_MEL)) {
    const float2* Tp = T + mel_part * kTPair + mst;
    float2 a0 = make_float2(0.0f, 0.0f), a1 = a0, a2 = a0, a3 = a0;
    int i = 0;
    for (; i + 4 <= mln; i += 4) {
      const float2 v0 = Tp[i], v1 = Tp[i + 1], v2 = Tp[i + 2], v3 = Tp[i + 3];
      a0.x += v0.x; a0.y += v0.y; a1.x += v1.x; a1.y += v1.y;
      a2.x += v2.x; a2.y += v2.y; a3.x += v3.x; a3.y += v3.y;
    }
    for (; i < mln; ++i) { const float2 v = Tp[i]; a0.x += v.x; a0.y += v.y; }
    rsum[mel_part][mel_run] = make_float2((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y));
    __syncthreads();
    const float* rs = reinterpret_cast<const float*>(&rsum[0][0]);
    s = rs[2 * m + sel] + ((m > 0) ? rs[2 * (128 + m - 1) + sel] : 0.0f);
  } else {
    s = sel ? T[m].y : T[m].x;
  }
  const float dbv = power_to_db(s);  // librosa.power_to_db(ref=1, amin=1e-10)
  const int f = sel ? f1 : f0;
  if (f < a.n_frames) a.db[((size_t)u * a.n_frames + f) * 128 + m] = dbv;
  const float wm = wave_max(dbv);
  if ((tid & 63) == 0) wmax[tid >> 6] = wm;
  __syncthreads();
  if (tid == 0) a.fmax[(size_t)u * a.n_frames + f0] = fmaxf(wmax[0], wmax[1]);
  if (tid == 128 && has1) a.fmax[(size_t)u * a.n_frames + f1] = fmaxf(wmax[2], wmax[3]);
}

// ---------------------------------------------------------------------------------------------
// stage 2, dual form (round 3): one workgroup = one clip x FOUR frames = two complex FFTs (A = frames f0 + i f1,
// B = f2 + i f3) evaluated by the same threads in lock step, the pair (A, B) in the two halves of every packed-fp32
// operand.  stft_mel_kernel keeps (re, im) of ONE FFT in a packed operand, and half of its vector instructions are the
// half-swaps, negations and moves complex arithmetic needs in that layout (112 v_mov + 57 v_cndmask against 285
// packed math instructions, 686 per wavefront in all).  With (A, B) packed, a complex product is two v_pk_mul + two
// v_pk_fma on plain registers, x(-i) is a register renaming, and one address computation serves both FFTs: about a third
// of the vector instructions per frame.  LDS: one float4 {reA, reB, imA, imB} per point, index e + (e >> 4) (one float4 of
// padding per 16): every access of the four passes is `per-thread base + compile-time offset` -- the XOR swizzle of
// stft_mel_kernel cost three integer instructions per access -- unit-stride ds_read_b128 are conflict-free, and so is the
// stride-8 scatter of pass 1 (8 lanes -> 8 x 4 distinct banks).  34.9 kB + 4 kB per workgroup: four workgroups per CU.
// The two mel weights of a bin multiply the four frames' powers at once (float4 {f0, f2, f1, f3}).
// ---------------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));
struct cp2 { v2f re, im; };
__device__ __forceinline__ cp2 add2(cp2 a, cp2 b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cp2 sub2(cp2 a, cp2 b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cp2 mulw(cp2 a, cpx w) { return {a.re * w.re - a.im * w.im, a.re * w.im + a.im * w.re}; }
__device__ __forceinline__ cp2 mmi2(cp2 a) { return {a.im, -a.re}; }  // a * (-i)

__device__ __forceinline__ void dft8_2(cp2 (&v)[8]) {
  const float s = 0.70710678118654752440f;
  cp2 a0 = add2(v[0], v[4]), a1 = sub2(v[0], v[4]), a2 = add2(v[2], v[6]), a3 = mmi2(sub2(v[2], v[6]));
  cp2 a4 = add2(v[1], v[5]), a5 = sub2(v[1], v[5]), a6 = add2(v[3], v[7]), a7 = mmi2(sub2(v[3], v[7]));
  cp2 b0 = add2(a0, a2), b2 = sub2(a0, a2), b1 = add2(a1, a3), b3 = sub2(a1, a3);
  cp2 b4 = add2(a4, a6), b6 = sub2(a4, a6), b5 = add2(a5, a7), b7 = sub2(a5, a7);
  cp2 t5 = {(b5.re + b5.im) * s, (b5.im - b5.re) * s};
  cp2 t6 = mmi2(b6);
  cp2 t7 = {(b7.im - b7.re) * s, (-b7.re - b7.im) * s};
  v[0] = add2(b0, b4); v[4] = sub2(b0, b4);
  v[1] = add2(b1, t5); v[5] = sub2(b1, t5);
  v[2] = add2(b2, t6); v[6] = sub2(b2, t6);
  v[3] = add2(b3, t7); v[7] = sub2(b3, t7);
}
__device__ __forceinline__ void dft4_2(cp2 (&v)[4]) {
  cp2 a0 = add2(v[0], v[2]), a1 = sub2(v[0], v[2]), a2 = add2(v[1], v[3]), a3 = mmi2(sub2(v[1], v[3]));
  v[0] = add2(a0, a2); v[2] = sub2(a0, a2); v[1] = add2(a1, a3); v[3] = sub2(a1, a3);
}

constexpr int kF2Buf = 2 * 1028 + 8;  // float4 elements: 2048 points, or the two weighted-power arrays of 1025 bins
constexpr int kF2TP = 1028;                    // stride of the two weighted-power arrays laid over the buffer
__device__ __forceinline__ float4 ld4(const float4* p) { return *p; }
__device__ __forceinline__ void st4(float4* p, cp2 v) { *p = make_float4(v.re.x, v.re.y, v.im.x, v.im.y); }
__device__ __forceinline__ cp2 tocp2(float4 t) { return {v2f{t.x, t.y}, v2f{t.z, t.w}}; }

// Radix-8 Stockham pass of the dual FFT.  rbase / wbase: this thread's padded float4 index of element 0 of its reads
// and writes; the other seven are compile-time offsets (RO(r), WO(r)).
#define LP_F2_PASS8(RO, WO, TW, FIRST)                                                    \
  {                                                                                        \
    cp2 v[8];                                                                              \
    if (FIRST) {                                                                           \
      _Pragma("unroll") for (int r = 0; r < 8; ++r) v[r] = x0[r];                          \
    } else {                                                                               \
      _Pragma("unroll") for (int r = 0; r < 8; ++r) v[r] = tocp2(ld4(rd + (RO(r))));       \
      lds_barrier2();                                                                      \
      _Pragma("unroll") for (int r = 1; r < 8; ++r) v[r] = mulw(v[r], TW[r - 1]);          \
    }                                                                                      \
    dft8_2(v);                                                                             \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) st4(wr + (WO(r)), v[r]);                 \
  }

// the power of two that brings a frame of peak m into [1, 2) (0 for a zero frame; a frame below 2^-30 is all at amin anyway, and the
// square of the factor must stay finite)
__device__ __forceinline__ int frame_peak_exp(float m) { return m > 0.0f ? min(max(ilogbf(m), -30), 30) : 0; }

// Four frames (f0 .. f0 + 3) of clip u: two complex FFTs in packed lock step, powers, mel, dB.  On return thread (pr = tid >> 7,
// m = tid & 127) holds the dB values of mel bin m for frames f0 + 2 pr (dbe) and f0 + 2 pr + 1 (dbo), which it has also
// stored to a.db.  buf / rsum: the workgroup's LDS; every barrier inside is an LDS-only barrier.
__device__ __forceinline__ void stft2_quad(const StftArgs& a, float4* __restrict__ buf, float4 (*__restrict__ rsum)[128],
                                           const float* __restrict__ yu, int u, int f0, int tid, int n_vy, int n_y, int n_frames, float& dbe, float& dbo) {
  const int lane = tid & 63;
  // per-thread constants (L2-resident tables), on their way before the sample loads
  const int mel_part = (tid >> 6) & 1, mel_run = ((tid >> 7) << 6) + lane;
  const int mst = a.mel_start[mel_run], mln = a.mel_len[mel_run];
  float hw[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) hw[e] = a.hann[tid + 256 * e];
  // twiddles of passes 2 and 3 leave now (their L2 round trip hides behind the sample loads and pass 1); those of pass 4 and
  // the mel weights are requested one pass ahead of their use.  The barriers below wait for LDS traffic only.
  cpx w2[7], w3[7];
  load_tw<8>(a.tw, tid, 8, w2);
  load_tw<8>(a.tw, tid, 64, w3);
  cp2 x0[8];
  if (f0 >= 2 && f0 + 3 < n_frames && (f0 + 3) * 512 + 1024 <= n_vy) {
    // all four frames inside the clip: frame j is frame 0 moved by 2 j of the thread's 256-sample steps
    const float* p = yu + (f0 * 512 - 1024) + tid;
    float sm[14];
#pragma unroll
    for (int e = 0; e < 14; ++e) sm[e] = p[256 * e];
#pragma unroll
    for (int e = 0; e < 8; ++e) x0[e] = {v2f{hw[e] * sm[e], hw[e] * sm[e + 4]}, v2f{hw[e] * sm[e + 2], hw[e] * sm[e + 6]}};
  } else {
    // edge quads (2 of a 1-s clip's 11): the generic np.pad index costs a division per sample -- a quarter of the kernel's
    // average instruction count when every edge quad paid it; clips longer than the padding reflect once
    if (n_y > kNFft) {  // workgroup-uniform
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j0 = f0 * 512 + tid + 256 * e - 1024;
        float sj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = reflect_once(j0 + 512 * j, n_y);
            sj[j] = (f0 + j < n_frames && k < n_vy) ? yu[k] : 0.0f;  // [n_vy, n_y): fix_length's zeros
          }
        x0[e] = {v2f{hw[e] * sj[0], hw[e] * sj[2]}, v2f{hw[e] * sj[1], hw[e] * sj[3]}};
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j0 = f0 * 512 + tid + 256 * e - 1024;
        float sj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = reflect_index(j0 + 512 * j, n_y);
            sj[j] = (f0 + j < n_frames && k < n_vy) ? yu[k] : 0.0f;
          }
        x0[e] = {v2f{hw[e] * sj[0], hw[e] * sj[2]}, v2f{hw[e] * sj[1], hw[e] * sj[3]}};
      }
    }
  }
  // ---- Frames f0, f1 share one complex transform and f2, f3 the other, and a transform's rounding error is 2^-24 of the LARGER of its
  // two spectra: a quiet frame next to a loud one would take the loud one's noise (measured: mel powers 73 x further from float64
  // than a float32 evaluation frame by frame).  Every frame is brought to a peak in [1, 2) by a power of two first -- exact -- and its
  // powers take the square of the factor back.  Frames of one binade keep the bits they had.  (rsum is free until the mel sums.)
  v2f q02, q13;  // {f0, f2}, {f1, f3}: 4^exponent
  {
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      m0 = fmaxf(m0, fabsf(x0[e].re.x)); m2 = fmaxf(m2, fabsf(x0[e].re.y));
      m1 = fmaxf(m1, fabsf(x0[e].im.x)); m3 = fmaxf(m3, fabsf(x0[e].im.y));
    }
    m0 = wave_max(m0); m1 = wave_max(m1); m2 = wave_max(m2); m3 = wave_max(m3);
    if (lane == 0) rsum[0][tid >> 6] = make_float4(m0, m1, m2, m3);
    lds_barrier2();
    const float4 t0 = rsum[0][0], t1 = rsum[0][1], t2 = rsum[0][2], t3 = rsum[0][3];
    const int e0 = frame_peak_exp(fmaxf(fmaxf(t0.x, t1.x), fmaxf(t2.x, t3.x))), e1 = frame_peak_exp(fmaxf(fmaxf(t0.y, t1.y), fmaxf(t2.y, t3.y)));
    const int e2 = frame_peak_exp(fmaxf(fmaxf(t0.z, t1.z), fmaxf(t2.z, t3.z))), e3 = frame_peak_exp(fmaxf(fmaxf(t0.w, t1.w), fmaxf(t2.w, t3.w)));
    const v2f n02 = {ldexpf(1.0f, -e0), ldexpf(1.0f, -e2)}, n13 = {ldexpf(1.0f, -e1), ldexpf(1.0f, -e3)};
#pragma unroll
    for (int e = 0; e < 8; ++e) { x0[e].re *= n02; x0[e].im *= n13; }
    q02 = v2f{ldexpf(1.0f, 2 * e0), ldexpf(1.0f, 2 * e2)};
    q13 = v2f{ldexpf(1.0f, 2 * e1), ldexpf(1.0f, 2 * e3)};
  }
  // ---- four passes.  Element e lives at float4 index swz(e) = e ^ (((e >> 4) & 3) << 1): inside every aligned block
  // of 16 float4 (one 256-byte bank row) a permutation, so unit-stride ds_read_b128 stay conflict-free in the hardware's
  // lane groups, and the stride-8 scatter of pass 1 spreads its 8-lane store groups over 8 different bank quads
  // (scratch/lds_model.py; additive padding made every read 2-way: 29 % of the LDS cycles of the first version).
  // Bits 4-5 of e are bits 4-5 of the thread index for every read and for the writes of passes 3 and 4, so those
  // addresses are `per-thread base + compile-time offset`; passes 1 and 2 pay one v_xor per store.
  const int sx = ((tid >> 4) & 3) << 1;
  const int tsw = tid ^ sx;  // swz(tid + 256 r) = tsw + 256 r
  {
    // pass 1 (Ns = 1): butterfly j = tid writes e = 8 j + r: bits 4-5 of e = bits 1-2 of j
    float4* wr = buf + 8 * tid;
    const int s1 = ((tid >> 1) & 3) << 1;
    const float4* rd = buf;  // (unused: pass 1 takes its inputs from registers)
#define LP_RO1(r) 0
#define LP_WO1(r) ((r) ^ s1)
    const cpx* none = nullptr;
    LP_F2_PASS8(LP_RO1, LP_WO1, none, true)
#undef LP_RO1
#undef LP_WO1
  }
  lds_barrier2();
  {
    // pass 2 (Ns = 8): reads tid + 256 r; writes e = 64 (j >> 3) + k + 8 r: bits 4-5 of e = r >> 1, so the xor value
    // 2 (r >> 1) is a compile-time constant applied to k = j & 7
    const float4* rd = buf + tsw;
    const int k = tid & 7;
    float4* wr = buf + 64 * (tid >> 3);
#define LP_RO2(r) (256 * (r))
#define LP_WO2(r) (8 * (r) + (k ^ (((r) >> 1) << 1)))
    LP_F2_PASS8(LP_RO2, LP_WO2, w2, false)
#undef LP_WO2
  }
  cpx wa[3], wb[3];
  load_tw<4>(a.tw, tid, 512, wa);
  load_tw<4>(a.tw, tid + 256, 512, wb);
  lds_barrier2();
  {
    // pass 3 (Ns = 64): writes e = 512 (j >> 6) + k + 64 r, k = j & 63: bits 4-5 of e = bits 4-5 of k
    const float4* rd = buf + tsw;
    const int k = tid & 63;
    float4* wr = buf + 512 * (tid >> 6) + (k ^ (((k >> 4) & 3) << 1));
#define LP_WO3(r) (64 * (r))
    LP_F2_PASS8(LP_RO2, LP_WO3, w3, false)
#undef LP_WO3
#undef LP_RO2
  }
  float mwl[5], mwh[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int kb = tid + 256 * i;
    mwl[i] = (kb <= 1024) ? a.mel_wlo[kb] : 0.0f;
    mwh[i] = (kb <= 1024) ? a.mel_whi[kb] : 0.0f;
  }
  lds_barrier2();
  // pass 4 (Ns = 512, radix 4): butterflies j = tid and tid + 256 read and write e = j + 512 r.  Its outputs are the
  // spectrum in natural order: bin tid + 256 i of this thread is va[i / 2] (i even) or vb[i / 2] (i odd)
  cp2 va[4], vb[4];
  {
    float4* pa = buf + tsw;
    float4* pb = pa + 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) { va[r] = tocp2(ld4(pa + 512 * r)); vb[r] = tocp2(ld4(pb + 512 * r)); }
    lds_barrier2();
#pragma unroll
    for (int r = 1; r < 4; ++r) { va[r] = mulw(va[r], wa[r - 1]); vb[r] = mulw(vb[r], wb[r - 1]); }
    dft4_2(va);
    dft4_2(vb);
    // only the upper half of the spectrum goes back to LDS: the partners Z[2048 - k] of the bins k <= 1024 live there
#pragma unroll
    for (int r = 2; r < 4; ++r) { st4(pa + 512 * r, va[r]); st4(pb + 512 * r, vb[r]); }
  }
  lds_barrier2();
  // ---- separation by conjugate symmetry, powers, the two mel weights of each bin.  Z[k] is in registers (above); the
  // partner Z[2048 - k] belongs to another thread and comes from LDS (k = 0 is its own partner).
  float4 zc[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int kb = tid + 256 * i;
    if (kb <= 1024) {
      const int kc = 2048 - kb;  // 1024 .. 2048
      if (kb == 0) zc[i] = make_float4(va[0].re.x, va[0].re.y, va[0].im.x, va[0].im.y);
      else zc[i] = buf[kc ^ (((kc >> 4) & 3) << 1)];
    }
  }
  lds_barrier2();
  float4* T = buf;  // Tlo[k] at k, Thi[k] at kF2TP + k: {f0, f2, f1, f3} x weight
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int kb = tid + 256 * i;
    if (kb <= 1024) {
      const cp2 z = (i & 1) ? vb[i >> 1] : va[i >> 1];
      const v2f zr = z.re, zi = z.im, cr = {zc[i].x, zc[i].y}, ci = {-zc[i].z, -zc[i].w};
      const v2f x0r = 0.5f * (zr + cr), x0i = 0.5f * (zi + ci), x1r = 0.5f * (zi - ci), x1i = -0.5f * (zr - cr);
      const v2f p0 = (x0r * x0r + x0i * x0i) * q02, p1 = (x1r * x1r + x1i * x1i) * q13;  // {f0, f2}, {f1, f3}
      T[kb] = make_float4(mwl[i] * p0.x, mwl[i] * p0.y, mwl[i] * p1.x, mwl[i] * p1.y);
      T[kF2TP + kb] = make_float4(mwh[i] * p0.x, mwh[i] * p0.y, mwh[i] * p1.x, mwh[i] * p1.y);
    }
  }
  lds_barrier2();
  // ---- mel run sums: one lane per (weight array, run), all four frames per load
  {
    const float4* Tp = T + mel_part * kF2TP + mst;
    v2f s0 = {0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int i = 0;
    for (; i + 2 <= mln; i += 2) {
      const float4 t0 = Tp[i], t1 = Tp[i + 1];
      s0 += v2f{t0.x, t0.y}; s1 += v2f{t0.z, t0.w};
      s2 += v2f{t1.x, t1.y}; s3 += v2f{t1.z, t1.w};
    }
    if (i < mln) { const float4 t0 = Tp[i]; s0 += v2f{t0.x, t0.y}; s1 += v2f{t0.z, t0.w}; }
    s0 += s2; s1 += s3;
    rsum[mel_part][mel_run] = make_float4(s0.x, s0.y, s1.x, s1.y);
  }
  lds_barrier2();
  // ---- mel = run(m) of Tlo + run(m - 1) of Thi; thread (pair, m) finishes frames f0 + 2 pair and f0 + 2 pair + 1
  const int pr = tid >> 7, m = tid & 127;
  float4 sum = rsum[0][m];
  if (m > 0) { const float4 h2 = rsum[1][m - 1]; sum.x += h2.x; sum.y += h2.y; sum.z += h2.z; sum.w += h2.w; }
  const float se = pr ? sum.y : sum.x, so = pr ? sum.w : sum.z;  // even / odd frame of the pair
  dbe = power_to_db(se);
  dbo = power_to_db(so);
  const int fe = f0 + 2 * pr, fo = fe + 1;
  if (fe < n_frames) a.db[((size_t)u * a.n_frames + fe) * 128 + m] = dbe;
  if (fo < n_frames) a.db[((size_t)u * a.n_frames + fo) * 128 + m] = dbo;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void stft_mel2_kernel(StftArgs a) {
  __shared__ __attribute__((aligned(16))) float4 buf[kF2Buf];
  __shared__ __attribute__((aligned(16))) float4 rsum[2][128];  // run sums {f0, f2, f1, f3}: [weight array][run]
  __shared__ float wmax[4][2];
  const int tid = threadIdx.x, lane = tid & 63;
  // XCD-aware block -> (clip, frame quad) map, as in stft_mel_kernel
  int u, fq;
  {
    const int nq = gridDim.x, L = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.y;
    const int full = (nb / 8) * 8 * nq;
    if (L < full) {
      const int chunk = L >> 3;
      u = (chunk / nq) * 8 + (L & 7);
      fq = chunk % nq;
    } else {
      u = blockIdx.y;
      fq = blockIdx.x;
    }
  }
  const int f0 = 4 * fq;
  const float* yu = a.y + (size_t)u * a.n_y;
  int n_y = a.n_y, n_frames = a.n_frames, n_vy = a.n_y;  // (one length for all: y already ends in its zeros)
  if (a.n_valid) {  // this clip's own length: frame count and reflect padding follow it
    clip_lengths(min(max(a.n_valid[u], 0), a.n_samp_max), a.sr_in, &n_vy, &n_y, &n_frames);
    n_frames = min(n_frames, a.n_frames);
  }
  if (f0 >= n_frames) return;  // (workgroup-uniform, before any barrier)
  float dbe, dbo;
  stft2_quad(a, buf, rsum, yu, u, f0, tid, n_vy, n_y, n_frames, dbe, dbo);
  const float me = wave_max(dbe), mo = wave_max(dbo);
  if (lane == 0) { wmax[tid >> 6][0] = me; wmax[tid >> 6][1] = mo; }
  lds_barrier2();
  if (tid < 4) {
    const int f = f0 + tid, w0 = 2 * (tid >> 1), c = tid & 1;
    if (f < n_frames) a.fmax[(size_t)u * a.n_frames + f] = fmaxf(wmax[w0][c], wmax[w0 + 1][c]);
  }
}
#undef LP_F2_PASS8

// ---------------------------------------------------------------------------------------------
// stage 2 for a short window of any length (Speaker recognition/extract_features_construct_dataset.py:224-226:
// librosa.feature.mfcc(win_length=441, n_fft=441, hop_length=220), 1 + 22050/220 = 101 frames): the windowed
// real DFT evaluated as an fp32 MFMA contraction  frames[rows][n_fft] x table[n_fft][re | im].
//
// Layout: every clip is thought of as reflect-padded into rpc*hop floats (rpc = rows per clip), so that global
// frame row r starts at position r*hop for ALL clips: the overlapping frames are just a matrix with leading
// dimension hop; rows frame >= n_frames of a clip are computed and dropped.  The padded layout is virtual -- the
// reflection is applied while a workgroup stages its rows.  One workgroup takes 64 consecutive rows: their
// samples (63*hop + K floats) are staged in LDS once, wavefront t owns the 32 bins of tile t and streams the
// table's 64 columns (re, im) for those bins from L2 in double-buffered groups of 8 K-steps, four
// 32x32x2 MFMA accumulators (2 row blocks x re/im).  Power goes back to LDS, then mel (CSR bank, sequential
// fp32 like the FFT path), dB and the per-frame maximum, one wavefront per row.
// ---------------------------------------------------------------------------------------------
struct DftArgs {
  const float* y;      // [batch][n_y] (unpadded: the reflect padding is applied while the rows are staged)
  const float* table;  // [k_rows][n_tiles*64]
  int n_y, batch;
  int hop, n_fft, k_rows, n_tiles, rpc, n_frames, total_rows;
  const int* mel_start;
  const int* mel_len;
  const int* mel_off;
  const float* mel_w;
  float* db;    // [B][n_frames][128]
  float* fmax;  // [B][n_frames]
};

__global__ __launch_bounds__(64 * kDftMaxTiles) __attribute__((amdgpu_waves_per_eu(4, 4))) void dft_mel_kernel(DftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, n_waves = nthreads >> 6;
  const int row0 = blockIdx.x * kDftRows;
  {
    // position g of the virtual padded layout (clip c at c * rpc * hop, np.pad(y, N/2, 'reflect') inside): 64 rows
    // span at most two clips because rpc > 64 is not required -- the clip index is found per element
    const int n_a = (kDftRows - 1) * a.hop + a.n_fft + 1;
    const int stride = a.rpc * a.hop, pad = a.n_fft / 2;
    const long g0 = (long)row0 * a.hop;
    for (int i = tid; i < n_a; i += nthreads) {
      const long g = g0 + i;
      const int c = (int)(g / stride);
      const int j = (int)(g - (long)c * stride);
      float v = 0.0f;
      if (c < a.batch && j < a.n_y + 2 * pad) {
        int k = j - pad;  // the edge sample is not repeated
        if (k < 0) k = -k;
        else if (k >= a.n_y) k = 2 * (a.n_y - 1) - k;
        v = a.y[(size_t)c * a.n_y + k];
      }
      dsm[i] = v;
    }
  }
  __syncthreads();
  const int li = lane & 31, kk = lane >> 5;
  const int ld = a.n_tiles * 64;
  rs_f32x16 re0, im0, re1, im1;
#pragma unroll
  for (int q = 0; q < 16; ++q) { re0[q] = 0.f; im0[q] = 0.f; re1[q] = 0.f; im1[q] = 0.f; }
  const float* bp = a.table + (size_t)kk * ld + wave * 64 + li;
  // row n of the folded table meets x[n] + x[(N - n) mod N] (real part) and x[n] - x[(N - n) mod N] (imaginary part)
  // (n = 2 s + kk walks forward from x[kk], its partner N - n backward from x[N - kk]; n = 0 meets x[N], one
  // past the frame, under a zero weight (w[0] = 0); padded rows n > N/2 stay inside the frame and meet zero rows)
  const float* fw0 = dsm + li * a.hop + kk;
  const float* bw0 = dsm + li * a.hop + a.n_fft - kk;
  const float* fw1 = fw0 + 32 * a.hop;
  const float* bw1 = bw0 + 32 * a.hop;
  const int n_groups = a.k_rows / (2 * kDftGroup);
  float br0[kDftGroup], bi0[kDftGroup], br1[kDftGroup], bi1[kDftGroup];
#define LP_DFT_LOAD(BR, BI, G)                                          \
  _Pragma("unroll") for (int u = 0; u < kDftGroup; ++u) {               \
    const float* q_ = bp + (size_t)(2 * ((G) * kDftGroup + u)) * ld;    \
    BR[u] = q_[0];                                                      \
    BI[u] = q_[32];                                                     \
  }
#define LP_DFT_MAC(BR, BI, G)                                           \
  _Pragma("unroll") for (int u = 0; u < kDftGroup; ++u) {               \
    const int s_ = 2 * ((G) * kDftGroup + u);                           \
    const float p0_ = fw0[s_], q0_ = bw0[-s_], p1_ = fw1[s_], q1_ = bw1[-s_]; \
    re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(p0_ + q0_, BR[u], re0, 0, 0, 0); \
    im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(p0_ - q0_, BI[u], im0, 0, 0, 0); \
    re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(p1_ + q1_, BR[u], re1, 0, 0, 0); \
    im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(p1_ - q1_, BI[u], im1, 0, 0, 0); \
  }
  LP_DFT_LOAD(br0, bi0, 0)
  for (int g = 0; g < n_groups; g += 2) {
    if (g + 1 < n_groups) { LP_DFT_LOAD(br1, bi1, g + 1) }
    LP_DFT_MAC(br0, bi0, g)
    if (g + 1 < n_groups) {
      if (g + 2 < n_groups) { LP_DFT_LOAD(br0, bi0, g + 2) }
      LP_DFT_MAC(br1, bi1, g + 1)
    }
  }
#undef LP_DFT_LOAD
#undef LP_DFT_MAC
  __syncthreads();  // every wavefront is done with the staged samples: the buffer becomes the power tile
  const int ldp = a.n_tiles * 32 + 1;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int r = (q & 3) + 8 * (q >> 2) + 4 * kk;
    dsm[r * ldp + wave * 32 + li] = re0[q] * re0[q] + im0[q] * im0[q];
    dsm[(32 + r) * ldp + wave * 32 + li] = re1[q] * re1[q] + im1[q] * im1[q];
  }
  __syncthreads();
  // mel + dB, one wavefront per frame row: lane handles filters lane and lane + 64
  for (int r = wave; r < kDftRows; r += n_waves) {
    const int grow = row0 + r;
    const int clip = grow / a.rpc, frame = grow - clip * a.rpc;
    if (grow >= a.total_rows || frame >= a.n_frames) continue;  // wave-uniform
    const float* pr = dsm + r * ldp;
    float dbv[2];
#pragma unroll
    for (int hmel = 0; hmel < 2; ++hmel) {
      const int m = lane + 64 * hmel;
      const int st = a.mel_start[m], ln = a.mel_len[m];
      const float* w = a.mel_w + a.mel_off[m];
      float sacc = 0.0f;
      for (int j = 0; j < ln; ++j) sacc = fmaf(w[j], pr[st + j], sacc);
      dbv[hmel] = power_to_db(sacc);  // librosa.power_to_db(ref=1, amin=1e-10)
    }
    float* dst = a.db + ((size_t)clip * a.n_frames + frame) * 128;
    dst[lane] = dbv[0];
    dst[lane + 64] = dbv[1];
    const float mx = wave_max(fmaxf(dbv[0], dbv[1]));
    if (lane == 0) a.fmax[(size_t)clip * a.n_frames + frame] = mx;
  }
}

// ---------------------------------------------------------------------------------------------
// stage 3: top_db floor, DCT, layout
// ---------------------------------------------------------------------------------------------

constexpr int kDctFrames = 64;  // most frames per workgroup (blockIdx.y = chunk): LDS stays <= 33 kB whatever the clip length

// One workgroup = one clip x `chunk` <= 64 output frames, two wavefronts (32 frames each):
//   out[c][t] = sum_m D[c][m] * max(dB[t][m], clipmax - 80)      c < 20 (padded to 32), m < 128
// as a 32 x 32 x 128 contraction per wavefront on v_mfma_f32_32x32x2_f32 (the same ascending-m fp32 fma chain a
// scalar loop would run): the DCT rows are the A operand (64 registers per lane: the table is stored in fragment order,
// [row][k parity][64], so a lane's share is 16 float4 loads, requested together with the dB tile), the clamped dB tile is
// staged transposed in LDS (row stride chunk + 1, odd: conflict-free writes, unit-stride B-operand reads).  The LDS
// image follows the chunk (44 frames: 23 kB, six workgroups per CU instead of four).
// n_frames = frames per clip the db / frame_max arrays are laid out for; with n_valid (clips of different lengths in
// one launch) clip u has its own, smaller count and frames past it are zero columns, as fix_frames pads them
// (extract_features_construct_dataset.py:33-37).
__global__ __launch_bounds__(128) void dct_kernel(const float* __restrict__ db, const float* __restrict__ frame_max,
                                                   int n_frames, int L, int chunk, const float4* __restrict__ dct_frag,
                                                   const double* __restrict__ aff_mean,
                                                   const double* __restrict__ aff_scale, float* __restrict__ out,
                                                   const int* __restrict__ n_valid, int n_samp_max, int sr_in) {
  extern __shared__ float dbs[];  // [128][chunk + 1] = [m][t]
  __shared__ float red[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = blockIdx.x;
  const int li = lane & 31, h = lane >> 5;
  const int t0 = blockIdx.y * chunk;                  // first output frame of this chunk
  const int tl = min(chunk, L - t0);                  // output frames of this chunk (incl. zero padding)
  int nf = n_frames;                                  // frames this clip really has
  if (n_valid) {
    int nvy, ny;
    clip_lengths(min(max(n_valid[u], 0), n_samp_max), sr_in, &nvy, &ny, &nf);
    nf = min(nf, n_frames);
  }
  const int tu = max(0, min(nf - t0, tl));            // of which computed from the spectrogram
  const int tp = chunk + 1;
  // dB tile: up to 64 frames x 128 mels = 64 floats per thread, ALL in flight at once (a plain loop keeps one load in
  // flight per thread, and every load here is a cold-L2 round trip: that was 28 of the first kernel's 30 us)
  const float* src = db + ((size_t)u * n_frames + t0) * 128;
  const int n_live = tu * 128;
  float stage[kDctFrames];
#pragma unroll
  for (int j = 0; j < kDctFrames; ++j) {
    const int i = tid + 128 * j;
    stage[j] = (i < n_live) ? src[i] : 0.0f;
  }
  // A operand: lane (li, h) holds D[li][2 s + h], s < 64 (rows >= 20 are zero in the table)
  float4 av4[16];
  const float4* ap = dct_frag + (li * 2 + h) * 16;
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) av4[s4] = ap[s4];
  float mx = -INFINITY;
  for (int t = tid; t < nf; t += 128) mx = fmaxf(mx, frame_max[(size_t)u * n_frames + t]);  // whole clip
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  const float thr = fmaxf(red[0], red[1]) - 80.0f;  // top_db = 80
#pragma unroll
  for (int j = 0; j < kDctFrames; ++j) {
    const int i = tid + 128 * j;  // frame j, mel tid: consecutive lanes, consecutive banks
    if (j < chunk) dbs[tid * tp + j] = (i < n_live) ? fmaxf(stage[j], thr) : 0.0f;
  }
  __syncthreads();
  rs_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  // (a wavefront whose 32 frames lie past the chunk still runs the chain on zeros of its own: columns >= chunk are never
  // stored, and the reads stay inside the image: clamp the column)
  const float* bp = dbs + h * tp + min(wave * 32 + li, chunk - 1);
#pragma unroll
  for (int s4 = 0; s4 < 16; ++s4) {
    const float a4[4] = {av4[s4].x, av4[s4].y, av4[s4].z, av4[s4].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], bp[2 * (4 * s4 + e) * tp], acc, 0, 0, 0);
  }
  // C layout: row (coefficient) = (q & 3) + 8 (q >> 2) + 4 h, column (frame) = li
  const int t = wave * 32 + li;
  const int n_out = kNMfcc * L;
  if (t < tl) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = (q & 3) + 8 * (q >> 2) + 4 * h;
      if (c < kNMfcc) {
        float v = (t < tu) ? acc[q] : 0.0f;
        const int oo = c * L + t0 + t;
        if (aff_mean) v = (float)(((double)v - aff_mean[oo]) / aff_scale[oo]);
        out[(size_t)u * n_out + oo] = v;
      }
    }
  }
}

// dct_kernel's A operand: lane (row li, k parity h) reads D[li][2 s + h], s < 64, as 16 float4
std::vector<float> dct_fragments() {
  const std::vector<float> d = tables::dct_matrix();  // [20][128]
  std::vector<float> f((size_t)32 * 2 * 64, 0.0f);
  for (int li = 0; li < kNMfcc; ++li)
    for (int h = 0; h < 2; ++h)
      for (int s = 0; s < 64; ++s) f[((size_t)li * 2 + h) * 64 + s] = d[(size_t)li * 128 + 2 * s + h];
  return f;
}

int launch_dct(const MfccPlan* p, int batch, int L, const double* am, const double* as, float* out, const int* n_valid,
                      hipStream_t st) {
  const int chunk = std::min(kDctFrames, (L + 3) & ~3);  // even, so that the LDS row stride chunk + 1 is odd
  const size_t lds = (size_t)128 * (chunk + 1) * sizeof(float);
  hipLaunchKernelGGL(dct_kernel, dim3(batch, (L + chunk - 1) / chunk), dim3(128), lds, st, p->d_db, p->d_fmax, p->n_frames, L, chunk,
                     reinterpret_cast<const float4*>(p->d_dct), am, as, out, n_valid, p->n_samp, p->sr_in);
  ++g_k1_launches[K1_DCT];
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

void fill_stft_args(const MfccPlan* p, const float* y, StftArgs* a) {
  a->y = y; a->n_y = p->n_y; a->n_frames = p->n_frames; a->hann = p->d_hann;
  a->tw = reinterpret_cast<const float2*>(p->d_tw);
  a->mel_wlo = p->d_mel_wlo; a->mel_whi = p->d_mel_whi; a->mel_start = p->d_mel_pstart; a->mel_len = p->d_mel_plen;
  a->db = p->d_db; a->fmax = p->d_fmax;
  a->stage_mask = p->stage_mask;
  a->n_valid = nullptr; a->sr_in = p->sr_in; a->n_samp_max = p->n_samp;
}

int launch_from_22k(const MfccPlan* p, MfccPath::Stft kind, const float* y, const int* n_valid, int batch, int L, const double* am,
                    const double* as, float* out, hipStream_t st, hipEvent_t mid, bool stft_only) {
  StftArgs a;
  fill_stft_args(p, y, &a);
  a.n_valid = n_valid;
  switch (kind) {
    case MfccPath::ST_DFT: {
      DftArgs d;
      d.y = y; d.n_y = p->n_y; d.batch = batch; d.table = p->d_dft; d.hop = p->hop; d.n_fft = p->n_fft; d.k_rows = p->dft_krows; d.n_tiles = p->dft_tiles;
      d.rpc = p->dft_rpc; d.n_frames = p->n_frames; d.total_rows = batch * p->dft_rpc;
      d.mel_start = p->d_mel_start; d.mel_len = p->d_mel_len; d.mel_off = p->d_mel_off; d.mel_w = p->d_mel_w;
      d.db = p->d_db; d.fmax = p->d_fmax;
      const int n_a = (kDftRows - 1) * p->hop + p->n_fft + 1, n_p = kDftRows * (p->dft_tiles * 32 + 1);
      const size_t dl = (size_t)(n_a > n_p ? n_a : n_p) * sizeof(float);
      LP_DYN_LDS(dft_mel_kernel, dl);
      hipLaunchKernelGGL(dft_mel_kernel, dim3((d.total_rows + kDftRows - 1) / kDftRows), dim3(64 * p->dft_tiles), dl, st, d);
      ++g_k1_launches[K1_DFT_MEL];
      break;
    }
    case MfccPath::ST_BDFT: {
      // one workgroup per clip: on request (plan key 4) the kernel finishes with the top_db floor and the DCT itself
      const bool fuse = !stft_only && p->bd_fuse_dct && bdft_can_fuse_dct(p->n_frames, p->bd_seg, L);
      BdftDct d;
      d.L = L; d.dct_frag = reinterpret_cast<const float4*>(p->d_dct); d.aff_mean = am; d.aff_scale = as; d.out = out;
      const int rc = launch_stft_bdft(a, p->bd, batch, p->bd_seg, fuse ? &d : nullptr, st);
      if (rc != LIPASR_OK) return rc;
      if (fuse) {
        if (mid) LP_HIP(hipEventRecord(mid, st));
        return LIPASR_OK;
      }
      break;
    }
    case MfccPath::ST_STOCKHAM4:
      hipLaunchKernelGGL(stft_mel2_kernel, dim3((p->n_frames + 3) / 4, batch), dim3(256), 0, st, a);
      ++g_k1_launches[K1_STFT_MEL2];
      break;
    case MfccPath::ST_STOCKHAM2:
      hipLaunchKernelGGL(stft_mel_kernel, dim3((p->n_frames + 1) / 2, batch), dim3(256), 0, st, a);
      ++g_k1_launches[K1_STFT_MEL];
      break;
  }
  LP_LAUNCH_CHECK();
  if (mid) LP_HIP(hipEventRecord(mid, st));
  if (stft_only) return LIPASR_OK;
  return launch_dct(p, batch, L, am, as, out, n_valid, st);
}

}  // namespace lipasr
