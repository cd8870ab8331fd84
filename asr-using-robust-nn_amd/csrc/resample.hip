// K1 stage 1: batched resampling to 22 050 Hz, a polyphase restatement of resampy 'kaiser_best' (librosa.load's default):
//     y[up*q + p] = sum_k H[p][k] * x[down*q + n_p - (left-1) + k].
// The kernels, in the order pick_mfcc_path (mfcc.hip) prefers them; launch_resample at the end takes its choice and launches:
//   resample_persist_h2_kernel  the default at 16 kHz / 8 kHz (441/320, 441/160): the contraction on the fp16 matrix instruction
//                               with both operands split into two fp16 planes; float32 or int16 PCM rows, per-clip lengths
//   resample_persist_kernel     the same schedule in exact fp32 (its parity reference, SM_NO_H2)
//   resample_mfma_kernel        one q-block per workgroup: rows that cannot be read as float4
//   resample_reg128_kernel      128 taps in registers on the VALU (SM_VALU_RESAMPLER)
//   resample_generic_kernel     any rational ratio, taps from global memory
//   copy_pad_kernel             22 050 Hz input: copy and zero-pad
// and the host builders of the banded tap tables of the MFMA forms (build_band_tables, build_band_h2).
#include "mfcc_plan.h"
#include <type_traits>

namespace lipasr {

using namespace tables;

// ---------------------------------------------------------------------------------------------
// stage 1: resample
// ---------------------------------------------------------------------------------------------
constexpr int kRsQBlocks = 10;  // q-blocks (of `up` outputs) per workgroup in the register kernel

// 16 kHz -> 22.05 kHz fast path: taps == 128, up <= 448.  One thread per output phase.
__global__ __launch_bounds__(448) void resample_reg128_kernel(const float* __restrict__ x, int n_samp,
                                                               float* __restrict__ y, int n_valid, int n_y, int up,
                                                               int down, int left, const float* __restrict__ H,
                                                               const int* __restrict__ noff) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [kRsQBlocks*down + 128]
  const int u = blockIdx.y;
  const int q0 = blockIdx.x * kRsQBlocks;
  const int tid = threadIdx.x;
  const float* xu = x + (size_t)u * n_samp;
  const int win = kRsQBlocks * down + 128;
  const int base = q0 * down - (left - 1);  // xs[i] = x[base + i]
  for (int i = tid; i < win; i += 448) {
    const int n = base + i;
    xs[i] = (n >= 0 && n < n_samp) ? xu[n] : 0.0f;
  }
  float h[128];
  int np = 0;
  if (tid < up) {
    const float4* hr = reinterpret_cast<const float4*>(H + (size_t)tid * 128);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const float4 v = hr[k];
      h[4 * k] = v.x; h[4 * k + 1] = v.y; h[4 * k + 2] = v.z; h[4 * k + 3] = v.w;
    }
    np = noff[tid];
  }
  __syncthreads();
  if (tid >= up) return;
  float* yu = y + (size_t)u * n_y;
  for (int qq = 0; qq < kRsQBlocks; ++qq) {
    const int t = (q0 + qq) * up + tid;
    if (t >= n_y) break;
    const float* xp = xs + qq * down + np;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 128; ++k) acc = fmaf(h[k], xp[k], acc);
    yu[t] = (t < n_valid) ? acc : 0.0f;
  }
}

// any rational ratio: one workgroup per q-block, taps from global memory
__global__ __launch_bounds__(256) void resample_generic_kernel(const float* __restrict__ x, int n_samp,
                                                                float* __restrict__ y, int n_valid, int n_y, int up,
                                                                int down, int left, int taps,
                                                                const float* __restrict__ H,
                                                                const int* __restrict__ noff) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [down + taps]
  const int u = blockIdx.y, q = blockIdx.x, tid = threadIdx.x;
  const float* xu = x + (size_t)u * n_samp;
  const int win = down + taps;
  const int base = q * down - (left - 1);
  for (int i = tid; i < win; i += 256) {
    const int n = base + i;
    xs[i] = (n >= 0 && n < n_samp) ? xu[n] : 0.0f;
  }
  __syncthreads();
  float* yu = y + (size_t)u * n_y;
  for (int p = tid; p < up; p += 256) {
    const int t = q * up + p;
    if (t >= n_y) continue;
    const float* hr = H + (size_t)p * taps;
    const float* xp = xs + noff[p];
    float acc = 0.0f;
    for (int k = 0; k < taps; ++k) acc = fmaf(hr[k], xp[k], acc);
    yu[t] = (t < n_valid) ? acc : 0.0f;
  }
}


// ---------------------------------------------------------------------------------------------
// stage 1, MFMA form (16 kHz / 8 kHz -> 22.05 kHz: up = 441, 128 taps).
//   For a tile of 32 consecutive phases p0..p0+31 every tap reads an input sample in a band of at most
//   152 consecutive samples (offsets n_p0 .. n_p0+151 from the block start - 63), so
//       Y[utterance i][phase j] = sum_kk  X[i][kk] * Hband[kk][j]
//   is a 32 x 32 x 152 GEMM per (32 utterances, q-block, phase tile) on v_mfma_f32_32x32x2_f32 (exact
//   fp32 fma chain; the zero taps of the band add exact zeros).  One workgroup = 32 utterances x 1
//   q-block: the 32 x 448 input samples sit in LDS (row stride 481 = 1 mod 32: the A-operand read
//   `lane i -> row i` is conflict-free; 61.6 kB, so two workgroups share a CU and one's float4 fill
//   overlaps the other's MFMAs), 7 wavefronts take 2 of the 14 phase tiles each, the 76 tap fragments
//   of a tile are loaded up front (coalesced 128 B per half-wave from the L2-resident 272 kB table).
//   Output rows are phases: 128 B contiguous stores per half-wave.
// ---------------------------------------------------------------------------------------------
constexpr int kRsWaves = 7;

__global__ __launch_bounds__(64 * kRsWaves) void resample_mfma_kernel(const float* __restrict__ x, int n_samp, int batch,
                                                                       float* __restrict__ y, int n_valid, int n_y,
                                                                       int up, int down, int left, int n_ptiles,
                                                                       const float* __restrict__ Hband,
                                                                       const int* __restrict__ lo, int dbg) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [32][kRsStride]; xs[i][t] = x_i[down*q - 64 + t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, h = lane >> 5;
  // XCD-aware map (speed only, see stft_mel_kernel): blocks L, L+8, ... share an L2 and take consecutive q-blocks of
  // one 32-clip tile, whose input windows overlap by 127 of 447 samples
  int ut, q;
  {
    const int nqb = gridDim.x, L = blockIdx.y * gridDim.x + blockIdx.x;
    const int full = (gridDim.y / 8) * 8 * nqb;
    if (L < full) {
      const int chunk = L >> 3;
      ut = (chunk / nqb) * 8 + (L & 7);
      q = chunk % nqb;
    } else {
      ut = blockIdx.y;
      q = blockIdx.x;
    }
  }
  const int u0 = ut * 32;
  const int base = down * q - left;  // = down*q - 64: one sample before the first tap, 16-byte aligned
  constexpr int kVecPerRow = (kRsStride - 1) / 4;  // 120 float4 = 480 floats per row
  const bool vec = ((n_samp & 3) == 0) && ((down & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  if (!(dbg & SM_MFMA_SKIP_FILL)) {
    if (vec) {
      for (int f = tid; f < 32 * kVecPerRow; f += 64 * kRsWaves) {
        const int i = f / kVecPerRow, v = f - i * kVecPerRow;
        const int u = u0 + i, n = base + 4 * v;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u < batch && n >= 0 && n + 3 < n_samp) val = *reinterpret_cast<const float4*>(x + (size_t)u * n_samp + n);
        float* d = xs + i * kRsStride + 4 * v;
        d[0] = val.x; d[1] = val.y; d[2] = val.z; d[3] = val.w;
      }
      if (tid < 32) xs[tid * kRsStride + kRsStride - 1] = 0.0f;
    } else {
      for (int f = tid; f < 32 * kRsStride; f += 64 * kRsWaves) {
        const int i = f / kRsStride, t = f - i * kRsStride;
        const int u = u0 + i, n = base + t;
        xs[f] = (u < batch && n >= 0 && n < n_samp) ? x[(size_t)u * n_samp + n] : 0.0f;
      }
    }
  }
  __syncthreads();
  for (int r = wave; r < n_ptiles; r += kRsWaves) {
    rs_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const float* hb = Hband + (size_t)r * kRsBand * 32 + h * 32 + li;
    const float* xa = xs + li * kRsStride + lo[r] + 1 + h;
    // all 76 tap fragments of this phase tile go to registers first: 76 coalesced loads in flight at once
    float bq[kRsBand / 2];
#pragma unroll
    for (int s = 0; s < kRsBand / 2; ++s) bq[s] = hb[s * 64];
    __builtin_amdgcn_sched_barrier(0);  // keep every load ahead of the MFMA chain (do not sink them back in)
    if (dbg & SM_MFMA_SKIP_CHAIN) {
      acc[0] = bq[0] + bq[75] + xa[0];
    } else {
#pragma unroll
      for (int s = 0; s < kRsBand / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s], bq[s], acc, 0, 0, 0);
    }
    const int p = 32 * r + li;
    const int t = q * up + p;
    if (p < up && t < n_y) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int u = u0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (u < batch) y[(size_t)u * n_y + t] = t < n_valid ? acc[e] : 0.0f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// stage 1, persistent MFMA form.  Same contraction as resample_mfma_kernel, scheduled for the whole chip:
//   * one workgroup per (32-clip tile, q-range): 32 x 8 = 256 workgroups for 1024 clips, one per CU, each walking
//     6-7 consecutive q-blocks (the one-q-block kernel runs 1600 workgroups in 4 rounds on 512 slots, 3.1 rounds of work);
//   * one wavefront per phase tile (14 wavefronts): its 76 tap fragments are loaded ONCE and stay in registers for the
//     whole q-range (they were re-read from L2 for every q-block and clip tile: 436 MB per 1024 clips);
//   * the input window of the next q-block travels global -> registers while the current one feeds the MFMA chain,
//     then registers -> the other LDS buffer (2 x 61.6 kB), one barrier per q-block.
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64 * kRpMaxWaves) __attribute__((amdgpu_waves_per_eu(4, 4)))
void resample_persist_kernel(const float* __restrict__ x, int n_samp, int batch, float* __restrict__ y, int n_valid, int n_y,
                             int up, int down, int left, int nq, int n_tiles, const float* __restrict__ Hband,
                             const int* __restrict__ lo) {
  extern __shared__ __attribute__((aligned(16))) float xs2[];  // [2][32][kRsStride]
  const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // = phase tile
  const int li = lane & 31, h = lane >> 5;
  // 1-D grid of W workgroups over T clip tiles: tile t gets ceil((t+1) W / T) - ceil(t W / T) of them (so W need not be
  // a multiple of T: the grid is sized to the CUs this stream may use), each a contiguous share of the tile's q-blocks
  const int W = gridDim.x, T = n_tiles;
  const int tile = (int)(((long)blockIdx.x * T) / W);
  const int first = (int)(((long)tile * W + T - 1) / T), next = (int)(((long)(tile + 1) * W + T - 1) / T);
  const int n_ranges = next - first, ri = blockIdx.x - first;
  const int q_begin = (int)(((long)ri * nq) / n_ranges), q_end = (int)(((long)(ri + 1) * nq) / n_ranges);
  const int u0 = tile * 32;
  constexpr int kVecPerRow = (kRsStride - 1) / 4;   // 120 float4 = 480 floats per row
  constexpr int kFillMax = 5;                        // float4 per thread per window: 3840 over >= 768 threads
  // tap fragments of this wavefront's phase tile: loaded once
  float bq[kRsBand / 2];
  {
    const float* hb = Hband + (size_t)wave * kRsBand * 32 + h * 32 + li;
#pragma unroll
    for (int s = 0; s < kRsBand / 2; ++s) bq[s] = hb[s * 64];
  }
  const int lo_r = lo[wave];
  float4 stage[kFillMax];
  // (the thread index is made opaque in both helpers so that their per-slot addresses are recomputed where they are
  // used instead of living in 15-20 registers across the MFMA chain -- the fragments need those registers)
  auto fetch = [&](int q) {
    const int base = down * q - left;
    int tq = tid;
    asm volatile("" : "+v"(tq));
#pragma unroll
    for (int j = 0; j < kFillMax; ++j) {
      const int f = tq + j * nthreads;
      const int i = f / kVecPerRow, v = f - i * kVecPerRow;
      const int u = u0 + i, n = base + 4 * v;
      stage[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f < 32 * kVecPerRow && u < batch && n >= 0 && n + 3 < n_samp)
        stage[j] = *reinterpret_cast<const float4*>(x + (size_t)u * n_samp + n);
    }
  };
  auto deposit = [&](float* xs) {
    int tq = tid;
    asm volatile("" : "+v"(tq));
#pragma unroll
    for (int j = 0; j < kFillMax; ++j) {
      const int f = tq + j * nthreads;
      if (f < 32 * kVecPerRow) {
        const int i = f / kVecPerRow, v = f - i * kVecPerRow;
        float* d = xs + i * kRsStride + 4 * v;
        d[0] = stage[j].x; d[1] = stage[j].y; d[2] = stage[j].z; d[3] = stage[j].w;
      }
    }
    if (tid < 32) xs[tid * kRsStride + kRsStride - 1] = 0.0f;
  };
  if (q_begin < q_end) {
    fetch(q_begin);
    deposit(xs2);
  }
  __syncthreads();
  int cur = 0;
  for (int q = q_begin; q < q_end; ++q) {
    const bool more = q + 1 < q_end;
    if (more) fetch(q + 1);
    const float* xa = xs2 + cur * 32 * kRsStride + li * kRsStride + lo_r + 1 + h;
    rs_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int s = 0; s < kRsBand / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s], bq[s], acc, 0, 0, 0);
    const int pp = 32 * wave + li;
    const int t = q * up + pp;
    if (pp < up && t < n_y) {
      float* yb = y + (size_t)u0 * n_y;
      int off = 4 * h * n_y + t;
      asm volatile("" : "+v"(off));  // formed here: sixteen hoisted 64-bit row addresses would cost the fragment registers
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2);
        if (u0 + row + 4 * h < batch) yb[off + row * n_y] = t < n_valid ? acc[e] : 0.0f;
      }
    }
    if (more) deposit(xs2 + (cur ^ 1) * 32 * kRsStride);  // the other buffer: nobody reads it during this q-block
    // LDS-only barrier: __syncthreads() would also wait for this q-block's output stores to reach memory
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------
// stage 1, persistent MFMA form on the fp16 matrix instruction (round 3).  Same schedule as resample_persist_kernel; the
// contraction Y[32 clips][32 phases] = X[32][band] . Hband[band][32] runs on v_mfma_f32_32x32x16_f16 with BOTH operands
// split into two fp16 planes, x = x_hi + x_lo, h = h_hi + h_lo (hi = the value rounded to fp16's 11 significant bits, lo =
// the fp16 rounding of the remainder: 22 bits between them), and three of the four cross terms accumulated in fp32:
//       x h  ~=  x_hi h_hi + x_hi h_lo + x_lo h_hi          (dropped: x_lo h_lo <= 2^-22 |x h|)
// Every product of two fp16 numbers is exact in fp32, so the error is the 2^-22 of the two representations and of the
// dropped term: <= 3 x 2.4e-7 x sum |x h| <= 1e-6 per output sample in the worst case, 1e-7 typically -- the fp32 kernel's
// own accumulation error is 6e-8 x sqrt(128).  tests: 2e-6 against the float64 oracle, as for the fp32 kernel, which stays
// the parity reference (SM_NO_H2).       Cost: 3 matrix instructions of 32 cycles per 16 taps instead of 8 of 64 cycles
// (v_mfma_f32_32x32x2_f32): 5.3x less matrix-pipe time (44 us of the fp32 kernel's 87 us per 1024 clips were MFMA-busy).
// fp16's exponent range is short: the low plane of a value below 2^-14 x 2^11 = 0.125 falls on the subnormal grid (step
// 2^-24) and a quiet passage at -60 dB would come out with a relative error of 1e-4.  So both operands are scaled by powers
// of two before the split -- the samples by 2^11 (full 22-bit precision down to |x| = 6e-5 = -84 dB, an absolute floor of
// 1.5e-11 below that; |x| must stay below 32, audio is in [-1, 1)), the taps by 2^6 -- and the accumulator by 2^-17
// afterwards (all exact).  The band of a phase tile starts at a multiple of 8
// samples (16-byte aligned ds_read_b128 of 8 consecutive fp16) and is padded to 160 = 10 k-steps.
// LDS per window: 32 rows x {hi[480] | lo[480]} fp16 + 16 bytes = 1936 B per row (121 x 16: the 32 rows of a b128 read
// fall on different bank quads), the same 62 kB as the fp32 window, double-buffered.
// ---------------------------------------------------------------------------------------------
typedef _Float16 rs_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 rs_h4 __attribute__((ext_vector_type(4)));

// I16: int16 PCM in (float32 otherwise).  RAGGED: nv[] holds a length per clip (else every row is n_samp long and nv is not read).
template <bool I16, bool RAGGED>
__global__ __launch_bounds__(64 * kRpMaxWaves) __attribute__((amdgpu_waves_per_eu(4, 4)))
void resample_persist_h2_kernel(const void* __restrict__ xv, const int* __restrict__ nv, int sr_in, int n_samp, int batch, float* __restrict__ y, int n_valid, int n_y,
                                int up, int down, int left, int nq, int n_tiles, const uint4* __restrict__ HbandH,
                                const int* __restrict__ lo, int n_ptiles_rt, int dbg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char xh[];  // [2][32][kRhRowBytes]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // = phase tile
  const int li = lane & 31, h = lane >> 5;
  const int W = gridDim.x, T = n_tiles;
  const int tile = (int)(((long)blockIdx.x * T) / W);
  const int first = (int)(((long)tile * W + T - 1) / T), next = (int)(((long)(tile + 1) * W + T - 1) / T);
  const int n_ranges = next - first, ri = blockIdx.x - first;
  const int q_begin = (int)(((long)ri * nq) / n_ranges), q_end = (int)(((long)(ri + 1) * nq) / n_ranges);
  const int u0 = tile * 32;
  constexpr int kVecPerRow = kRhRowHalfs / 4;  // 120 float4 per row
  constexpr int kFillMax = 4;  // 16 wavefronts fill (3840 float4 over 1024 threads); the first n_ptiles of them also multiply
  const bool mm = wave < n_ptiles_rt;
  // tap fragments of this wavefront's phase tile, both planes: loaded once  [tile][plane][chunk][lane] x 16 bytes
  rs_h8 bh[kRhChunks], bl[kRhChunks];
  if (mm) {
    const uint4* hb = HbandH + ((size_t)wave * 2 * kRhChunks) * 64 + lane;
#pragma unroll
    for (int c = 0; c < kRhChunks; ++c) {
      const uint4 t0 = hb[c * 64], t1 = hb[(kRhChunks + c) * 64];
      bh[c] = __builtin_bit_cast(rs_h8, t0);
      bl[c] = __builtin_bit_cast(rs_h8, t1);
    }
  }
  const int band0 = mm ? ((lo[wave] + 1) & ~7) : 0;  // first sample of the band in the window, a multiple of 8
  // what a fill holds between its loads and its LDS stores: float4, or the four int16 samples as they came
  using stage_t = typename std::conditional<I16, short4, float4>::type;
  stage_t stage[kFillMax];
  // Fill mapping without divisions: a wavefront moves two window rows (16 wavefronts, 32 rows), lane l the 4-sample columns l and
  // l + 64 of each (120 of the 128 exist): 1 KB contiguous per load instruction (fp32), 512 B per LDS store, and the length of
  // the row's clip is wave-uniform -- it stays in a scalar register (this kernel has no vector register to spare: the tap
  // fragments alone take 80 of its 128).
  const int r0 = u0 + 2 * wave;
  const int n_clip0 = __builtin_amdgcn_readfirstlane((r0 < batch) ? (RAGGED ? min(max(nv[r0], 0), n_samp) : n_samp) : 0);
  const int n_clip1 = __builtin_amdgcn_readfirstlane((r0 + 1 < batch) ? (RAGGED ? min(max(nv[r0 + 1], 0), n_samp) : n_samp) : 0);
  // outputs from int(n ratio) on are zeros (fix_length).  With per-clip lengths that is at most ONE sample per clip that anyone
  // reads (ceil(n ratio) - int(n ratio) <= 1) and stft_mel2_kernel, which knows the clip's length, takes it as zero itself
  const int t_lim = RAGGED ? n_y : n_valid;
  auto fetch = [&](int q) {
    const int base = down * q - left;  // a multiple of 4, as n_samp is
    const stage_t* src = static_cast<const stage_t*>(xv) + (((long)r0 * n_samp + base) >> 2) + lane;
#pragma unroll
    for (int j = 0; j < kFillMax; ++j) {
      const int v = lane + 64 * (j & 1), n = base + 4 * v;
      const int n_clip = (j >> 1) ? n_clip1 : n_clip0;
      stage[j] = stage_t{};
      // (n + 3 < n_samp: n and n_samp are multiples of 4; a clip that ends inside the four is cut in deposit)
      if (v < kVecPerRow && n >= 0 && n < n_clip) stage[j] = src[(j >> 1) * (n_samp >> 2) + 64 * (j & 1)];
    }
  };
  auto deposit = [&](unsigned char* xs, int q) {
    unsigned char* drow = xs + 2 * wave * kRhRowBytes + 8 * lane;
    // a clip that ends inside a group of four: what follows in the row is not the clip's.  Cut under a scalar branch (rare; no
    // select on the path below, where every register is taken -- as it is, this code costs the RAGGED instances two spilled
    // tap fragments, reloaded per q-block)
#pragma unroll
    for (int r = 0; RAGGED && r < 2; ++r) {
      const int rel = (r ? n_clip1 : n_clip0) - (down * q - left);  // samples of the clip in this window (wave-uniform)
      if ((rel & 3) != 0 && rel > 0 && rel < 4 * kVecPerRow) {
        const int g = rel >> 2, cr = rel & 3;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          if (lane + 64 * jj == g) {
            stage_t& t = stage[2 * r + jj];
            if (cr <= 1) t.y = 0;
            if (cr <= 2) t.z = 0;
            t.w = 0;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kFillMax; ++j) {
      if (lane + 64 * (j & 1) < kVecPerRow) {
        float e[4];
        if constexpr (I16) {
          const short4 sv = stage[j];
          e[0] = (float)sv.x * (kRhSigScale / 32768.0f); e[1] = (float)sv.y * (kRhSigScale / 32768.0f);
          e[2] = (float)sv.z * (kRhSigScale / 32768.0f); e[3] = (float)sv.w * (kRhSigScale / 32768.0f);
        } else {
          const float4 fv = stage[j];
          e[0] = fv.x * kRhSigScale; e[1] = fv.y * kRhSigScale; e[2] = fv.z * kRhSigScale; e[3] = fv.w * kRhSigScale;
        }
        rs_h4 hi, lw;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float sc = fminf(fmaxf(e[c], -65000.0f), 65000.0f);
          const _Float16 a = (_Float16)sc;
          hi[c] = a;
          lw[c] = (_Float16)(sc - (float)a);
        }
        unsigned char* d = drow + (j >> 1) * kRhRowBytes + 512 * (j & 1);
        *reinterpret_cast<rs_h4*>(d) = hi;
        *reinterpret_cast<rs_h4*>(d + 2 * kRhRowHalfs) = lw;
        // a clip that ends inside this group of four: what follows in the row is not the clip's.  Zeroed after the fact, by
        // the lane that wrote it (rare, and no select on the main path)
      }
    }
  };
  if (q_begin < q_end) {
    fetch(q_begin);
    deposit(xh, q_begin);
  }
  __syncthreads();
  int cur = 0;
  for (int q = q_begin; q < q_end; ++q) {
    const bool more = q + 1 < q_end && !(dbg & H2_NO_PREFETCH);  // (dbg: profiling switches, results wrong)
    if (more) fetch(q + 1);
    const unsigned char* xa = xh + cur * 32 * kRhRowBytes + li * kRhRowBytes + 2 * (band0 + 8 * h);
    rs_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    if (mm && !(dbg & H2_SKIP_MFMA)) {
#pragma unroll
    for (int c = 0; c < kRhChunks; ++c) {
      const rs_h8 ah = *reinterpret_cast<const rs_h8*>(xa + 32 * c);
      const rs_h8 al = *reinterpret_cast<const rs_h8*>(xa + 32 * c + 2 * kRhRowHalfs);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[c], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[c], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[c], acc, 0, 0, 0);
    }
    }
    const int pp = 32 * wave + li;
    const int t = q * up + pp;
    if (mm && pp < up && t < n_y && !(dbg & H2_SKIP_STORE)) {
      float* yb = y + (size_t)u0 * n_y;
      int off = 4 * h * n_y + t;
      asm volatile("" : "+v"(off));
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2);
        if (u0 + row + 4 * h < batch) yb[off + row * n_y] = t < t_lim ? acc[e] * (1.0f / (kRhTapScale * kRhSigScale)) : 0.0f;
      }
    }
    if (more) deposit(xh + (cur ^ 1) * 32 * kRhRowBytes, q + 1);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }
}

__global__ __launch_bounds__(256) void copy_pad_kernel(const float* __restrict__ x, int n_samp, float* __restrict__ y,
                                                        int n_y) {
  const int u = blockIdx.y;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_y; i += gridDim.x * 256)
    y[(size_t)u * n_y + i] = i < n_samp ? x[(size_t)u * n_samp + i] : 0.0f;
}

// With per-clip lengths the resamplers leave the filter's ringing past a clip's int(n ratio) outputs (the STFT kernels, which
// know the length, read zeros there themselves).  A caller that takes the resampled rows gets fix_length's zeros instead.
__global__ __launch_bounds__(256) void clear_tail_kernel(float* __restrict__ y, int n_y, const int* __restrict__ nv, int n_samp, int sr_in) {
  const int u = blockIdx.y;
  int n_vy, c_y, c_frames;
  clip_lengths(min(max(nv[u], 0), n_samp), sr_in, &n_vy, &c_y, &c_frames);
  for (int i = n_vy + blockIdx.x * 256 + threadIdx.x; i < n_y; i += gridDim.x * 256) y[(size_t)u * n_y + i] = 0.0f;
}

int launch_clear_tail(const MfccPlan* p, const int* n_valid, int batch, float* y, hipStream_t st) {
  hipLaunchKernelGGL(clear_tail_kernel, dim3(32, batch), dim3(256), 0, st, y, p->n_y, n_valid, p->n_samp, p->sr_in);
  ++g_k1_launches[K1_CLEAR_TAIL];
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

// Banded taps [n_tiles][kRsBand][32] and first-phase offsets [n_tiles] for the MFMA resampler; false when the
// ratio does not fit its fixed geometry (128 taps, band <= 152 samples, LDS row of 801 floats).
bool build_band_tables(const Polyphase& pp, std::vector<float>* hb_out, std::vector<int>* lo_out) {
  if (!(pp.taps == 128 && pp.left == 64 && pp.down + 128 <= kRsStride - 1)) return false;
  const int nt = (pp.up + 31) / 32;
  std::vector<float> hb((size_t)nt * kRsBand * 32, 0.0f);
  std::vector<int> lo(nt, 0);
  for (int r = 0; r < nt; ++r) {
    const int p0 = 32 * r;
    lo[r] = pp.n_off[p0];
    for (int j = 0; j < 32; ++j) {
      const int ph = p0 + j;
      if (ph >= pp.up) break;
      const int d = pp.n_off[ph] - pp.n_off[p0];
      if (d < 0 || d + 128 > kRsBand) return false;
      for (int t = 0; t < 128; ++t) hb[((size_t)r * kRsBand + d + t) * 32 + j] = pp.h[(size_t)ph * 128 + t];
    }
    // the last sample a workgroup's band can touch must stay inside its LDS row
    if (lo[r] + 1 + kRsBand > kRsStride) return false;
  }
  *hb_out = hb;
  *lo_out = lo;
  return true;
}

// fp16 hi / lo fragments of the banded taps in the B-operand lane order of v_mfma_f32_32x32x16_f16: lane (col, h) of k-step c
// holds B[k = 16 c + 8 h + j][col], j < 8; the band starts at the window position (lo + 1) & ~7
std::vector<unsigned int> build_band_h2(const std::vector<float>& hb, const std::vector<int>& lo) {
  const int nt = (int)lo.size();
  std::vector<unsigned int> out((size_t)nt * 2 * kRhChunks * 64 * 4, 0u);
  for (int r = 0; r < nt; ++r) {
    const int first = lo[r] + 1, band0 = first & ~7;
    for (int c = 0; c < kRhChunks; ++c)
      for (int ln = 0; ln < 64; ++ln) {
        const int col = ln & 31, hh = ln >> 5;
        unsigned short hi[8], lw[8];
        for (int j = 0; j < 8; ++j) {
          const int kk = band0 + 16 * c + 8 * hh + j - first;  // index into the 152-sample band of the fp32 table
          const float v = (kk >= 0 && kk < kRsBand) ? hb[((size_t)r * kRsBand + kk) * 32 + col] * kRhTapScale : 0.0f;
          const _Float16 a = (_Float16)v;
          const _Float16 b = (_Float16)(v - (float)a);
          memcpy(&hi[j], &a, 2);
          memcpy(&lw[j], &b, 2);
        }
        unsigned int* dh = &out[((((size_t)r * 2 + 0) * kRhChunks + c) * 64 + ln) * 4];
        unsigned int* dl = &out[((((size_t)r * 2 + 1) * kRhChunks + c) * 64 + ln) * 4];
        for (int w = 0; w < 4; ++w) {
          dh[w] = (unsigned int)hi[2 * w] | ((unsigned int)hi[2 * w + 1] << 16);
          dl[w] = (unsigned int)lw[2 * w] | ((unsigned int)lw[2 * w + 1] << 16);
        }
      }
  }
  return out;
}

// Launches the resampler pick_mfcc_path chose (it has checked that `kind` can read these rows)
int launch_resample(const MfccPlan* p, MfccPath::Resampler kind, const void* wav_any, int fmt, const int* n_valid, int batch, float* y,
                    hipStream_t st) {
  const float* wav = static_cast<const float*>(wav_any);
  const int nq = (p->n_y + p->up - 1) / p->up, tiles = (batch + 31) / 32;
  int wgs = p->rs_target_wgs;  // persistent forms: one workgroup per CU this stream may use
  if (wgs < tiles) wgs = tiles;
  if (wgs > tiles * nq) wgs = tiles * nq;
  switch (kind) {
    case MfccPath::RS_H2: {
      const size_t ldsh = (size_t)2 * 32 * kRhRowBytes;
      using kern_t = void (*)(const void*, const int*, int, int, int, float*, int, int, int, int, int, int, int, const uint4*, const int*, int, int);
      static const kern_t kerns[4] = {resample_persist_h2_kernel<false, false>, resample_persist_h2_kernel<true, false>,
                                      resample_persist_h2_kernel<false, true>, resample_persist_h2_kernel<true, true>};
      const int inst = (fmt ? 1 : 0) + (n_valid ? 2 : 0);
      const kern_t kern = kerns[inst];
      LP_DYN_LDS(kern, ldsh);
      hipLaunchKernelGGL(kern, dim3(wgs), dim3(64 * kRpMaxWaves), ldsh, st, wav_any, n_valid,
                         p->sr_in, p->n_samp, batch, y, p->n_valid, p->n_y, p->up, p->down, p->left, nq, tiles,
                         reinterpret_cast<const uint4*>(p->d_hbandh), p->d_lo, p->n_ptiles, (p->stage_mask >> SM_H2_SHIFT) & SM_H2_BITS);
      ++g_k1_launches[K1_RESAMPLE_H2 + inst];
      break;
    }
    case MfccPath::RS_PERSIST_F32: {
      // persistent fp32 form (the parity reference of the fp16-plane kernel): one workgroup per CU-sized share of the work
      const size_t lds = (size_t)2 * 32 * kRsStride * sizeof(float);
      LP_DYN_LDS(resample_persist_kernel, lds);
      hipLaunchKernelGGL(resample_persist_kernel, dim3(wgs), dim3(64 * p->n_ptiles), lds, st, wav, p->n_samp, batch, y,
                         p->n_valid, p->n_y, p->up, p->down, p->left, nq, tiles, p->d_hband, p->d_lo);
      ++g_k1_launches[K1_RESAMPLE_PERSIST];
      break;
    }
    case MfccPath::RS_MFMA: {
      const size_t lds = (size_t)32 * kRsStride * sizeof(float);
      LP_DYN_LDS(resample_mfma_kernel, lds);
      hipLaunchKernelGGL(resample_mfma_kernel, dim3(nq, (batch + 31) / 32), dim3(64 * kRsWaves), lds, st, wav,
                         p->n_samp, batch, y, p->n_valid, p->n_y, p->up, p->down, p->left, p->n_ptiles, p->d_hband, p->d_lo, p->stage_mask);
      ++g_k1_launches[K1_RESAMPLE_MFMA];
      break;
    }
    case MfccPath::RS_REG128: {
      const int nb = (nq + kRsQBlocks - 1) / kRsQBlocks;
      const size_t lds = (size_t)(kRsQBlocks * p->down + 128) * sizeof(float);
      hipLaunchKernelGGL(resample_reg128_kernel, dim3(nb, batch), dim3(448), lds, st, wav, p->n_samp, y, p->n_valid,
                         p->n_y, p->up, p->down, p->left, p->d_h, p->d_noff);
      ++g_k1_launches[K1_RESAMPLE_REG128];
      break;
    }
    case MfccPath::RS_GENERIC: {
      const size_t lds = (size_t)(p->down + p->taps) * sizeof(float);
      hipLaunchKernelGGL(resample_generic_kernel, dim3(nq, batch), dim3(256), lds, st, wav, p->n_samp, y, p->n_valid,
                         p->n_y, p->up, p->down, p->left, p->taps, p->d_h, p->d_noff);
      ++g_k1_launches[K1_RESAMPLE_GENERIC];
      break;
    }
    case MfccPath::RS_COPY:
      hipLaunchKernelGGL(copy_pad_kernel, dim3(32, batch), dim3(256), 0, st, wav, p->n_samp, y, p->n_y);
      ++g_k1_launches[K1_COPY_PAD];
      break;
    case MfccPath::RS_NONE:
      set_error("launch_resample: no resampler was chosen");
      return LIPASR_ESTATE;
  }
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr
