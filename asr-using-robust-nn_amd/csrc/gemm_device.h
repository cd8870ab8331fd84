// K2: device code shared by the GEMM tile families (gemm_frag.hip, gemm_lds.hip, gemm_ring.hip, gemm_ring_group.hip, gemm_ring2.hip):
// the MFMA operand types and the fp16 two-plane split, the fragment loader, the per-element epilogues, the exchange epilogue
// (training-mode BatchNorm inside the producing GEMM) and the XCD-aware tile map.  Everything here is __device__ __forceinline__;
// the interface a launch is told (GemmArgs) is gemm.h.
#pragma once
#include "gemm.h"
#include <cstdint>
#include <type_traits>
#include <utility>

namespace lipasr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// eight consecutive-k fp32 operand values of a lane -> one bf16 fragment (lane (r, h) holds k = 8 h + j, j < 8)
__device__ __forceinline__ bf16x8 to_bf16x8(const float (&v)[8]) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
  return o;
}

// Arithmetic mode 2 (round 5): fp32-accurate products on the fp16 matrix instruction.  Each operand value x (scaled by a power of two
// that keeps it inside fp16's range) is split into two fp16 planes, hi = RNE(x) and lo = RNE(x - hi) (v_fma_mix: the subtraction
// reads hi as fp16), and a product is hi hi + hi lo + lo hi accumulated in fp32: products of fp16 numbers are exact in fp32, what
// is lost is the 2^-22 of the two-plane representation and the lo lo term -- the technique of the resampler and the block-DFT
// STFT (resample.hip, stft_bdft.hip), with three v_mfma_f32_32x32x16_f16 of 32 cycles per 16-deep chunk in place of eight
// v_mfma_f32_32x32x2_f32 of 64.  The low plane is ONE asm statement ending in s_nop 1 (a vector-ALU result needs two wait states
// before a matrix instruction reads it, and the hazard recogniser does not look inside inline asm).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
// UNIT: the operand runs unscaled (activations): hi by v_cvt_pk_f16_f32, 12 vector instructions per 8 values.  Otherwise the power-of-two
// scale rides in the conversions themselves, hi = f16(x s + 0) and lo = f16(x s - hi) on v_fma_mix (the scale from an SGPR): 16
// instructions.  (The first version multiplied in front of a run-time `scale != 1` test, which the compiler turned into a multiply
// AND two selects per pair of values: ~26 instructions per split, and the ring kernels are bound by vector-instruction issue.)
template <bool UNIT>
__device__ __forceinline__ void split8(const float (&x)[8], const float scale, f16x8& hi, f16x8& lo) {
  unsigned h[4], l[4];
  if constexpr (UNIT) {
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2v){x[2 * i], x[2 * i + 1]}, f16x2v));
    asm("v_fma_mixlo_f16 %0, %4, 1.0, -%12 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %1, %6, 1.0, -%13 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %2, %8, 1.0, -%14 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %3, %10, 1.0, -%15 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %5, 1.0, -%12 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %7, 1.0, -%13 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %2, %9, 1.0, -%14 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %3, %11, 1.0, -%15 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(l[0]), "=&v"(l[1]), "=&v"(l[2]), "=&v"(l[3])
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]));
  } else {
    const float s = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, scale)));  // (wave-uniform by construction)
    asm("v_fma_mixlo_f16 %0, %8, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %10, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %2, %12, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %3, %14, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %9, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %11, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %2, %13, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %3, %15, %16, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %4, %8, %16, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %5, %10, %16, -%1 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %6, %12, %16, -%2 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %7, %14, %16, -%3 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %4, %9, %16, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %5, %11, %16, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %6, %13, %16, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %7, %15, %16, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(h[0]), "=&v"(h[1]), "=&v"(h[2]), "=&v"(h[3]), "=&v"(l[0]), "=&v"(l[1]), "=&v"(l[2]), "=&v"(l[3])
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]), "s"(s));
  }
  hi = __builtin_bit_cast(f16x8, make_uint4(h[0], h[1], h[2], h[3]));
  lo = __builtin_bit_cast(f16x8, make_uint4(l[0], l[1], l[2], l[3]));
}
// one 16-deep chunk: acc += a b on three fp16 matrix instructions
template <bool UA = false>  // UA: the A operand is unscaled (sa == 1: activations)
__device__ __forceinline__ f32x16 mfma_split(const float (&a)[8], const float (&b)[8], const float sa, const float sb, f32x16 acc) {
  f16x8 ah, al, bh, bl;
  split8<UA>(a, sa, ah, al);
  split8<false>(b, sb, bh, bl);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  return acc;
}

// AMODE/BMODE 0: K contiguous in memory (operand(i,k) = P[i*ld + k]); 1: K strided (P[k*ld + i]).
template <int MODE>
__device__ __forceinline__ void load_frag(const float* __restrict__ P, int ld, int idx, int kb, int K, bool vec,
                                          float (&f)[8], bool ones = false) {
  if (MODE == 0) {
    const float* p = P + (size_t)idx * ld + kb;
    if (vec && kb + 8 <= K) {
      const float4 lo = *reinterpret_cast<const float4*>(p);
      const float4 hi = *reinterpret_cast<const float4*>(p + 4);
      f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
      f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = (kb + q < K) ? p[q] : 0.0f;
    }
  } else {
    if (ones) {
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = (kb + q < K) ? 1.0f : 0.0f;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = (kb + q < K) ? P[(size_t)(kb + q) * ld + idx] : 0.0f;
    }
  }
}

// One output element: returns the value to store; s1/s2 receive the column statistics of the *_STATS epilogues.
// dm: the element's dropout multiplier, drawn by the caller for its four columns at once (epilogue_dropout4).
__device__ __forceinline__ float epilogue_elem(const GemmArgs& g, float dm, int gm, int gn, float v, float& s1, float& s2) {
  switch (g.epi) {
    case EPI_BIAS:
      return v + g.bias[gn];
    case EPI_BIAS_RELU:
      return relu_keep_nan(v + g.bias[gn]);
    case EPI_BIAS_RELU_STATS: {
      const float a = relu_keep_nan(v + g.bias[gn]);
      s1 = a;
      s2 = a * a;
      return a;
    }
    case EPI_BIAS_RELU_BN: {
      const float a = relu_keep_nan(v + g.bias[gn]);
      if (g.aux) g.aux[(size_t)gm * g.ldc + gn] = a;
      if (g.gamma) return (a - g.mmean[gn]) / sqrtf(g.mvar[gn] + kBnEps) * g.gamma[gn] + g.beta[gn];
      return a;
    }
    case EPI_DZ_INFER: {
      const float s = g.gamma ? g.gamma[gn] / sqrtf(g.mvar[gn] + kBnEps) : 1.0f;
      return relu_mask_keep_nan(g.aux[(size_t)gm * g.ldc + gn], v * s);
    }
    case EPI_DH_STATS: {
      const size_t e = (size_t)gm * g.ldc + gn;
      const float gg = v * dm;
      const float xh = (g.aux[e] - g.save_mean[gn]) * g.save_mean[g.N + gn];
      s1 = gg;
      s2 = gg * xh;
      return gg;
    }
    case EPI_DZ_NOBN: {
      const size_t e = (size_t)gm * g.ldc + gn;
      return relu_mask_keep_nan(g.aux[e], v * dm);
    }
    case EPI_SIGNSTEP: {
      const size_t i = (size_t)gm * g.ldc + gn;
      const float sg = (v > 0.0f) ? 1.0f : ((v < 0.0f) ? -1.0f : 0.0f);  // NaN -> 0, as ART zeroes NaN gradients
      const float x0 = g.x0[i];
      const float xa = g.x_adv[i] + g.alpha * sg;
      if (isinf(g.eps)) return xa;
      return x0 + fminf(fmaxf(xa - x0, -g.eps), g.eps);
    }
    default:
      return v;
  }
}

// the dropout multipliers of the row's four columns gn .. gn + 3 for the two epilogues that apply them (1 for every other one)
__device__ __forceinline__ void epilogue_dropout4(const GemmArgs& g, int step, int gm, int gn, float (&dm)[4]) {
  if (g.epi == EPI_DH_STATS || g.epi == EPI_DZ_NOBN) {
    dropout_mult4(g.drop, step, gm, g.ldc, gn, g.N, dm);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) dm[e] = 1.0f;
  }
}

// ---------------------------------------------------------------------------------------------
// Round 5: the exchange epilogue.  Training-mode BatchNorm needs column statistics over ALL rows of the batch, i.e. over
// every row tile of a column block; until round 4 the GEMM left per-tile partial sums and a second kernel (bn_apply_*) summed
// them and transformed the tile -- a launch boundary plus a cold round trip for the activations it had just written
// (8.4 / 5.9 us per layer and direction, 72 us of a 352 us step).  Here the row tiles of one column block exchange their
// partial sums inside the launch and every tile finishes its own BatchNorm on the values it still holds in registers:
//   * each tile publishes its 2 x CB partial sums as 8-byte {tag, value} granules (one sc1 store each: the data is the flag),
//   * sweeps the granules of the block's other row tiles until every tag equals this launch's tag (relaxed sc1 loads; the
//     sums are then added in a fixed order in fp64: bitwise reproducible, no float atomics),
//   * and arrives on the block's counter; the last arriver resets it and advances the block's generation, so the next launch
//     (ordered behind this one by the stream) uses the next tag.  Every workgroup reads the generation before it publishes,
//     and the generation cannot move before every workgroup of the block has arrived: all of them use the same tag.
// Needs every workgroup of a column block resident at the same time: the host takes this path only when the whole grid fits
// the CUs the plan's stream may use (bnx_fits), and the sweep is bounded by a wall-clock limit that sets an error word and
// lets the grid drain.  scratch/link_bench.hip (c) prices the exchange alone: 3.7 us (16 row tiles) to 5.5-6.9 us (32).
// ---------------------------------------------------------------------------------------------
struct XcView {
  unsigned long long* gran;
  unsigned* ctrl;
  int* err;
  int rt_max;
};
constexpr long long kXcTimeoutTicks = 200000000LL;  // 2 s of the 100 MHz wall clock
#ifndef LIPASR_XC_POLL_SLEEP
#define LIPASR_XC_POLL_SLEEP 6  // s_sleep units (64 cycles) between two reads of the `published` word by the one polling lane (16 / 6 / 2 measured: config 3 0.3526 / 0.3483 / 0.3490, config 2 0.3109 / 0.3104 / 0.3102)
#endif

// NT threads; CB columns per block (32: the fragment kernel, 64: the LDS-tiled kernel).  mine[2 CB]: this tile's partial sums
// (LDS).  On return tot[2 CB] (LDS, fp64) holds the sums over all n_rt row tiles.  sbuf: LDS, (NT / (2 CB)) x 2 CB doubles.
// this launch's tag for column block bx: the block's generation + 1.  Read at the START of the kernel (the round trip hides behind
// the K loop; any time before this workgroup's own arrival is early enough: the generation cannot move before every row tile
// of the block has arrived)
template <int CB>
__device__ __forceinline__ unsigned xc_tag(const XcView& xc, int bx) {
  return __hip_atomic_load(xc.ctrl + (size_t)bx * (CB / 32) * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
}

// `mid`: work of every thread that does not depend on the exchange (the forward pass's store of the post-ReLU activations), run
// while lane 0 waits for the block's other row tiles -- in front of the publish it would sit in the drain the counter waits for
template <int NT, int CB, typename Mid>
__device__ __forceinline__ void xc_exchange(const XcView& xc, int bx, int by, int n_rt, const unsigned want, const float* mine, double* sbuf,
                                            double* tot, Mid mid) {
  constexpr int NI = 2 * CB, PER = NT / NI, MAXK = 64 / PER;
  typedef unsigned long long u64;
  const int tid = threadIdx.x, item = tid % NI, rl = tid / NI;
  const int jblk = bx * (CB / 32);
  unsigned* cw = xc.ctrl + (size_t)jblk * 32;
  u64* g = xc.gran + (size_t)jblk * xc.rt_max * 128;
  if (tid < NI)
    __hip_atomic_store(g + (size_t)by * 128 + tid, ((u64)want << 32) | (u64)__float_as_uint(mine[tid]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // Waiting quietly: the granules carry their own tags, but a workgroup that swept them over and over while the block's other row
  // tiles still computed put 16 KB of sc1 loads on the fabric every 1.5 us -- with 256 tiles on 160 CUs (two rounds) the first
  // round's workgroups polled through the whole second round and the launch took 58 us instead of 36 + 6 (round 5; the guide's
  // polling-cost row).  So a tile counts itself on the block's `published` word once its granule stores have drained, ONE lane
  // polls that word with a pause between reads, and the granules are swept ONCE when it says every row tile is there.
  // (Measured against it: the count without the drain and a sweep that repeats on an old tag -- config 2 0.3409 against 0.3352 ms,
  // config 3 0.404 against 0.400: the repeated sweeps cost more than the drain.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_fetch_add(cw + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  mid();
  if (tid == 0 && n_rt > 0) {
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(cw + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)n_rt) {
      __builtin_amdgcn_s_sleep(LIPASR_XC_POLL_SLEEP);
      if (wall_clock64() - t0 > kXcTimeoutTicks) { __hip_atomic_store(xc.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
    }
  }
  __syncthreads();
  float v[MAXK];
  {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      const int t = rl + PER * k;
      v[k] = 0.0f;
      if (t < n_rt) {
        const u64 x = __hip_atomic_load(g + (size_t)t * 128 + item, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = ok && (unsigned)(x >> 32) == want;
        v[k] = __uint_as_float((unsigned)x);
      }
    }
    if (!ok) __hip_atomic_store(xc.err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a tag that is not this launch's: never expected
  }
  // arrive now: the returning atomic's round trip runs beside the sums, the normalisation and the stores below
  unsigned old = 0;
  if (tid == 0) old = __hip_atomic_fetch_add(cw + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) s += (double)v[k];  // (slots past n_rt hold 0)
  sbuf[rl * NI + item] = s;
  __syncthreads();
  if (tid < NI) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < PER; ++r) t += sbuf[r * NI + tid];
    tot[tid] = t;
  }
  if (tid == 0 && old == (unsigned)n_rt - 1u) {  // the last row tile of the block: nobody reads the generation or polls any more in this launch
    __hip_atomic_store(cw + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cw + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cw, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
}

// BatchNorm element arithmetic shared by the apply kernels and the exchange epilogues
__device__ __forceinline__ void bn_col_stats(double s1, double s2, int Bstat, float& mean, float& var, float& rstd) {
  const double m = s1 / (double)Bstat;
  double v = s2 / (double)Bstat - m * m;
  v = v > 0.0 ? v : 0.0;
  mean = (float)m;
  var = (float)v;
  rstd = (float)(1.0 / sqrt(v + (double)kBnEps));
}

// The tile's R rows x 4 columns per thread after the exchange.  val: a (forward) or g (backward); av: post-ReLU a (backward).
// colp (LDS floats): forward [mean | rstd] per column of the block, backward [dbeta | dgamma].
// The per-column operands of bnx_finish that do not depend on the exchange (forward gamma / beta, backward gamma and the saved mean /
// rstd): requested BEFORE the exchange, so that their round trip runs beside its waits instead of behind them
struct BnxLate {
  float ga[4], b0[4], b1[4];  // forward: gamma, beta, -; backward: gamma, saved mean, saved rstd
};
__device__ __forceinline__ void bnx_late_load(const GemmArgs& g, const int gn, BnxLate& q) {
  const bool fwd = g.epi == EPI_BIAS_RELU_BNX;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cv = gn + e < g.N;
    q.ga[e] = cv ? g.gamma[gn + e] : 1.0f;
    if (fwd) {
      q.b0[e] = cv ? g.beta[gn + e] : 0.0f;
      q.b1[e] = 0.0f;
    } else {
      q.b0[e] = cv ? g.save_mean[gn + e] : 0.0f;
      q.b1[e] = cv ? g.save_mean[g.N + gn + e] : 1.0f;
    }
  }
}

template <int R>
__device__ __forceinline__ void bnx_finish(const GemmArgs& g, const int step, const int* gm, const int gn, const float (*val)[4],
                                           const float (*av)[4], const float* colp, const int CB, const int c4, const BnxLate& lt) {
  const bool fwd = g.epi == EPI_BIAS_RELU_BNX;
  float ga[4], p0[4], p1[4], be[4], mean[4], rstd[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ga[e] = lt.ga[e];
    p0[e] = colp[c4 + e];
    p1[e] = colp[CB + c4 + e];
    if (fwd) {
      be[e] = lt.b0[e];
      mean[e] = p0[e]; rstd[e] = p1[e];
    } else {
      be[e] = 0.0f;
      mean[e] = lt.b0[e];
      rstd[e] = lt.b1[e];
    }
  }
  const float invB = 1.0f / (float)g.Bstat;
  float omax = 0.0f;  // backward: max |dz| of this thread (arithmetic mode 2 scales the consumers' operand by it)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (gm[r] >= g.M) continue;
    float o[4], dm[4];
    if (fwd) dropout_mult4(g.drop, step, gm[r], g.ldc, gn, g.N, dm);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (fwd) {
        float x = (val[r][e] - mean[e]) * rstd[e] * ga[e] + be[e];
        x *= dm[e];
        o[e] = x;
      } else {
        const float xh = (av[r][e] - mean[e]) * rstd[e];
        const float d = ga[e] * rstd[e] * (val[r][e] - p0[e] * invB - xh * p1[e] * invB);
        o[e] = relu_mask_keep_nan(av[r][e], d);
        if (gn + e < g.N) omax = fmaxf(omax, fabsf(o[e]));
      }
    }
    float* crow = (fwd ? g.h_out : g.C) + (size_t)gm[r] * g.ldc;
    if (gn + 3 < g.N && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(crow) & 15) == 0)) {
      *reinterpret_cast<float4*>(crow + gn) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (gn + e < g.N) crow[gn + e] = o[e];
    }
  }
  if (!fwd && g.amax_out) amax_publish(g.amax_out, omax);  // (every thread of the wavefront reaches this point)
}

// one column of the block after the exchange: forward -> [mean | rstd] (+ moving statistics and the saved statistics, by
// row tile 0), backward -> [dbeta | dgamma] (+ the parameter gradients, by row tile 0)
// (mm0, mv0: the column's moving statistics, requested by row tile 0 before the exchange -- bnx_moving_load)
__device__ __forceinline__ void bnx_moving_load(const GemmArgs& g, const int by, const int col, const bool mine, float& mm0, float& mv0) {
  mm0 = 0.0f; mv0 = 0.0f;
  if (mine && g.epi == EPI_BIAS_RELU_BNX && by == 0 && col < g.N) { mm0 = g.mmean_w[col]; mv0 = g.mvar_w[col]; }
}
__device__ __forceinline__ void bnx_column(const GemmArgs& g, const int by, const int col, const int j, const int CB, const double* tot,
                                           float* colp, const float mm0, const float mv0) {
  if (g.epi == EPI_BIAS_RELU_BNX) {
    float mean, var, rstd;
    bn_col_stats(tot[j], tot[CB + j], g.Bstat, mean, var, rstd);
    colp[j] = mean;
    colp[CB + j] = rstd;
    if (by == 0 && col < g.N) {
      g.mmean_w[col] = mm0 * kBnMomentum + mean * (1.0f - kBnMomentum);
      g.mvar_w[col] = mv0 * kBnMomentum + var * (1.0f - kBnMomentum);
      g.save_w[col] = mean;
      g.save_w[g.N + col] = rstd;
    }
  } else {
    const float dbt = (float)tot[j], dg = (float)tot[CB + j];
    colp[j] = dbt;
    colp[CB + j] = dg;
    if (by == 0 && col < g.N) {
      g.dbeta[col] = dbt * g.grad_scale;
      g.dgamma[col] = dg * g.grad_scale;
    }
  }
}

// The per-element operands of the exchange epilogue, requested BEFORE the K-split partial tiles meet in LDS (their round trip
// runs beside that barrier): forward the bias, backward the post-ReLU activation and the column's saved mean / rstd.
struct BnxPre {
  float p0[4], p1[4], p2[4];
};
__device__ __forceinline__ void bnx_prefetch(const GemmArgs& g, const int gm, const int gn, BnxPre& q) {
  const bool rv = gm < g.M;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool cv = rv && gn + e < g.N;
    if (g.epi == EPI_BIAS_RELU_BNX) {
      q.p0[e] = cv ? g.bias[gn + e] : 0.0f;
      q.p1[e] = 0.0f; q.p2[e] = 0.0f;
    } else {
      q.p0[e] = cv ? g.aux[(size_t)gm * g.ldc + gn + e] : 0.0f;
      q.p1[e] = cv ? g.save_mean[gn + e] : 0.0f;
      q.p2[e] = cv ? g.save_mean[g.N + gn + e] : 0.0f;
    }
  }
}

// one row's four columns before the exchange: values kept in registers, their two statistics each (rv: the row is inside M)
__device__ __forceinline__ void bnx_row4(const GemmArgs& g, const int step, const bool rv, const int gm, const int gn, const float (&acc)[4],
                                         const BnxPre& q, float (&val)[4], float (&av)[4], float (&s1)[4], float (&s2)[4]) {
  if (g.epi == EPI_BIAS_RELU_BNX) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = (rv && gn + e < g.N) ? relu_keep_nan(acc[e] + q.p0[e]) : 0.0f;
      val[e] = a; av[e] = a; s1[e] = a; s2[e] = a * a;
    }
  } else {
    float dm[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (rv) dropout_mult4(g.drop, step, gm, g.ldc, gn, g.N, dm);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool cv = rv && gn + e < g.N;
      const float gg = cv ? acc[e] * dm[e] : 0.0f;
      const float a = q.p0[e];
      const float xh = cv ? (a - q.p1[e]) * q.p2[e] : 0.0f;
      val[e] = gg; av[e] = a; s1[e] = gg; s2[e] = gg * xh;
    }
  }
}

// XCD-aware workgroup -> tile map (speed only; nothing depends on where a workgroup really runs).  Workgroups are dealt
// round-robin over the 8 XCDs by their linear id, each XCD has its own 4 MiB L2.  With the plain map (bx = id % ntx) XCD x gets the
// column tiles x and x + 8 of EVERY row tile: it reads the whole A operand (3.6-4 MB for the 1024-row layers: its entire L2) and
// an eighth of B.  Here the workgroups of one XCD (ids = x mod 8) take a compact gx x gy patch of the tile grid instead, e.g.
// 8 x 4 tiles of the 16 x 16 grid of layer 1: a quarter of A and half of B, 2.7 MB, so both operands stay in that L2.
// Bijective whenever it applies (ntx divisible by gx, nty by gy); otherwise the plain map.
__device__ __forceinline__ void xcd_tile(const int L, const int ntx, const int nty, int& bx, int& by) {
  // Any grid (round 5; the first version needed ntx, nty divisible by the patch counts, and the 8 x 7 grid of 128-wide weight-gradient
  // tiles fell to "one column of tiles per XCD": seven A panels + one B panel = 4 MB, the whole L2).  The tiles are put in a BLOCKED
  // order -- row groups of height h, inside a group column by column -- and the 8 XCDs take consecutive runs of that order; XCD x runs
  // the workgroups L = x (mod 8) in sequence, so its q-th workgroup takes the q-th tile of its run.  h ~ sqrt(run) makes a run
  // roughly square: about 2 sqrt(run) operand panels instead of run + 1.
  const int total = ntx * nty;
  if (total < 16) { bx = L % ntx; by = L / ntx; return; }
  const int xcd = L & 7, q = L >> 3, base = total >> 3, rem = total & 7;
  const int t = xcd * base + min(xcd, rem) + q;            // position in the blocked order
  int h = (int)(sqrtf((float)(base + (rem ? 1 : 0))) + 0.5f);
  h = max(1, min(h, nty));
  const int per_group = h * ntx, grp = t / per_group, u = t - grp * per_group;
  const int hg = min(h, nty - grp * h);                     // height of this (maybe last, shorter) group
  bx = u / hg;
  by = grp * h + (u - bx * hg);
}

}  // namespace lipasr
