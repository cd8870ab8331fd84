// K2: the dense classifier's GEMMs on fp32 / bf16 / fp16 MFMA (gfx950): the tile kernels, the choice of one for a problem
// (pick_gemm) and the launchers.  The interface is gemm.h; the BatchNorm / dropout / softmax-CE kernels and the plan-level
// forward / backward / predict / attack sequences that call these launchers are mlp.hip.
//
// GEMM design (v_mfma_f32_32x32x2_f32, exact fp32 fma chains):
//   The classifier's GEMMs are small (M = batch 512..1024, N <= 1024, K <= 1024): with one 32x32
//   accumulator per wavefront the time of a tile is (K/2) MFMAs * 64 cycles whatever M and N are,
//   so the lever is K, not the tile.  One workgroup = one 32x32 output tile, its 4 wavefronts split
//   K four ways (16-deep chunks, round-robin), operands go straight from global/L2 to VGPRs in MFMA
//   layout (no LDS staging, no barrier in the main loop, next chunk prefetched behind the MFMAs),
//   the four partial tiles meet in LDS once and 256 threads run the fused epilogue with float4
//   stores.  K order inside a chunk is permuted (lane half h takes k0+8h..k0+8h+7) so that
//   K-contiguous operands load as two float4 per lane; both operands use the same permutation.
//
//   Epilogues fuse: bias (+ReLU), inference BatchNorm affine, the ReLU/BN backward mask of the
//   inference-mode input gradient, and the FGSM/PGD sign step (K4) on the last backward GEMM.
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
__device__ __forceinline__ float epilogue_elem(const GemmArgs& g, int step, int gm, int gn, float v, float& s1, float& s2) {
  switch (g.epi) {
    case EPI_BIAS:
      return v + g.bias[gn];
    case EPI_BIAS_RELU:
      return fmaxf(v + g.bias[gn], 0.0f);
    case EPI_BIAS_RELU_STATS: {
      const float a = fmaxf(v + g.bias[gn], 0.0f);
      s1 = a;
      s2 = a * a;
      return a;
    }
    case EPI_BIAS_RELU_BN: {
      const float a = fmaxf(v + g.bias[gn], 0.0f);
      if (g.aux) g.aux[(size_t)gm * g.ldc + gn] = a;
      if (g.gamma) return (a - g.mmean[gn]) / sqrtf(g.mvar[gn] + kBnEps) * g.gamma[gn] + g.beta[gn];
      return a;
    }
    case EPI_DZ_INFER: {
      const float s = g.gamma ? g.gamma[gn] / sqrtf(g.mvar[gn] + kBnEps) : 1.0f;
      return g.aux[(size_t)gm * g.ldc + gn] > 0.0f ? v * s : 0.0f;
    }
    case EPI_DH_STATS: {
      const size_t e = (size_t)gm * g.ldc + gn;
      const float gg = v * dropout_mult(g.drop, step, e);
      const float xh = (g.aux[e] - g.save_mean[gn]) * g.save_mean[g.N + gn];
      s1 = gg;
      s2 = gg * xh;
      return gg;
    }
    case EPI_DZ_NOBN: {
      const size_t e = (size_t)gm * g.ldc + gn;
      return g.aux[e] > 0.0f ? v * dropout_mult(g.drop, step, e) : 0.0f;
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
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t idx = (size_t)gm[r] * g.ldc + gn + e;
      if (fwd) {
        float x = (val[r][e] - mean[e]) * rstd[e] * ga[e] + be[e];
        x *= (gn + e < g.N) ? dropout_mult(g.drop, step, idx) : 0.0f;
        o[e] = x;
      } else {
        const float xh = (av[r][e] - mean[e]) * rstd[e];
        const float d = ga[e] * rstd[e] * (val[r][e] - p0[e] * invB - xh * p1[e] * invB);
        o[e] = av[r][e] > 0.0f ? d : 0.0f;
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

// the element before the exchange: value kept in registers, its two statistics
__device__ __forceinline__ void bnx_elem(const GemmArgs& g, const int step, const bool cv, const int gm, const int gn, const float acc,
                                         const BnxPre& q, const int e, float& val, float& av, float& s1, float& s2) {
  if (g.epi == EPI_BIAS_RELU_BNX) {
    const float a = cv ? fmaxf(acc + q.p0[e], 0.0f) : 0.0f;
    val = a; av = a; s1 = a; s2 = a * a;
  } else {
    const size_t idx = (size_t)gm * g.ldc + gn;
    const float gg = cv ? acc * dropout_mult(g.drop, step, idx) : 0.0f;
    const float a = q.p0[e];
    const float xh = cv ? (a - q.p1[e]) * q.p2[e] : 0.0f;
    val = gg; av = a; s1 = gg; s2 = gg * xh;
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

// One workgroup = one 32x32 output tile; its NW wavefronts (4, or 16 for small outputs with a long K) split K
// in 16-deep chunks, round-robin.  Operand fragments go global/L2 -> VGPR directly, one chunk ahead of the MFMAs.
template <int AMODE, int BMODE, int NW, int BF, bool X = false>  // X: the exchange epilogue (its own instances: with it as a run-time
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, const int bx, const int by, const int n_row_tiles) {  // branch every GEMM grew from 50-66 to 83 VGPRs)
  constexpr int TS = 32;
  constexpr int TPR = 8;                       // threads per output row (one float4 each)
  extern __shared__ __attribute__((aligned(16))) float red[];  // [NW][32][32] + stats [4][8][8]
  float* stat = red + NW * TS * TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int m0 = by * TS, n0 = bx * TS;
  const int nch = (g.K + 15) >> 4;
  const bool vecA = (AMODE == 0) && ((g.lda & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.A) & 15) == 0);
  const bool vecB = (BMODE == 0) && ((g.ldb & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.B) & 15) == 0);
  const int m_real = g.ones_row ? g.M - 1 : g.M;  // rows of op(A) that exist in memory
  const int row_a = m0 + r;
  const bool aones = (AMODE == 1) && g.ones_row && (row_a == g.M - 1);
  const int ai = min(row_a, m_real - 1);
  const int bj = min(n0 + r, g.N - 1);

  unsigned xtag = 0;
  if constexpr (X) xtag = xc_tag<32>(XcView{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max}, bx);
  float rsa = 1.0f, rsb = 1.0f;
  if (BF == 2) { rsa = scale_from_amax(g.sa_dyn, g.sa); rsb = scale_from_amax(g.sb_dyn, g.sb); }
  if (g.amax_zero && bx == 0 && by == 0) amax_clear(g.amax_zero);
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  float a0[8], b0[8], a1[8], b1[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) { a0[q] = b0[q] = a1[q] = b1[q] = 0.0f; }
  // one chunk of loads in flight behind the MFMAs (two measured slower: config 2 0.384 -> 0.390 ms, config 5 +4 %)
  int c = wave;
  if (c < nch) {
    load_frag<AMODE>(g.A, g.lda, ai, c * 16 + 8 * h, g.K, vecA, a0, aones);
    load_frag<BMODE>(g.B, g.ldb, bj, c * 16 + 8 * h, g.K, vecB, b0);
  }
  while (c < nch) {
    const int cn = c + NW;
    if (cn < nch) {
      load_frag<AMODE>(g.A, g.lda, ai, cn * 16 + 8 * h, g.K, vecA, a1, aones);
      load_frag<BMODE>(g.B, g.ldb, bj, cn * 16 + 8 * h, g.K, vecB, b1);
    }
    if (BF == 1) {
      // the chunk's 16 k values are exactly one 32x32x16 bf16 fragment per operand (same lane map as the loads)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(to_bf16x8(a0), to_bf16x8(b0), acc, 0, 0, 0);
    } else if (BF == 2) {
      acc = mfma_split(a0, b0, rsa, rsb, acc);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], b0[q], acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) { a0[q] = a1[q]; b0[q] = b1[q]; }
    c = cn;
  }
  if (BF == 2) {
    const float un = 1.0f / (rsa * rsb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] *= un;
  }
  BnxPre xpre;
  if constexpr (X && NW == 4) bnx_prefetch(g, m0 + (tid >> 3), n0 + (tid & 7) * 4, xpre);
  // C/D map of one 32x32 accumulator: col = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
    red[wave * TS * TS + row * TS + r] = acc[q];
  }
  __syncthreads();

  if constexpr (X && NW == 4) {
    {
      const int step = g.drop.step_dev ? *g.drop.step_dev : 0;
      const int tcol = tid & 7, row = tid >> 3, c4 = tcol * 4, gn = n0 + c4;
      const int gm1[1] = {m0 + row};
      float4 s = *reinterpret_cast<const float4*>(red + row * TS + c4);
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float4 t = *reinterpret_cast<const float4*>(red + w * TS * TS + row * TS + c4);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
      const float accv[4] = {s.x, s.y, s.z, s.w};
      float val[1][4], av[1][4], c1[4], c2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) bnx_elem(g, step, gm1[0] < g.M && gn + e < g.N, gm1[0], gn + e, accv[e], xpre, e, val[0][e], av[0][e], c1[e], c2[e]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = TPR; o < 64; o <<= 1) {
          c1[e] += __shfl_xor(c1[e], o, 64);
          c2[e] += __shfl_xor(c2[e], o, 64);
        }
      }
      if (lane < TPR) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          stat[(wave * TPR + lane) * 8 + e] = c1[e];
          stat[(wave * TPR + lane) * 8 + 4 + e] = c2[e];
        }
      }
      __syncthreads();  // (also: every read of `red` is done, it is carved up below)
      float* mine = red;                                       // [2][32]
      float* colp = red + 64;                                  // [2][32]
      double* sbuf = reinterpret_cast<double*>(red + 128);     // [4][64]
      double* tot = sbuf + 4 * 64;                             // [64]
      if (tid < 2 * TS) {
        const int which = tid / TS, col = tid % TS, l4 = col >> 2, e = col & 3;
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) t += stat[(w * TPR + l4) * 8 + which * 4 + e];
        mine[tid] = t;
      }
      __syncthreads();
      BnxLate late;
      bnx_late_load(g, gn, late);
      float mm0, mv0;
      bnx_moving_load(g, by, n0 + tid, tid < TS, mm0, mv0);
      XcView xc{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max};
      xc_exchange<256, 32>(xc, bx, by, g.Bstat < 0 ? 0 : n_row_tiles, xtag, mine, sbuf, tot, [&]() {  // (Bstat < 0: timing probe, below)
        if (g.epi == EPI_BIAS_RELU_BNX && gm1[0] < g.M) {  // the post-ReLU activations: the backward pass reads them
          float* crow = g.C + (size_t)gm1[0] * g.ldc;
          if (gn + 3 < g.N && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(crow) & 15) == 0)) {
            *reinterpret_cast<float4*>(crow + gn) = make_float4(val[0][0], val[0][1], val[0][2], val[0][3]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (gn + e < g.N) crow[gn + e] = val[0][e];
          }
        }
      });
      if (tid < TS) bnx_column(g, by, n0 + tid, tid, TS, tot, colp, mm0, mv0);
      __syncthreads();
      bnx_finish<1>(g, step, gm1, gn, val, av, colp, TS, c4, late);
      return;
    }
  }

  const bool stats = (g.epi == EPI_BIAS_RELU_STATS) || (g.epi == EPI_DH_STATS);
  float cs1[4] = {0.f, 0.f, 0.f, 0.f}, cs2[4] = {0.f, 0.f, 0.f, 0.f};
  if (tid < 256) {
    const int step = g.drop.step_dev ? *g.drop.step_dev : 0;
    const int tcol = tid & 7, row = tid >> 3;
    const int c4 = tcol * 4;
    const int gn = n0 + c4;
    float4 s = *reinterpret_cast<const float4*>(red + row * TS + c4);
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const float4 t = *reinterpret_cast<const float4*>(red + w * TS * TS + row * TS + c4);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    const int gm = m0 + row;
    if (g.epi == EPI_BIAS_SOFTMAX_CE) {
      // the row's (<= 32) logits sit in the 8 consecutive lanes that share `row`: butterfly over lane bits 0..2.
      // Same definitions as softmax_ce_kernel (first maximum wins ties); every lane takes part in the shuffles.
      const bool rv = gm < g.M;
      float z[4];
      float mx = -INFINITY;
      int am = 0x7fffffff;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool cv = rv && (gn + e < g.N);
        z[e] = cv ? (&s.x)[e] + g.bias[gn + e] : -INFINITY;
        if (z[e] > mx) { mx = z[e]; am = gn + e; }
      }
#pragma unroll
      for (int o2 = 1; o2 < 8; o2 <<= 1) {
        const float omx = __shfl_xor(mx, o2, 64);
        const int oam = __shfl_xor(am, o2, 64);
        if (omx > mx || (omx == mx && oam < am)) { mx = omx; am = oam; }
      }
      float se = 0.0f;
#pragma unroll
      for (int e = 0; e < 4; ++e) se += (z[e] > -INFINITY) ? expf(z[e] - mx) : 0.0f;
#pragma unroll
      for (int o2 = 1; o2 < 8; o2 <<= 1) se += __shfl_xor(se, o2, 64);
      const float lse = logf(se), inv = 1.0f / se;
      float loss = 0.0f, ymax = -INFINITY;
      int ay = 0x7fffffff;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (rv && gn + e < g.N) {
          const size_t idx = (size_t)gm * g.N + gn + e;
          const float zs = z[e] - mx;
          const float pc = expf(zs) * inv;
          g.C[(size_t)gm * g.ldc + gn + e] = z[e];
          if (g.prob) g.prob[idx] = pc;
          if (g.y) {
            const float yc = g.y[idx];
            if (yc != 0.0f) loss -= yc * (zs - lse);
            if (yc > ymax) { ymax = yc; ay = gn + e; }
            if (g.dz) g.dz[idx] = (pc - yc) * g.inv_batch;
          }
        }
      }
#pragma unroll
      for (int o2 = 1; o2 < 8; o2 <<= 1) {
        loss += __shfl_xor(loss, o2, 64);
        const float oym = __shfl_xor(ymax, o2, 64);
        const int oay = __shfl_xor(ay, o2, 64);
        if (oym > ymax || (oym == ymax && oay < ay)) { ymax = oym; ay = oay; }
      }
      if (rv && tcol == 0) {
        if (g.loss_rows) g.loss_rows[gm] = loss;
        if (g.correct_rows) g.correct_rows[gm] = (am == ay) ? 1.0f : 0.0f;
      }
    } else if (gm < g.M) {
      const float v[4] = {s.x, s.y, s.z, s.w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t1 = 0.0f, t2 = 0.0f;
        o[e] = (gn + e < g.N) ? epilogue_elem(g, step, gm, gn + e, v[e], t1, t2) : 0.0f;
        cs1[e] = t1;
        cs2[e] = t2;
      }
      float* crow;
      if (g.ones_row && gm == g.M - 1) crow = g.extra_out;
      else crow = (g.epi == EPI_SIGNSTEP ? g.x_adv : g.C) + (size_t)gm * g.ldc;
      if (gn + 3 < g.N && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(crow) & 15) == 0)) {
        *reinterpret_cast<float4*>(crow + gn) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gn + e < g.N) crow[gn + e] = o[e];
      }
    }
  }
  if (stats) {
    // column sums over the tile's 32 rows: lanes with equal tcol inside a wavefront (8 rows), then 4 wavefronts
    if (tid < 256) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = TPR; o < 64; o <<= 1) {
          cs1[e] += __shfl_xor(cs1[e], o, 64);
          cs2[e] += __shfl_xor(cs2[e], o, 64);
        }
      }
      if (lane < TPR) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          stat[(wave * TPR + lane) * 8 + e] = cs1[e];
          stat[(wave * TPR + lane) * 8 + 4 + e] = cs2[e];
        }
      }
    }
    __syncthreads();
    if (tid < 2 * TS) {
      const int which = tid / TS, col = tid % TS;
      const int l4 = col >> 2, e = col & 3;
      float t = 0.0f;
#pragma unroll
      for (int w = 0; w < 4; ++w) t += stat[(w * TPR + l4) * 8 + which * 4 + e];
      if (n0 + col < g.N) g.part[((size_t)which * n_row_tiles + by) * g.N + n0 + col] = t;
    }
  }
}

template <int AMODE, int BMODE, int NW, int BF = 0, bool X = false>  // BF: operands rounded to bf16 at the MFMA (compile-time: a
__global__ __launch_bounds__(64 * NW) void gemm_f32_kernel(GemmArgs g) {  // run-time switch cost the fp32 path 6 %)
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_tile<AMODE, BMODE, NW, BF, X>(g, bx, by, gridDim.y);
}


template <int AMODE, int BMODE, int NW, int BF = 0>
__global__ __launch_bounds__(64 * NW) void gemm_f32_grouped_kernel(GemmGroup grp) {
  int p = 0;
  while (p + 1 < grp.n && (int)blockIdx.x >= grp.tile_start[p + 1]) ++p;
  const GemmArgs& g = grp.g[p];
  const int local = blockIdx.x - grp.tile_start[p];
  const int ntx = (g.N + 31) / 32, nty = (g.M + 31) / 32;
  int bx = local % ntx, by = local / ntx;
  if (g.xcd_map && (grp.tile_start[p] & 7) == 0) xcd_tile(local, ntx, nty, bx, by);
  gemm_tile<AMODE, BMODE, NW, BF>(g, bx, by, nty);
}

// ---------------------------------------------------------------------------------------------
// LDS-tiled variant for the large GEMMs: one workgroup (512 threads, 8 wavefronts) = one 64x64 tile.  K advances
// in 32-deep stages through a double-buffered LDS image stored k-major ([k][m] and [k][n], row stride 68
// floats): MFMA operand reads are unit-stride ds_read_b32 (conflict-free) and every operand element is
// fetched from L2 once per workgroup instead of once per 32x32 tile.  Wavefronts 0-3 take k 0..15 of each
// stage for the four 32x32 quadrants, wavefronts 4-7 take k 16..31: two wavefronts per SIMD, so one's LDS
// latency hides behind the other's MFMAs.  Global loads for stage t+1 are issued before the MFMAs of stage t
// and written to the other LDS buffer afterwards: one barrier per stage.  The two K halves meet in LDS.
// ---------------------------------------------------------------------------------------------
constexpr int kLdsBK = 32, kLdsLD = 68;

template <int MODE>  // 0: operand(i,k) = P[i*ld + k] (K contiguous), 1: P[k*ld + i]
__device__ __forceinline__ float4 tile_fetch(const float* __restrict__ P, int ld, int i0, int i_real, int k0, int K,
                                             bool ones_last, int i_last, int tid) {
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  const bool al = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(P) & 15) == 0);
  if (MODE == 0) {
    const int i = i0 + (tid >> 3);                     // 64 rows, 8 float4 (32 k) per row
    const int kq = k0 + (tid & 7) * 4;
    const float* p = P + (size_t)min(i, i_real - 1) * ld + kq;
    if (kq + 3 < K && al) {
      const float4 x = *reinterpret_cast<const float4*>(p);
      t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = (kq + c < K) ? p[c] : 0.0f;
    }
  } else {
    const int k = k0 + (tid >> 4);                     // 32 k rows, 16 float4 (64 i) per row
    const int iq = i0 + (tid & 15) * 4;
    if (k < K) {
      const float* p = P + (size_t)k * ld;
      if (iq + 3 < i_real && al) {
        const float4 x = *reinterpret_cast<const float4*>(p + iq);
        t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = iq + c;
          t[c] = (ones_last && i == i_last) ? 1.0f : p[min(i, i_real - 1)];
        }
      }
    }
  }
  return make_float4(t[0], t[1], t[2], t[3]);
}

template <int MODE>
__device__ __forceinline__ void tile_store(float* __restrict__ S, int tid, const float4 v) {
  if (MODE == 0) {
    const int i = tid >> 3, kq = (tid & 7) * 4;
    S[(kq + 0) * kLdsLD + i] = v.x;
    S[(kq + 1) * kLdsLD + i] = v.y;
    S[(kq + 2) * kLdsLD + i] = v.z;
    S[(kq + 3) * kLdsLD + i] = v.w;
  } else {
    const int k = tid >> 4, iq = (tid & 15) * 4;
    *reinterpret_cast<float4*>(S + k * kLdsLD + iq) = v;
  }
}

constexpr int kLdsBKMax = 32;  // 64-row tiles measured slower (30.4 vs 26.3 us on the 1024x1024x880 GEMM)
constexpr size_t lds_gemm_bytes(int bk) {
  return ((size_t)(2 * 2 * bk * kLdsLD > 2 * 64 * 64 ? 2 * 2 * bk * kLdsLD : 2 * 64 * 64) + 8 * 16 * 8) * sizeof(float);
}

// The epilogue of a 64 x 64 tile held as eight 32 x 32 accumulators (wavefront = (K half, quadrant)): the two K halves meet in LDS
// (`red`: the first 32 KB of the workgroup's dynamic LDS, free by now), then bias / ReLU / statistics / the exchange epilogue /
// stores.  Shared by the LDS-tiled kernel and the LDS-DMA ring kernel.
template <bool X>
__device__ __forceinline__ void lds_tile_epilogue(const GemmArgs& g, const f32x16& acc, float* lds, float* stat, const int bx, const int by,
                                                  const int n_row_tiles, const unsigned xtag) {
  constexpr int TS = 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int kh = wave >> 2, wi = (wave >> 1) & 1, wj = wave & 1;
  const int m0 = by * TS, n0 = bx * TS;
  BnxPre xpre[2];
  if constexpr (X) {
    bnx_prefetch(g, m0 + (tid >> 4), n0 + (tid & 15) * 4, xpre[0]);
    bnx_prefetch(g, m0 + (tid >> 4) + 32, n0 + (tid & 15) * 4, xpre[1]);
  }
  // accumulators -> LDS as two 64x64 partial tiles (one per K half), then the shared epilogue shape
  float* red = lds;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = 32 * wi + (q & 3) + 8 * (q >> 2) + 4 * h;
    red[kh * TS * TS + row * TS + 32 * wj + r] = acc[q];
  }
  __syncthreads();
  const bool stats = (g.epi == EPI_BIAS_RELU_STATS) || (g.epi == EPI_DH_STATS);
  const int step = g.drop.step_dev ? *g.drop.step_dev : 0;
  const int tcol = tid & 15, trow = tid >> 4;
  const int c4 = tcol * 4, gn = n0 + c4;
  if constexpr (X) {
    const int gm2[2] = {m0 + trow, m0 + trow + 32};
    float val[2][4], av[2][4], c1[4] = {0.f, 0.f, 0.f, 0.f}, c2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int row = trow + 32 * pass;
      float4 s = *reinterpret_cast<const float4*>(red + row * TS + c4);
      const float4 s2 = *reinterpret_cast<const float4*>(red + TS * TS + row * TS + c4);
      const float accv[4] = {s.x + s2.x, s.y + s2.y, s.z + s2.z, s.w + s2.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t1, t2;
        bnx_elem(g, step, gm2[pass] < g.M && gn + e < g.N, gm2[pass], gn + e, accv[e], xpre[pass], e, val[pass][e], av[pass][e], t1, t2);
        c1[e] += t1;
        c2[e] += t2;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c1[e] += __shfl_xor(c1[e], 16, 64); c1[e] += __shfl_xor(c1[e], 32, 64);
      c2[e] += __shfl_xor(c2[e], 16, 64); c2[e] += __shfl_xor(c2[e], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        stat[(wave * 16 + lane) * 8 + e] = c1[e];
        stat[(wave * 16 + lane) * 8 + 4 + e] = c2[e];
      }
    }
    __syncthreads();  // (every read of `red` is done: it is carved up below)
    float* mine = red;                                       // [2][64]
    float* colp = red + 128;                                 // [2][64]
    double* sbuf = reinterpret_cast<double*>(red + 256);     // [4][128]
    double* tot = sbuf + 4 * 128;                            // [128]
    if (tid < 2 * TS) {
      const int which = tid / TS, col = tid % TS, l4 = col >> 2, e = col & 3;
      float t = 0.0f;
#pragma unroll
      for (int w = 0; w < 8; ++w) t += stat[(w * 16 + l4) * 8 + which * 4 + e];
      mine[tid] = t;
    }
    __syncthreads();
    BnxLate late;
    bnx_late_load(g, gn, late);
    float mm0, mv0;
    bnx_moving_load(g, by, n0 + tid, tid < TS, mm0, mv0);
    XcView xc{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max};
    xc_exchange<512, 64>(xc, bx, by, g.Bstat < 0 ? 0 : n_row_tiles, xtag, mine, sbuf, tot, [&]() {
      if (g.epi != EPI_BIAS_RELU_BNX) return;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        if (gm2[pass] >= g.M) continue;
        float* crow = g.C + (size_t)gm2[pass] * g.ldc;
        if (gn + 3 < g.N && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(crow) & 15) == 0)) {
          *reinterpret_cast<float4*>(crow + gn) = make_float4(val[pass][0], val[pass][1], val[pass][2], val[pass][3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (gn + e < g.N) crow[gn + e] = val[pass][e];
        }
      }
    });
    if (tid < TS) bnx_column(g, by, n0 + tid, tid, TS, tot, colp, mm0, mv0);
    __syncthreads();
    bnx_finish<2>(g, step, gm2, gn, val, av, colp, TS, c4, late);
    return;
  }
  float cs1[4] = {0.f, 0.f, 0.f, 0.f}, cs2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int row = trow + 32 * pass;
    float4 s = *reinterpret_cast<const float4*>(red + row * TS + c4);
    const float4 s2 = *reinterpret_cast<const float4*>(red + TS * TS + row * TS + c4);
    s.x += s2.x; s.y += s2.y; s.z += s2.z; s.w += s2.w;
    const int gm = m0 + row;
    if (gm < g.M) {
      const float v[4] = {s.x, s.y, s.z, s.w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t1 = 0.0f, t2 = 0.0f;
        o[e] = (gn + e < g.N) ? epilogue_elem(g, step, gm, gn + e, v[e], t1, t2) : 0.0f;
        cs1[e] += t1;
        cs2[e] += t2;
      }
      float* crow;
      if (g.ones_row && gm == g.M - 1) crow = g.extra_out;
      else crow = (g.epi == EPI_SIGNSTEP ? g.x_adv : g.C) + (size_t)gm * g.ldc;
      if (gn + 3 < g.N && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(crow) & 15) == 0)) {
        *reinterpret_cast<float4*>(crow + gn) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gn + e < g.N) crow[gn + e] = o[e];
      }
    }
  }
  if (stats) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      cs1[e] += __shfl_xor(cs1[e], 16, 64); cs1[e] += __shfl_xor(cs1[e], 32, 64);
      cs2[e] += __shfl_xor(cs2[e], 16, 64); cs2[e] += __shfl_xor(cs2[e], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        stat[(wave * 16 + lane) * 8 + e] = cs1[e];
        stat[(wave * 16 + lane) * 8 + 4 + e] = cs2[e];
      }
    }
    __syncthreads();
    if (tid < 2 * TS) {
      const int which = tid / TS, col = tid % TS;
      const int l4 = col >> 2, e = col & 3;
      float t = 0.0f;
#pragma unroll
      for (int w = 0; w < 8; ++w) t += stat[(w * 16 + l4) * 8 + which * 4 + e];
      if (n0 + col < g.N) g.part[((size_t)which * n_row_tiles + by) * g.N + n0 + col] = t;
    }
  }
}


template <int AMODE, int BMODE, int BF, int BK, bool X = false>  // BK: k rows per LDS tile (32 or 64); X: the exchange epilogue
__device__ __forceinline__ void gemm_lds_tile(const GemmArgs& g, const int bx, const int by, const int n_row_tiles) {
  constexpr int TS = 64;
  constexpr int NF = BK / kLdsBK;  // 32-row fetches per operand and tile
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [buf][A|B][BK][68]; reused as [2][64][64]; then stat
  float* stat = lds + (2 * 2 * BK * kLdsLD > 2 * 64 * 64 ? 2 * 2 * BK * kLdsLD : 2 * 64 * 64);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int kh = wave >> 2, wi = (wave >> 1) & 1, wj = wave & 1;
  const int m0 = by * TS, n0 = bx * TS;
  const int m_real = g.ones_row ? g.M - 1 : g.M;
  const int nst = (g.K + BK - 1) / BK;
  const bool ones = g.ones_row != 0;
  unsigned xtag = 0;
  if constexpr (X) xtag = xc_tag<64>(XcView{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max}, bx);
  float rsa = 1.0f, rsb = 1.0f;
  if (BF == 2) { rsa = scale_from_amax(g.sa_dyn, g.sa); rsb = scale_from_amax(g.sb_dyn, g.sb); }
  if (g.amax_zero && bx == 0 && by == 0) amax_clear(g.amax_zero);
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  // Operand tiles travel global/L2 -> registers -> LDS.  A k-step's MFMAs take 0.25 us per 32 k rows, an L2 round trip
  // more: with the fetch of tile t+1 issued at the top of step t and stored at its bottom, every step waited for memory
  // (28 steps x ~0.8 us on the 880-deep layer-1 GEMMs).  The ring below keeps TWO tiles in flight (tile t+2 is
  // requested at the top of step t and stored at the bottom of step t+1): 29.1 -> 26.3 us on that GEMM.
  struct Tile { float4 a[NF], b[NF]; };
  auto fetch = [&](Tile& tl, const int t) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      tl.a[f] = tile_fetch<AMODE>(g.A, g.lda, m0, m_real, t * BK + f * kLdsBK, g.K, ones, g.M - 1, tid);
      tl.b[f] = tile_fetch<BMODE>(g.B, g.ldb, n0, g.N, t * BK + f * kLdsBK, g.K, false, 0, tid);
    }
  };
  auto park = [&](const Tile& tl, const int t) {
    float* An = lds + (t & 1) * 2 * BK * kLdsLD;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      tile_store<AMODE>(An + f * kLdsBK * kLdsLD, tid, tl.a[f]);
      tile_store<BMODE>(An + BK * kLdsLD + f * kLdsBK * kLdsLD, tid, tl.b[f]);
    }
  };
  Tile t0, t1;
  fetch(t0, 0);
  if (nst > 1) fetch(t1, 1);
  park(t0, 0);
  __syncthreads();
  // one k-step: request tile t+2 into the free register slot, multiply tile t out of LDS, park tile t+1 (requested one
  // step ago) in the other LDS buffer
  auto kstep = [&](const int t, Tile& free_slot, const Tile& ready) {
    if (t + 2 < nst) fetch(free_slot, t + 2);
    // this wavefront's K half of the tile: BK/2 rows from (BK/2) kh, in groups of 16.  fp32: lane half h takes
    // k = h + 2 s of a group (one 32x32x2 per s); bf16: k = 8 h + s (one 32x32x16 per group)
    constexpr int kstr = BF ? kLdsLD : 2 * kLdsLD;  // (modes 1 and 2 share the 32x32x16 lane map)
    const int koff = BF ? 8 * h : h;
    const float* base = lds + (t & 1) * 2 * BK * kLdsLD + ((BK / 2) * kh + koff) * kLdsLD + r;
#pragma unroll
    for (int q = 0; q < BK / 32; ++q) {
      const float* As = base + 16 * q * kLdsLD + 32 * wi;
      const float* Bs = base + BK * kLdsLD + 16 * q * kLdsLD + 32 * wj;
      float av[8], bv[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        av[s] = As[s * kstr];
        bv[s] = Bs[s * kstr];
      }
      if (BF == 1) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(to_bf16x8(av), to_bf16x8(bv), acc, 0, 0, 0);
      } else if (BF == 2) {
        acc = mfma_split(av, bv, rsa, rsb, acc);
      } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
      }
    }
    if (t + 1 < nst) park(ready, t + 1);
    __syncthreads();
  };
  for (int t = 0; t < nst; t += 2) {
    kstep(t, t0, t1);                    // even step: slot 0 is free (tile t is in LDS), slot 1 holds tile t+1
    if (t + 1 < nst) kstep(t + 1, t1, t0);  // odd step: the roles swap
  }
  if (BF == 2) {
    const float un = 1.0f / (rsa * rsb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] *= un;
  }
  lds_tile_epilogue<X>(g, acc, lds, stat, bx, by, n_row_tiles, xtag);
}


// ---------------------------------------------------------------------------------------------
// The LDS-DMA ring kernel (round 5; arithmetic mode 2 only).  Same 64 x 64 tile, same eight wavefronts (K half, quadrant) and the
// same epilogue as gemm_lds_tile -- what changes is how the operand tiles reach LDS.  With the products on the fp16 matrix
// instruction a 32-deep k-step is ~200 cycles of arithmetic per wavefront, and the register-staged pipeline (global -> VGPR ->
// ds_write, two tiles in flight, 8 + 8 ds_read_b32 per operand group) was bound by the memory round trip per step: the grouped
// weight-gradient launch took 77 us on 128 CUs for ~10 us of arithmetic.  Here every wavefront issues two
// `global_load_lds_dwordx4` per k-step (1 KB each, straight into the ring slot: no staging registers, no LDS store instructions),
// FOUR k-steps live in the 64 KB ring and three are in flight behind the one being multiplied; one workgroup barrier per k-step.
//   * operand stored k-major in memory (P[k ld + i]: both operands of the weight-gradient GEMMs, the kernels in the forward
//     pass): the slot holds [32 k][64 i], one DMA instruction = 4 k rows; fragment reads are unit-stride ds_read_b32.
//   * operand stored K-contiguous (P[i ld + k]: activations, dz, the kernels in the dX GEMMs): the slot holds [64 i][32 k] with the
//     eight 16-byte chunks of a row XOR-swizzled by (i >> 1) & 7 -- an LDS-DMA instruction writes lane l's 16 bytes at l x 16, so
//     the swizzle is applied to the ADDRESS each lane fetches from; a fragment (8 consecutive k of row i) is two ds_read_b128,
//     conflict-free in the hardware's 16-lane groups (MI355X_MICROARCH.md, LDS).
// The DMA instructions are inline asm: the compiler waits for vmcnt(0) in front of every LDS read that follows a
// __builtin_amdgcn_global_load_lds (it cannot tell the slots apart), which would take the three k-steps in flight back to none;
// the waits are counted by hand (two DMA instructions per wavefront and k-step, completed in order).
// Legal when K is a multiple of 32, both leading dimensions are multiples of 4, both bases 16-byte aligned and a k-major
// operand's extent is a multiple of 4 (ring_legal); anything else takes gemm_lds_tile / gemm_tile, which handle every shape.
// ---------------------------------------------------------------------------------------------
#ifndef LIPASR_RING_STAGES
#define LIPASR_RING_STAGES 4
#endif
constexpr int kRingStages = LIPASR_RING_STAGES;
constexpr int kRingTile = 64 * 32;  // floats of one operand tile of one k-step (8 KB)
constexpr size_t ring_gemm_bytes() { return (size_t)(kRingStages * 2 * kRingTile + 8 * 16 * 8) * sizeof(float); }

__device__ __forceinline__ void dma16(const float* gsrc, const unsigned lds_byte_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_byte_addr)
               : "memory");
}

// this lane's source address of operand tile rows/columns i0 .. i0 + 63 at k = 0 (advance by ring_step per k-step)
template <int MODE>
__device__ __forceinline__ const float* ring_src(const float* P, const int ld, const int i0, const int i_real, const int wave, const int lane) {
  if (MODE == 1) {
    const int k = 4 * wave + (lane >> 4), i = min(i0 + (lane & 15) * 4, i_real - 4);
    return P + (size_t)k * ld + i;
  }
  const int il = 8 * wave + (lane >> 3), c = (lane & 7) ^ ((il >> 1) & 7);
  return P + (size_t)min(i0 + il, i_real - 1) * ld + 4 * c;
}
template <int MODE>
__device__ __forceinline__ size_t ring_step(const int ld) { return MODE == 1 ? (size_t)32 * ld : (size_t)32; }

// the 8 consecutive k (16 kh + 8 hh ..) of row / column `il` of an operand tile in a ring slot
template <int MODE>
__device__ __forceinline__ void ring_frag(const float* __restrict__ T, const int il, const int kh, const int hh, float (&v)[8]) {
  if (MODE == 1) {
    const float* q = T + (16 * kh + 8 * hh) * 64 + il;
#pragma unroll
    for (int s = 0; s < 8; ++s) v[s] = q[s * 64];
  } else {
    const int sw = (il >> 1) & 7, c0 = 4 * kh + 2 * hh;
    const float4 lo = *reinterpret_cast<const float4*>(T + (il * 8 + (c0 ^ sw)) * 4);
    const float4 hi = *reinterpret_cast<const float4*>(T + (il * 8 + ((c0 + 1) ^ sw)) * 4);
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
  }
}

template <int AMODE, int BMODE, bool X = false, int NL = 0>  // NL: loader wavefronts beside the eight that multiply (0: every wavefront brings its own two pieces)
__device__ __forceinline__ void gemm_ring_tile(const GemmArgs& g, const int bx, const int by, const int n_row_tiles) {
  constexpr int TS = 64, S = kRingStages;
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [S][A | B][2048]; the epilogue reuses the first 32 KB; then stat
  float* stat = lds + S * 2 * kRingTile;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int kh = wave >> 2, wi = (wave >> 1) & 1, wj = wave & 1;
  const int m0 = by * TS, n0 = bx * TS;
  const int m_real = g.ones_row ? g.M - 1 : g.M;
  const int nst = (g.K + 31) >> 5;
  unsigned xtag = 0;
  if constexpr (X) xtag = xc_tag<64>(XcView{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max}, bx);
  // K that is no multiple of 32 (the 880 features of layer 1): in the last k-step the lanes whose 16 bytes lie at k >= K fetch zeros
  const int koff_a = AMODE == 1 ? 4 * wave + (lane >> 4) : 4 * ((lane & 7) ^ (((8 * wave + (lane >> 3)) >> 1) & 7));
  const int koff_b = BMODE == 1 ? 4 * wave + (lane >> 4) : 4 * ((lane & 7) ^ (((8 * wave + (lane >> 3)) >> 1) & 7));
  const bool k_tail = (g.K & 31) != 0;
  const float rsa = scale_from_amax(g.sa_dyn, g.sa), rsb = scale_from_amax(g.sb_dyn, g.sb);
  if (g.amax_zero && bx == 0 && by == 0) amax_clear(g.amax_zero);
  const float* pa = ring_src<AMODE>(g.A, g.lda, m0, m_real, wave, lane);
  const float* pb = ring_src<BMODE>(g.B, g.ldb, n0, g.N, wave, lane);
  const size_t sa_step = ring_step<AMODE>(g.lda), sb_step = ring_step<BMODE>(g.ldb);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds) + (unsigned)wave * 1024u;  // this wavefront's 1 KB of an A tile
  auto issue = [&](const int t) {
    const unsigned slot = lds0 + (unsigned)(t % S) * (2u * kRingTile * 4u);
    const bool last = k_tail && t == nst - 1;
    dma16((last && 32 * t + koff_a >= g.K) ? g.zeros : pa, slot);
    dma16((last && 32 * t + koff_b >= g.K) ? g.zeros : pb, slot + kRingTile * 4u);
    pa += sa_step;
    pb += sb_step;
  };
  const int il_ones = (AMODE == 1 && g.ones_row && g.M - 1 >= m0 && g.M - 1 < m0 + TS) ? g.M - 1 - m0 : -1;
  if constexpr (NL > 0) {
    // NL extra wavefronts bring the 16 pieces of a k-step (see the weight-gradient tile: a wavefront that issues LDS-DMA sits in the address
    // path meanwhile); loader L takes the pieces of wavefronts L, L + NL, ... of both operands
    if (wave >= 8) {
      const int L = wave - 8;
      constexpr int NP = 8 / NL;
      const float* sa[NP];
      const float* sb[NP];
      int ka[NP], kb[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int w = L + NL * q;
        sa[q] = ring_src<AMODE>(g.A, g.lda, m0, m_real, w, lane);
        sb[q] = ring_src<BMODE>(g.B, g.ldb, n0, g.N, w, lane);
        ka[q] = AMODE == 1 ? 4 * w + (lane >> 4) : 4 * ((lane & 7) ^ (((8 * w + (lane >> 3)) >> 1) & 7));
        kb[q] = BMODE == 1 ? 4 * w + (lane >> 4) : 4 * ((lane & 7) ^ (((8 * w + (lane >> 3)) >> 1) & 7));
      }
      const unsigned base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds);
      auto issue_l = [&](const int t) {
        const unsigned slot = base + (unsigned)(t % S) * (2u * kRingTile * 4u);
        const bool last = k_tail && t == nst - 1;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          const unsigned d = slot + (unsigned)(L + NL * q) * 1024u;
          dma16((last && 32 * t + ka[q] >= g.K) ? g.zeros : sa[q], d);
          dma16((last && 32 * t + kb[q] >= g.K) ? g.zeros : sb[q], d + kRingTile * 4u);
          sa[q] += sa_step;
          sb[q] += sb_step;
        }
      };
      for (int t = 0; t < min(S - 1, nst); ++t) issue_l(t);
      for (int t = 0; t < nst; ++t) {
        const int ahead = min(t + S - 2, nst - 1) - t;  // k-steps requested beyond t: 2 NP instructions each, completed in order
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NP) : "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (il_ones >= 0 && lane < 4 * NP) lds[(t % S) * 2 * kRingTile + (4 * (L + NL * (lane >> 2)) + (lane & 3)) * 64 + il_ones] = 1.0f;
        __syncthreads();
        if (t + S - 1 < nst) issue_l(t + S - 1);
      }
      __syncthreads();  // (the barrier in front of the epilogue)
      return;
    }
  }
  const int pre = NL > 0 ? 0 : min(S - 1, nst);
  for (int t = 0; t < pre; ++t) issue(t);
  // (the all-ones row of op(A) -- bias gradient of the weight-gradient GEMMs -- does not exist in memory: it is written into the slot)
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  auto k_loop = [&](auto unit_a) {  // (two copies of the loop: an unscaled A operand -- the activations -- splits in 12 instructions instead of 16)
    constexpr bool UA = decltype(unit_a)::value;
    for (int t = 0; t < nst; ++t) {
      float* At = lds + (t % S) * 2 * kRingTile;
      if constexpr (NL == 0) {
        const int ahead = min(t + S - 2, nst - 1) - t;  // k-steps requested beyond t: two DMA instructions each, completed in order
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (il_ones >= 0 && lane < 4) At[(4 * wave + lane) * 64 + il_ones] = 1.0f;  // (this wavefront's own four k rows: they have landed)
      }
      __syncthreads();  // every wavefront's part of k-step t is in LDS, and everybody is done with the slot of k-step t - 1
#if !defined(LIPASR_RING_PROBE) || LIPASR_RING_PROBE != 2   // (timing probes, never shipped: 1 = no arithmetic, 2 = no operand traffic after the prologue)
      if constexpr (NL == 0) {
        if (t + S - 1 < nst) issue(t + S - 1);
      }
#endif
#if !defined(LIPASR_RING_PROBE) || LIPASR_RING_PROBE != 1
      float av[8], bv[8];
      ring_frag<AMODE>(At, 32 * wi + r, kh, hh, av);
      ring_frag<BMODE>(At + kRingTile, 32 * wj + r, kh, hh, bv);
      acc = mfma_split<UA>(av, bv, rsa, rsb, acc);
#endif
    }
  };
  if (rsa == 1.0f) k_loop(std::true_type{});
  else k_loop(std::false_type{});
  {
    const float un = 1.0f / (rsa * rsb);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] *= un;
  }
  __syncthreads();  // the last k-step's fragments are read: the ring becomes the epilogue's `red`
  lds_tile_epilogue<X>(g, acc, lds, stat, bx, by, n_row_tiles, xtag);
}

#ifndef LIPASR_RING_LOADERS
#define LIPASR_RING_LOADERS 0
#endif
constexpr int kRingLoaders = LIPASR_RING_LOADERS;  // 0, 1, 2 or 4 (with the exchange epilogue's 81 registers two workgroups of ten wavefronts still share a CU).
// Measured with 2 (same box, interleaved): config 3 0.3427 against 0.3422 ms, config 2 0.3117 against 0.3108 -- two workgroups per CU already
// overlap one's address-path time with the other's arithmetic; the loaders pay where ONE workgroup owns the CU (the tiles below).  Off.
template <int AMODE, int BMODE, bool X = false>
__global__ __launch_bounds__(512 + 64 * kRingLoaders) void gemm_ring_kernel(GemmArgs g) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_ring_tile<AMODE, BMODE, X, kRingLoaders>(g, bx, by, gridDim.y);
}
// The exchange instance for launches of at most ONE workgroup per CU (layer 2 on a 128-CU share, layer 1 on the whole chip): four loader
// wavefronts.  Same box, interleaved, loaders on every exchange launch: config 2 0.3067 against 0.3098 ms (its 256-tile launches are one per
// CU); config 3 lost (two workgroups of twelve wavefronts no longer share a CU at 81 registers) -- hence per launch.
constexpr int kRingLoadersOnePerCu = 4;
template <int BMODE>
__global__ __launch_bounds__(512 + 64 * kRingLoadersOnePerCu) void gemm_ring_x1_kernel(GemmArgs g) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_ring_tile<0, BMODE, true, kRingLoadersOnePerCu>(g, bx, by, gridDim.y);
}

template <int AMODE, int BMODE, int BF = 0, int BK = kLdsBKMax, bool X = false>
__global__ __launch_bounds__(512) void gemm_lds_kernel(GemmArgs g) {
  int bx = blockIdx.x, by = blockIdx.y;
  if (g.xcd_map) xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y, bx, by);
  gemm_lds_tile<AMODE, BMODE, BF, BK, X>(g, bx, by, gridDim.y);
}

// The grouped launch with 64x64 LDS tiles: the weight-gradient GEMMs read both operands k-major (lin[k][i], dz[k][j]), which
// is exactly the LDS image, so a tile is staged by plain float4 copies and every operand element leaves L2 once per 64x64
// tile -- half the L2 -> CU traffic of the 32x32 fragment kernel (410 MB per step at batch 1024), which is what bounded it.
template <int AMODE, int BMODE, int BF = 0>
__global__ __launch_bounds__(512) void gemm_lds_grouped_kernel(GemmGroup grp) {
  int p = 0;
  while (p + 1 < grp.n && (int)blockIdx.x >= grp.tile_start[p + 1]) ++p;
  const GemmArgs& g = grp.g[p];
  const int local = blockIdx.x - grp.tile_start[p];
  const int ntx = (g.N + 63) / 64, nty = (g.M + 63) / 64;
  int bx = local % ntx, by = local / ntx;
  if (g.xcd_map && (grp.tile_start[p] & 7) == 0) xcd_tile(local, ntx, nty, bx, by);
  gemm_lds_tile<AMODE, BMODE, BF, kLdsBKMax>(g, bx, by, nty);
}


// ---------------------------------------------------------------------------------------------
// The weight-gradient tile of arithmetic mode 2: 128 x 128 outputs per workgroup, TWO accumulators per wavefront.
// The 64 x 64 ring tile above issues ~75 instructions per wavefront and k-step for 3 matrix instructions (one A and one B fragment
// split per 32 x 32 x 16 product) and was bound by that (its probes: 56 us with the arithmetic compiled out, 64 us with the operand
// traffic compiled out, 76 us whole, on 128 CUs).  Here wavefront (ri, cj) owns a 32 x 64 strip: per 16-deep chunk ONE A fragment is
// split and multiplies TWO B fragments -- 36 split instructions and 24 LDS reads for 6 matrix instructions --, every wavefront takes the
// whole 32-deep k-step (no K halves to add up afterwards), a k-step moves 32 KB for four times the 64 x 64 tile's arithmetic (half the
// operand traffic per flop), and the accumulators go straight to memory (the epilogue of a weight gradient is a store).  Both operands
// k-major (lin[k][i], dz[k][j]); ring of three k-steps = 96 KB, one workgroup per CU; 105 tiles for the reference's model.
// ---------------------------------------------------------------------------------------------
constexpr int kR128Stages = 3;
constexpr int kR128Tile = 32 * 128;  // floats of one operand tile of one k-step (16 KB)
constexpr size_t ring128_bytes() { return (size_t)(kR128Stages * 2 * kR128Tile) * sizeof(float); }

__device__ __forceinline__ void gemm_ring128_tile(const GemmArgs& g, const int bx, const int by) {
  constexpr int TS = 128, S = kR128Stages;
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [S][A | B][32 k][128]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int ri = wave >> 1, cj = wave & 1;
  const int m0 = by * TS, n0 = bx * TS;
  const int m_real = g.ones_row ? g.M - 1 : g.M;
  const int nst = (g.K + 31) >> 5;
  const float rsa = scale_from_amax(g.sa_dyn, g.sa), rsb = scale_from_amax(g.sb_dyn, g.sb);
  // DMA: an instruction moves 2 k rows of 128 floats; wavefront w moves k rows 4 w .. 4 w + 3 of both operands (two instructions each)
  const int kl = 4 * wave + (lane >> 5), il = (lane & 31) * 4;
  const float* pa = g.A + (size_t)kl * g.lda + min(m0 + il, m_real - 4);
  const float* pb = g.B + (size_t)kl * g.ldb + min(n0 + il, g.N - 4);
  const size_t a2 = (size_t)2 * g.lda, b2 = (size_t)2 * g.ldb, a32 = (size_t)32 * g.lda, b32 = (size_t)32 * g.ldb;
  const bool k_tail = (g.K & 31) != 0;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds) + (unsigned)wave * 2048u;  // this wavefront's 4 k rows of an A tile
  auto issue = [&](const int t) {
    const unsigned slot = lds0 + (unsigned)(t % S) * (2u * kR128Tile * 4u);
    const bool z0 = k_tail && 32 * t + kl >= g.K, z1 = k_tail && 32 * t + kl + 2 >= g.K;
    dma16(z0 ? g.zeros : pa, slot);
    dma16(z1 ? g.zeros : pa + a2, slot + 1024u);
    dma16(z0 ? g.zeros : pb, slot + kR128Tile * 4u);
    dma16(z1 ? g.zeros : pb + b2, slot + kR128Tile * 4u + 1024u);
    pa += a32;
    pb += b32;
  };
  const int pre = min(S - 1, nst);
  for (int t = 0; t < pre; ++t) issue(t);
  const int il_ones = (g.ones_row && g.M - 1 >= m0 && g.M - 1 < m0 + TS) ? g.M - 1 - m0 : -1;
  f32x16 acc0, acc1;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc0[q] = 0.0f; acc1[q] = 0.0f; }
  auto k_loop = [&](auto unit_a) {
  constexpr bool UA = decltype(unit_a)::value;
  for (int t = 0; t < nst; ++t) {
    const int ahead = min(t + S - 2, nst - 1) - t;  // k-steps requested beyond t: four DMA instructions each, completed in order
    if (ahead >= 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float* At = lds + (t % S) * 2 * kR128Tile;
    if (il_ones >= 0 && lane < 4) At[(4 * wave + lane) * TS + il_ones] = 1.0f;
    __syncthreads();
#if !defined(LIPASR_RING_PROBE) || LIPASR_RING_PROBE != 2
    if (t + S - 1 < nst) issue(t + S - 1);
#endif
    const float* Bt = At + kR128Tile;
#if !defined(LIPASR_RING_PROBE) || LIPASR_RING_PROBE != 1
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float* qa = At + (16 * c + 8 * hh) * TS + 32 * ri + r;
      const float* qb = Bt + (16 * c + 8 * hh) * TS + 64 * cj + r;
      float av[8], b0[8], b1[8];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        av[s8] = qa[s8 * TS];
        b0[s8] = qb[s8 * TS];
        b1[s8] = qb[s8 * TS + 32];
      }
      f16x8 ah, al, bh, bl;
      split8<UA>(av, rsa, ah, al);
      split8<false>(b0, rsb, bh, bl);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc0, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc0, 0, 0, 0);
      split8<false>(b1, rsb, bh, bl);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc1, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc1, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc1, 0, 0, 0);
    }
#else
    (void)Bt;
#endif
  }
  };
  if (rsa == 1.0f) k_loop(std::true_type{});
  else k_loop(std::false_type{});
  const float un = 1.0f / (rsa * rsb);
  const int gn0 = n0 + 64 * cj + r, gn1 = gn0 + 32;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int gm = m0 + 32 * ri + (q & 3) + 8 * (q >> 2) + 4 * hh;
    if (gm >= g.M) continue;
    float* crow = (g.ones_row && gm == g.M - 1) ? g.extra_out : g.C + (size_t)gm * g.ldc;
    if (gn0 < g.N) crow[gn0] = acc0[q] * un;
    if (gn1 < g.N) crow[gn1] = acc1[q] * un;
  }
}

// ---------------------------------------------------------------------------------------------
// The same 128 x 128 tile with a SPLIT PASS (round 5, after the counters): in the tile above every wavefront splits the fragments it
// multiplies -- the A fragment of a strip is split by both wavefronts that share it, a B fragment by all four -- and the launch was
// bound by that instruction stream (SQ counters on 128 CUs: 138 vector instructions per wavefront and k-step at ~6 cycles each, the
// wavefronts 39 % issuing / 25 % stalled on issue / 36 % parked at the barrier, the matrix pipe 16 % busy).  Here a k-step's fp32
// tile is split ONCE: each thread takes one 8-deep group of A and one of B from the ring slot (unit-stride ds_read_b32 down the
// k rows), splits them and writes the fp16 hi / lo planes K-CONTIGUOUS into a second, double-buffered region ([row][32 k] halves, the
// four 16-byte chunks of a row XOR-swizzled by (row >> 2) & 3); the matrix pass reads a fragment as ONE ds_read_b128 per plane and
// issues no vector arithmetic at all.  Per wavefront and k-step: 16 + 12 LDS reads, ~30 vector instructions, 12 matrix instructions.
// One barrier per k-step still: iteration t splits k-step t (landed: its DMA was issued two iterations ago) while it multiplies
// k-step t - 1 (split in the iteration before), and re-issues the ring slot the previous split pass emptied.
// LDS: 3 x 32 KB ring + 2 x 32 KB planes = 160 KB, the whole CU (gfx950's addressable maximum).
// ---------------------------------------------------------------------------------------------
#ifndef LIPASR_R128_LOADERS
#define LIPASR_R128_LOADERS 4
#endif
constexpr int kR128Loaders = LIPASR_R128_LOADERS;  // 1, 2 or 4
constexpr int kR128PlaneBytes = 128 * 64;  // one fp16 plane of one operand: 128 rows x 32 k
constexpr size_t ring128s_bytes() { return ring128_bytes() + (size_t)2 * 4 * kR128PlaneBytes; }

__device__ __forceinline__ void gemm_ring128s_tile(const GemmArgs& g, const int bx, const int by) {
  constexpr int TS = 128, S = kR128Stages;
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [S][A | B][32 k][128] fp32, then [2][A hi | A lo | B hi | B lo][128][32] fp16
  char* const planes = reinterpret_cast<char*>(lds) + ring128_bytes();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int ri = wave >> 1, cj = wave & 1;
  const int m0 = by * TS, n0 = bx * TS;
  const int m_real = g.ones_row ? g.M - 1 : g.M;
  const int nst = (g.K + 31) >> 5;
  const float rsa = scale_from_amax(g.sa_dyn, g.sa), rsb = scale_from_amax(g.sb_dyn, g.sb);
  const int il_ones = (g.ones_row && g.M - 1 >= m0 && g.M - 1 < m0 + TS) ? g.M - 1 - m0 : -1;  // the all-ones row of op(A) (bias gradients): patched into the slot
  // kR128Loaders extra wavefronts are LOADERS: they issue the 32 DMA instructions of a k-step (16 pieces of two k rows per operand) while the
  // eight others split and multiply.  With every wavefront issuing its own four pieces right behind the barrier each of them sat ~800
  // cycles of a ~2800-cycle k-step in the address path (s_memtime), the vector and matrix pipes idle meanwhile; a single wavefront gets a
  // piece accepted every ~130 cycles and the path itself takes ~64 per piece (16 B per cycle and CU), so it takes two to keep it busy.
  if (wave >= 8) {
    const int L = wave - 8;
    constexpr int NQ = 32 / kR128Loaders;  // pieces per loader and k-step: piece q -> operand q / (NQ / 2), piece index j = kR128Loaders (q % (NQ / 2)) + L
    const float* src[NQ];
    int krow[NQ];
    unsigned dst[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int op = q / (NQ / 2), j = kR128Loaders * (q % (NQ / 2)) + L;
      krow[q] = 2 * j + (lane >> 5);
      const int c = (lane & 31) * 4;
      src[q] = op ? g.B + (size_t)krow[q] * g.ldb + min(n0 + c, g.N - 4) : g.A + (size_t)krow[q] * g.lda + min(m0 + c, m_real - 4);
      dst[q] = (unsigned)op * (unsigned)(kR128Tile * 4) + (unsigned)j * 1024u;
    }
    const size_t a32 = (size_t)32 * g.lda, b32 = (size_t)32 * g.ldb;
    const bool k_tail = (g.K & 31) != 0;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds);
    auto issue = [&](const int t) {
      const unsigned slot = lds0 + (unsigned)(t % S) * (2u * kR128Tile * 4u);
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
#if defined(LIPASR_R128_PROBE) && LIPASR_R128_PROBE == 3   // (timing probes, never shipped: 1 no arithmetic, 2 no operand traffic after the prologue, 3 every DMA from one hot line)
        dma16(g.zeros, slot + dst[q]);
#else
        dma16((k_tail && 32 * t + krow[q] >= g.K) ? g.zeros : src[q], slot + dst[q]);
#endif
        src[q] += q < NQ / 2 ? a32 : b32;
      }
    };
    for (int t = 0; t < min(2, nst); ++t) issue(t);
    for (int t = 0; t <= nst; ++t) {
      if (t < nst) {  // this loader's pieces of k-step t have landed (those of t + 1 may still be in flight)
        if (t + 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (il_ones >= 0 && lane < NQ) {  // the ones row, in the k rows this loader brought: A pieces j = kR128Loaders (lane / 2) + L, row lane & 1
          const int k = 2 * (kR128Loaders * (lane >> 1) + L) + (lane & 1);
          lds[(t % S) * 2 * kR128Tile + k * TS + il_ones] = 1.0f;
        }
      }
      __syncthreads();
#if !defined(LIPASR_R128_PROBE) || LIPASR_R128_PROBE != 2
      if (t + 2 < nst) issue(t + 2);  // into the slot the split pass of t - 1 emptied
#endif
    }
    return;  // (the barriers count the wavefronts that are left; there are none behind the loop)
  }
  // split pass: this thread's group = rows k = 8 sc .. 8 sc + 7 of column si, of A and of B
  const int si = 64 * (wave & 1) + lane, sc = wave >> 1;
  const unsigned sp_off = (unsigned)si * 64u + (unsigned)((sc ^ ((si >> 2) & 3)) << 4);
  // matrix pass: fragment (row, chunk c = 2 cc + hh) of a plane
  const int row_a = 32 * ri + r, row_b = 64 * cj + r;
  unsigned off_a[2], off_b[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    off_a[cc] = (unsigned)row_a * 64u + (unsigned)(((2 * cc + hh) ^ ((row_a >> 2) & 3)) << 4);
    off_b[cc] = (unsigned)row_b * 64u + (unsigned)(((2 * cc + hh) ^ ((row_b >> 2) & 3)) << 4);
  }
  f32x16 acc0, acc1;
#pragma unroll
  for (int q = 0; q < 16; ++q) { acc0[q] = 0.0f; acc1[q] = 0.0f; }
  auto k_loop = [&](auto unit_a) {
    constexpr bool UA = decltype(unit_a)::value;
    for (int t = 0; t <= nst; ++t) {
      __syncthreads();  // k-step t is in its ring slot (the loaders waited for it); the split pass of t - 1 and the matrix pass of t - 2 are over everywhere
#if !defined(LIPASR_R128_PROBE) || (LIPASR_R128_PROBE != 1 && LIPASR_R128_PROBE != 3)
      if (t < nst) {
        const float* Ra = lds + (t % S) * 2 * kR128Tile + (8 * sc) * TS + si;
        char* P = planes + (t & 1) * 4 * kR128PlaneBytes + sp_off;
        float av[8], bv[8];
#pragma unroll
        for (int s8 = 0; s8 < 8; ++s8) {
          av[s8] = Ra[s8 * TS];
          bv[s8] = Ra[kR128Tile + s8 * TS];
        }
        f16x8 h, l;
        split8<UA>(av, rsa, h, l);
        *reinterpret_cast<f16x8*>(P) = h;
        *reinterpret_cast<f16x8*>(P + kR128PlaneBytes) = l;
        split8<false>(bv, rsb, h, l);
        *reinterpret_cast<f16x8*>(P + 2 * kR128PlaneBytes) = h;
        *reinterpret_cast<f16x8*>(P + 3 * kR128PlaneBytes) = l;
      }
      if (t >= 1) {
        const char* P = planes + ((t - 1) & 1) * 4 * kR128PlaneBytes;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          const f16x8 ah = *reinterpret_cast<const f16x8*>(P + off_a[cc]);
          const f16x8 al = *reinterpret_cast<const f16x8*>(P + kR128PlaneBytes + off_a[cc]);
          const f16x8 b0h = *reinterpret_cast<const f16x8*>(P + 2 * kR128PlaneBytes + off_b[cc]);
          const f16x8 b0l = *reinterpret_cast<const f16x8*>(P + 3 * kR128PlaneBytes + off_b[cc]);
          const f16x8 b1h = *reinterpret_cast<const f16x8*>(P + 2 * kR128PlaneBytes + off_b[cc] + 32 * 64);
          const f16x8 b1l = *reinterpret_cast<const f16x8*>(P + 3 * kR128PlaneBytes + off_b[cc] + 32 * 64);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b0h, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b1h, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b0l, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b1l, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b0h, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b1h, acc1, 0, 0, 0);
        }
      }
#endif
    }
  };
  if (rsa == 1.0f) k_loop(std::true_type{});
  else k_loop(std::false_type{});
  const float un = 1.0f / (rsa * rsb);
  const int gn0 = n0 + 64 * cj + r, gn1 = gn0 + 32;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int gm = m0 + 32 * ri + (q & 3) + 8 * (q >> 2) + 4 * hh;
    if (gm >= g.M) continue;
    float* crow = (g.ones_row && gm == g.M - 1) ? g.extra_out : g.C + (size_t)gm * g.ldc;
    if (gn0 < g.N) crow[gn0] = acc0[q] * un;
    if (gn1 < g.N) crow[gn1] = acc1[q] * un;
  }
}

// the grouped weight-gradient launch in arithmetic mode 2: every problem that is ring_legal on the LDS-DMA ring tile, the others
// (the 64 x 10 output layer: its extent is no multiple of 4) on the register-staged tile
__global__ __launch_bounds__(512 + 64 * kR128Loaders) void gemm_ring_grouped_kernel(GemmGroup grp) {
  int p = 0;
  while (p + 1 < grp.n && (int)blockIdx.x >= grp.tile_start[p + 1]) ++p;
  const GemmArgs& g = grp.g[p];
  const int local = blockIdx.x - grp.tile_start[p];
  const int ts = g.ring >= 2 ? 128 : 64;
  const int ntx = (g.N + ts - 1) / ts, nty = (g.M + ts - 1) / ts;
  int bx = local % ntx, by = local / ntx;
  if (g.xcd_map && (grp.tile_start[p] & 7) == 0) xcd_tile(local, ntx, nty, bx, by);
  if (g.ring == 2) { gemm_ring128s_tile(g, bx, by); return; }
  if (threadIdx.x >= 512) return;  // (the loader wavefronts of the split-pass tile: the other tiles are eight wavefronts)
  if (g.ring == 3) gemm_ring128_tile(g, bx, by);
  else if (g.ring) gemm_ring_tile<1, 1>(g, bx, by, nty);
  else gemm_lds_tile<1, 1, 2, kLdsBKMax>(g, bx, by, nty);
}

// ---------------------------------------------------------------------------------------------
// The exchange-epilogue GEMMs of arithmetic mode 2 on 128 x 64 tiles (round 5): forward (A = activations, row-major; B = kernel,
// k-major) and input-gradient (B = kernel, K-contiguous) launches whose 64 x 64 tiling would put two or more workgroups on every CU
// of the plan's share.  What bounds the ring kernels on a CU share is the LDS-DMA fill rate of a CU (~32 GB/s: probe 3 of the
// weight-gradient tile above), so what counts is bytes per CU: a 128 x 64 tile moves 24 KB per k-step for the work of two 64 x 64
// tiles (32 KB).  Same split pass as the weight-gradient tile: every thread splits one 8-deep group of A (and the first 256 threads
// one of B) from the ring slot into K-contiguous fp16 planes, wavefront (ri, cj) multiplies the 32 x 32 output block (32 ri, 32 cj)
// over the whole k-step from four ds_read_b128 per 16-deep chunk; no K halves to add up.  Ring of three k-steps (72 KB) + two plane
// buffers (48 KB) + the epilogue's statistics: one workgroup per CU.  The epilogue is lds_tile_epilogue's exchange branch on four
// 32-row passes: the workgroup contributes ONE row tile of 128 rows to its column block's exchange.
// ---------------------------------------------------------------------------------------------
constexpr int kR2TileA = 128 * 32, kR2TileB = 64 * 32;            // floats of one k-step's operand tiles
constexpr int kR2Slot = kR2TileA + kR2TileB;                       // 24 KB
constexpr int kR2Stages = 3;
constexpr int kR2PlaneA = 128 * 64, kR2PlaneB = 64 * 64;           // bytes of one fp16 plane
constexpr int kR2Planes = 2 * kR2PlaneA + 2 * kR2PlaneB;           // one buffer: A hi | A lo | B hi | B lo (24 KB)
constexpr size_t ring2_bytes() { return (size_t)kR2Stages * kR2Slot * sizeof(float) + 2 * (size_t)kR2Planes + (size_t)8 * 16 * 8 * sizeof(float); }
#ifndef LIPASR_R2_LOADERS
#define LIPASR_R2_LOADERS 4
#endif
constexpr int kR2Loaders = LIPASR_R2_LOADERS;  // 1, 2, 3, 4, 6 or 8: divides the 24 pieces of a k-step

template <int BMODE>
__device__ __forceinline__ void gemm_ring2_tile(const GemmArgs& g, const int bx, const int by, const int n_row_tiles) {
  constexpr int S = kR2Stages;
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [S][A 128x32 | B 64x32] fp32, [2] plane buffers, stat
  char* const planes = reinterpret_cast<char*>(lds + S * kR2Slot);
  float* const stat = reinterpret_cast<float*>(planes + 2 * kR2Planes);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int ri = wave >> 1, cj = wave & 1;
  const int m0 = by * 128, n0 = bx * 64;
  const int nst = (g.K + 31) >> 5;
  const unsigned xtag = xc_tag<64>(XcView{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max}, bx);
  const float rsa = scale_from_amax(g.sa_dyn, g.sa), rsb = scale_from_amax(g.sb_dyn, g.sb);
  if (g.amax_zero && bx == 0 && by == 0) amax_clear(g.amax_zero);
  // kR2Loaders extra wavefronts are loaders (see the weight-gradient tile): the 24 pieces of a k-step -- 16 of 8 rows of the A tile (the eight
  // 16-byte chunks of a row XOR-swizzled through the source address as in the 64 x 64 ring tile), 8 of the B tile -- dealt round-robin
  if (wave >= 8) {
    const int L = wave - 8;
    constexpr int NQ = 24 / kR2Loaders;
    const float* src[NQ];
    int koff[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = kR2Loaders * q + L;  // piece 0 .. 23
      if (j < 16) {
        const int row = 8 * j + (lane >> 3);
        koff[q] = 4 * ((lane & 7) ^ ((row >> 1) & 7));
        src[q] = g.A + (size_t)min(m0 + row, g.M - 1) * g.lda + koff[q];
      } else if (BMODE == 1) {
        koff[q] = 4 * (j - 16) + (lane >> 4);
        src[q] = g.B + (size_t)koff[q] * g.ldb + min(n0 + (lane & 15) * 4, g.N - 4);
      } else {
        const int br = 8 * (j - 16) + (lane >> 3);
        koff[q] = 4 * ((lane & 7) ^ ((br >> 1) & 7));
        src[q] = g.B + (size_t)min(n0 + br, g.N - 1) * g.ldb + koff[q];
      }
    }
    const size_t sb_step = BMODE == 1 ? (size_t)32 * g.ldb : (size_t)32;
    const bool k_tail = (g.K & 31) != 0;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds);
    auto issue = [&](const int t) {
      const unsigned slot = lds0 + (unsigned)(t % S) * (unsigned)(kR2Slot * 4);
      const bool last = k_tail && t == nst - 1;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        dma16((last && 32 * t + koff[q] >= g.K) ? g.zeros : src[q], slot + (unsigned)(kR2Loaders * q + L) * 1024u);
        src[q] += (kR2Loaders * q + L) < 16 ? (size_t)32 : sb_step;
      }
    };
    for (int t = 0; t < min(2, nst); ++t) issue(t);
    for (int t = 0; t <= nst; ++t) {
      if (t < nst) {
        if (t + 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NQ) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
      if (t + 2 < nst) issue(t + 2);  // into the slot the split pass of t - 1 emptied
    }
    return;  // (the barriers of the epilogue count the wavefronts that are left)
  }
  // split pass: row si = 64 (w & 1) + lane, chunk sc = w >> 1 of A; wavefronts 0 .. 3 also row / column `lane`, chunk w of B
  const int si = 64 * (wave & 1) + lane, sc = wave >> 1;
  const unsigned spa = (unsigned)si * 64u + (unsigned)((sc ^ ((si >> 2) & 3)) << 4);
  const unsigned spb = (unsigned)lane * 64u + (unsigned)(((wave & 3) ^ ((lane >> 2) & 3)) << 4);
  // matrix pass: fragment (row, chunk 2 cc + hh)
  const int row_a = 32 * ri + r, row_b = 32 * cj + r;
  unsigned off_a[2], off_b[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    off_a[cc] = (unsigned)row_a * 64u + (unsigned)(((2 * cc + hh) ^ ((row_a >> 2) & 3)) << 4);
    off_b[cc] = (unsigned)(2 * kR2PlaneA) + (unsigned)row_b * 64u + (unsigned)(((2 * cc + hh) ^ ((row_b >> 2) & 3)) << 4);
  }
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  auto k_loop = [&](auto unit_a) {
    constexpr bool UA = decltype(unit_a)::value;
    for (int t = 0; t <= nst; ++t) {
      __syncthreads();  // k-step t is in its ring slot (the loaders waited for it); the split pass of t - 1 and the matrix pass of t - 2 are over everywhere
      // Order inside a k-step (one dependent chain per wavefront, so the LDS round trips are put behind each other's shadow): the
      // split pass's raw reads and the matrix pass's first fragments are requested together, the splits run while the fragments
      // arrive, the second chunk's fragments are requested in front of the first chunk's matrix instructions.
      const float* Rs = lds + (t % S) * kR2Slot;
      const char* Pm = planes + ((t - 1) & 1) * kR2Planes;
      float va[8], vb[8];
      f16x8 ah, al, bh, bl;
      if (t < nst) {
        ring_frag<0>(Rs, si, sc >> 1, sc & 1, va);
        if (wave < 4) ring_frag<BMODE>(Rs + kR2TileA, lane, wave >> 1, wave & 1, vb);
      }
      if (t >= 1) {
        ah = *reinterpret_cast<const f16x8*>(Pm + off_a[0]);
        al = *reinterpret_cast<const f16x8*>(Pm + kR2PlaneA + off_a[0]);
        bh = *reinterpret_cast<const f16x8*>(Pm + off_b[0]);
        bl = *reinterpret_cast<const f16x8*>(Pm + kR2PlaneB + off_b[0]);
      }
      if (t < nst) {
        char* P = planes + (t & 1) * kR2Planes;
        f16x8 h, l;
        split8<UA>(va, rsa, h, l);
        *reinterpret_cast<f16x8*>(P + spa) = h;
        *reinterpret_cast<f16x8*>(P + kR2PlaneA + spa) = l;
        if (wave < 4) {
          split8<false>(vb, rsb, h, l);
          *reinterpret_cast<f16x8*>(P + 2 * kR2PlaneA + spb) = h;
          *reinterpret_cast<f16x8*>(P + 2 * kR2PlaneA + kR2PlaneB + spb) = l;
        }
      }
      if (t >= 1) {
        const f16x8 ah1 = *reinterpret_cast<const f16x8*>(Pm + off_a[1]);
        const f16x8 al1 = *reinterpret_cast<const f16x8*>(Pm + kR2PlaneA + off_a[1]);
        const f16x8 bh1 = *reinterpret_cast<const f16x8*>(Pm + off_b[1]);
        const f16x8 bl1 = *reinterpret_cast<const f16x8*>(Pm + kR2PlaneB + off_b[1]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1, bh1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1, bl1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al1, bh1, acc, 0, 0, 0);
      }
    }
  };
  if (rsa == 1.0f) k_loop(std::true_type{});
  else k_loop(std::false_type{});
  // ---- epilogue: the exchange branch of lds_tile_epilogue on four 32-row passes
  constexpr int TS = 64;
  const int tcol = tid & 15, trow = tid >> 4;
  const int c4 = tcol * 4, gn = n0 + c4;
  const int gm4[4] = {m0 + trow, m0 + trow + 32, m0 + trow + 64, m0 + trow + 96};
  BnxPre xpre[4];
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) bnx_prefetch(g, gm4[p4], gn, xpre[p4]);
  const float un = 1.0f / (rsa * rsb);
  float* red = lds;  // [128][64] over the ring slots: their last reader was the split pass of k-step nst - 1, in front of the loop's last barrier
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int row = 32 * ri + (q & 3) + 8 * (q >> 2) + 4 * hh;
    red[row * TS + 32 * cj + r] = acc[q] * un;
  }
  __syncthreads();
  const int step = g.drop.step_dev ? *g.drop.step_dev : 0;
  float val[4][4], av[4][4], c1[4] = {0.f, 0.f, 0.f, 0.f}, c2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) {
    const float4 s = *reinterpret_cast<const float4*>(red + (trow + 32 * p4) * TS + c4);
    const float accv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t1, t2;
      bnx_elem(g, step, gm4[p4] < g.M && gn + e < g.N, gm4[p4], gn + e, accv[e], xpre[p4], e, val[p4][e], av[p4][e], t1, t2);
      c1[e] += t1;
      c2[e] += t2;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c1[e] += __shfl_xor(c1[e], 16, 64); c1[e] += __shfl_xor(c1[e], 32, 64);
    c2[e] += __shfl_xor(c2[e], 16, 64); c2[e] += __shfl_xor(c2[e], 32, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      stat[(wave * 16 + lane) * 8 + e] = c1[e];
      stat[(wave * 16 + lane) * 8 + 4 + e] = c2[e];
    }
  }
  __syncthreads();  // (every read of `red` is done: it is carved up below)
  float* mine = red;                                       // [2][64]
  float* colp = red + 128;                                 // [2][64]
  double* sbuf = reinterpret_cast<double*>(red + 256);     // [4][128]
  double* tot = sbuf + 4 * 128;                            // [128]
  if (tid < 2 * TS) {
    const int which = tid / TS, col = tid % TS, l4 = col >> 2, e = col & 3;
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += stat[(w * 16 + l4) * 8 + which * 4 + e];
    mine[tid] = t;
  }
  __syncthreads();
  BnxLate late;
  bnx_late_load(g, gn, late);
  float mm0, mv0;
  bnx_moving_load(g, by, n0 + tid, tid < TS, mm0, mv0);
  XcView xc{g.xc_gran, g.xc_ctrl, g.xc_err, g.xc_rt_max};
  xc_exchange<512, 64>(xc, bx, by, g.Bstat < 0 ? 0 : n_row_tiles, xtag, mine, sbuf, tot, [&]() {
    if (g.epi != EPI_BIAS_RELU_BNX) return;
#pragma unroll
    for (int p4 = 0; p4 < 4; ++p4) {
      if (gm4[p4] >= g.M) continue;
      float* crow = g.C + (size_t)gm4[p4] * g.ldc;
      if (gn + 3 < g.N && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(crow) & 15) == 0)) {
        *reinterpret_cast<float4*>(crow + gn) = make_float4(val[p4][0], val[p4][1], val[p4][2], val[p4][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gn + e < g.N) crow[gn + e] = val[p4][e];
      }
    }
  });
  if (tid < TS) bnx_column(g, by, n0 + tid, tid, TS, tot, colp, mm0, mv0);
  __syncthreads();
  bnx_finish<4>(g, step, gm4, gn, val, av, colp, TS, c4, late);
}

template <int BMODE>
__global__ __launch_bounds__(512 + 64 * kR2Loaders) void gemm_ring2_kernel(GemmArgs g) {
  gemm_ring2_tile<BMODE>(g, blockIdx.x, blockIdx.y, gridDim.y);
}


// ---------------------------------------------------------------------------------------------
// Host side.  pick_gemm is the ONE place that decides which instance runs a problem; launch_gemm, gemm_row_tiles and
// exchange_fits all go through it or through the predicates it is written with.
// ---------------------------------------------------------------------------------------------
static GemmKnobs g_knobs;
const GemmKnobs& gemm_knobs() { return g_knobs; }
constexpr int kEpiCount = EPI_DH_BNX + 1;
// Test hooks (lipasr_debug_gemm_launches / lipasr_debug_group_launches): launches since load, counted from the GemmPick / group that
// is actually launched.  Plain host increments; the kernels see nothing of them.
static long g_gemm_launches[GK_KINDS][2][2][2][3][kEpiCount] = {};  // [kind][exchange][AMODE][BMODE][arithmetic][epilogue]
static long g_group_launches[3][3] = {};   // [0 fragment, 1 LDS, 2 ring tiles][arithmetic]: grouped weight-gradient launches
static long g_group_ring_problems[4] = {};  // problems inside ring launches by GemmArgs::ring (0: not ring-legal, on plain tiles)
static long g_group_ring_launches[4] = {};  // ring launches by the launch's ring tile (1 64 x 64, 2 128 x 128 split pass, 3 per fragment)

// Every instantiated GEMM kernel, indexed by what the templates are parameterised on; null = not instantiated.
// arithmetic mode (GemmArgs::bf16: 0 exact fp32, 1 bf16 operands, 2 fp16 two-plane split) -> index
static int arith_index(int bf16) { return bf16 == 2 ? 2 : bf16 == 1 ? 1 : 0; }
struct GemmTable {
  const void* fn[GK_KINDS][2][2][2][3] = {};  // [kind][exchange epilogue][AMODE][BMODE][arithmetic]
  const void* grouped_frag[3] = {}, *grouped_lds[3] = {}, *grouped_ring = nullptr;  // weight-gradient groups (AMODE 1, BMODE 1)
  template <int A, int B, int AR> void plain() {
    fn[GK_FRAG4][0][A][B][AR] = reinterpret_cast<const void*>(gemm_f32_kernel<A, B, 4, AR>);
    fn[GK_FRAG16][0][A][B][AR] = reinterpret_cast<const void*>(gemm_f32_kernel<A, B, 16, AR>);
    fn[GK_LDS][0][A][B][AR] = reinterpret_cast<const void*>(gemm_lds_kernel<A, B, AR>);
  }
  template <int A, int B> void plain_modes() {
    plain<A, B, 0>(); plain<A, B, 1>(); plain<A, B, 2>();
    fn[GK_RING][0][A][B][2] = reinterpret_cast<const void*>(gemm_ring_kernel<A, B>);
  }
  template <int B, int AR> void exchange() {  // forward (NN) or input-gradient (NT) GEMMs only: AMODE 0
    fn[GK_FRAG4][1][0][B][AR] = reinterpret_cast<const void*>(gemm_f32_kernel<0, B, 4, AR, true>);
    fn[GK_LDS][1][0][B][AR] = reinterpret_cast<const void*>(gemm_lds_kernel<0, B, AR, kLdsBKMax, true>);
  }
  template <int B> void exchange_modes() {
    exchange<B, 0>(); exchange<B, 1>(); exchange<B, 2>();
    fn[GK_RING][1][0][B][2] = reinterpret_cast<const void*>(gemm_ring_kernel<0, B, true>);
    fn[GK_RING_X1][1][0][B][2] = reinterpret_cast<const void*>(gemm_ring_x1_kernel<B>);
    fn[GK_RING2][1][0][B][2] = reinterpret_cast<const void*>(gemm_ring2_kernel<B>);
  }
  template <int AR> void grouped() {
    grouped_frag[AR] = reinterpret_cast<const void*>(gemm_f32_grouped_kernel<1, 1, 4, AR>);
    grouped_lds[AR] = reinterpret_cast<const void*>(gemm_lds_grouped_kernel<1, 1, AR>);
  }
  GemmTable() {
    plain_modes<0, 0>(); plain_modes<0, 1>(); plain_modes<1, 0>(); plain_modes<1, 1>();
    exchange_modes<0>(); exchange_modes<1>();
    grouped<0>(); grouped<1>(); grouped<2>();
    grouped_ring = reinterpret_cast<const void*>(gemm_ring_grouped_kernel);
  }
};
static const GemmTable& gemm_table() { static const GemmTable t; return t; }

constexpr size_t frag_gemm_bytes(int nw) { return (size_t)(nw * 32 * 32 + 4 * 8 * 8) * sizeof(float); }

// the instance of a kind with its tile and launch shape
static GemmPick gemm_instance(int kind, bool exchange, int amode, int bmode, int ar) {
  static const struct { int tile_m, tile_n, threads; size_t lds; } shape[GK_KINDS] = {
      {32, 32, 256, frag_gemm_bytes(4)},
      {32, 32, 1024, frag_gemm_bytes(16)},
      {64, 64, 512, lds_gemm_bytes(kLdsBKMax)},
      {64, 64, 512 + 64 * kRingLoaders, ring_gemm_bytes()},
      {64, 64, 512 + 64 * kRingLoadersOnePerCu, ring_gemm_bytes()},
      {128, 64, 512 + 64 * kR2Loaders, ring2_bytes()}};
  return GemmPick{kind, shape[kind].tile_m, shape[kind].tile_n, shape[kind].threads, shape[kind].lds,
                  gemm_table().fn[kind][exchange ? 1 : 0][amode][bmode][ar]};
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool ring_legal(int amode, int bmode, const GemmArgs& g) {
  if (g_knobs.no_ring || g.bf16 != 2 || g.M < 64 || g.N < 64 || g.K < 32) return false;
  if ((g.K & 31) && (!g.zeros || (g.K & 3))) return false;  // a K tail needs the zero source, and whole 16-byte chunks
  if ((g.lda & 3) || (g.ldb & 3) || !aligned16(g.A) || !aligned16(g.B)) return false;
  const int m_real = g.ones_row ? g.M - 1 : g.M;
  if (amode == 1 && ((m_real & 3) || m_real < 4)) return false;
  if (bmode == 1 && ((g.N & 3) || g.N < 4)) return false;
  return true;
}

// The 128 x 64 exchange tile (gemm_ring2_tile) pays where the 64 x 64 tiling would put two workgroups on (nearly) every CU of the
// plan's share: then it halves the workgroups and moves 3/4 of the bytes per CU; with fewer tiles than that it would leave CUs idle.
// One workgroup per CU (124 KB of LDS) and every workgroup resident (the exchange): at most `cus` tiles.
static bool use_ring2(int bmode, const GemmArgs& g, int cus) {
  if (!g_knobs.ring2 || g.bf16 != 2 || g.M < 128 || g.N < 64 || !ring_legal(0, bmode, g)) return false;
  const long tiles = (long)((g.M + 127) / 128) * ((g.N + 63) / 64);
  return 4 * tiles >= 3 * (long)cus && tiles <= (long)cus && (g.M + 127) / 128 <= g.xc_rt_max;
}

constexpr int kLdsMinTiles = 224;  // measured on MI355X (scratch/time_gemm.py): the LDS kernel wins from ~one tile per CU

static bool use_lds_gemm(int M, int N, int K, int min_tiles = 0) {
  if (g_knobs.gemm_mode == 1) return false;
  const bool legal = M >= 64 && N >= 64 && K >= 32;
  if (g_knobs.gemm_mode == 2) return legal;
  const long tiles = (long)((M + 63) / 64) * ((N + 63) / 64);
  return legal && tiles >= (min_tiles > 0 ? min_tiles : kLdsMinTiles);
}

int pick_gemm(int amode, int bmode, const GemmArgs& g, GemmPick* out) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) { set_error("gemm: empty problem %dx%dx%d", g.M, g.N, g.K); return LIPASR_EINVAL; }
  const bool lds_k = use_lds_gemm(g.M, g.N, g.K, g.lds_min_tiles);
  const bool exchange = g.epi == EPI_BIAS_RELU_BNX || g.epi == EPI_DH_BNX;
  int kind;
  if (g.epi == EPI_BIAS_SOFTMAX_CE) {  // one 32-wide column tile, 4 wavefronts: the epilogue reduces along lanes
    if (g.N > 32) { set_error("gemm: the fused softmax epilogue needs N <= 32 (got %d)", g.N); return LIPASR_EINVAL; }
    if (amode != 0 || bmode != 1) { set_error("gemm: the fused softmax epilogue is a forward (NN) epilogue"); return LIPASR_EINVAL; }
    kind = GK_FRAG4;
  } else if (exchange) {  // the exchange epilogue: forward (NN) or input-gradient (NT) GEMMs only
    if (amode != 0) { set_error("gemm: the exchange epilogue needs a row-major A operand"); return LIPASR_EINVAL; }
    const int cus = g.cus > 0 ? g.cus : device_cus();
    if (use_ring2(bmode, g, cus)) kind = GK_RING2;  // 128 x 64 tiles, one workgroup per CU of the plan's share
    else if (lds_k && ring_legal(0, bmode, g))      // at most one workgroup per CU: the instance with loader wavefronts
      kind = (g_knobs.ring_x1 && (long)((g.N + 63) / 64) * ((g.M + 63) / 64) <= (long)cus) ? GK_RING_X1 : GK_RING;
    else kind = lds_k ? GK_LDS : GK_FRAG4;
  } else if (lds_k) {
    kind = ring_legal(amode, bmode, g) ? GK_RING : GK_LDS;
  } else {
    // Few output tiles and a long K (the dW GEMMs of the narrow layers, K = batch): 16 wavefronts split K so that
    // the serial chain of chunk loads per wavefront stays short.  Not for the *_STATS epilogues (never needed there).
    const long tiles = (long)((g.N + 31) / 32) * ((g.M + 31) / 32);
    const bool deep = tiles <= 192 && g.K >= 512 && g.epi != EPI_BIAS_RELU_STATS && g.epi != EPI_DH_STATS;
    kind = deep ? GK_FRAG16 : GK_FRAG4;
  }
  *out = gemm_instance(kind, exchange, amode ? 1 : 0, bmode ? 1 : 0, kind >= GK_RING ? 2 : arith_index(g.bf16));
  if (!out->fn) { set_error("gemm: no kernel instance for this problem"); return LIPASR_EINVAL; }  // (a hole in the table: a bug)
  return LIPASR_OK;
}

int launch_gemm(int amode, int bmode, const GemmArgs& g, hipStream_t st) {
  GemmPick p;
  const int rc = pick_gemm(amode, bmode, g, &p);
  if (rc != LIPASR_OK) return rc;
  if (g.epi >= 0 && g.epi < kEpiCount) {
    const bool exchange = g.epi == EPI_BIAS_RELU_BNX || g.epi == EPI_DH_BNX;
    ++g_gemm_launches[p.kind][exchange ? 1 : 0][amode ? 1 : 0][bmode ? 1 : 0][p.kind >= GK_RING ? 2 : arith_index(g.bf16)][g.epi];
  }
  (void)ensure_dyn_lds(p.fn, p.lds_bytes);
  void* args[] = {const_cast<GemmArgs*>(&g)};
  (void)hipLaunchKernel(p.fn, dim3((g.N + p.tile_n - 1) / p.tile_n, (g.M + p.tile_m - 1) / p.tile_m), dim3(p.threads), args, p.lds_bytes, st);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int gemm_row_tiles(int amode, int bmode, const GemmArgs& g) {
  GemmPick p;
  return pick_gemm(amode, bmode, g, &p) == LIPASR_OK ? (g.M + p.tile_m - 1) / p.tile_m : 0;
}

// The exchange epilogue (EPI_*_BNX) spins until every row tile of its column block has published: every workgroup of the launch
// must be able to be resident at the same time.  Workgroups per CU = the occupancy query capped by the SGPR admission rule,
// times the CUs the plan's stream may use.  The row tiles must also fit the granule regions.  Anything else takes the launch
// chain (GEMM + apply kernel).
static int blocks_per_cu(const GemmPick& p) {
  int occ = 0;
  // the query answers 0 for a dynamic LDS size the kernel has not been allowed yet (launch_gemm raises the limit at a kernel's FIRST
  // launch -- which, for the exchange instances, only happens once this function has said they fit: in a fresh process the first
  // mode-2 training step then took the launch chain for every LDS-tiled layer, found by the launch-count test hook)
  (void)ensure_dyn_lds(p.fn, p.lds_bytes);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, p.fn, p.threads, p.lds_bytes) != hipSuccess) { (void)hipGetLastError(); return 0; }
  // MI355X_MICROARCH.md (residency): the hardware admits 256-thread blocks up to floor(800 / (ceil(sgpr / 16) 16 + 16)) per CU,
  // which the query does not know about (it can be one high).  These kernels use 102-106 SGPRs (GemmArgs is a large by-value
  // argument): 800 / 128 = 6 blocks of four wavefronts = 24 wavefronts per CU.
  const int by_sgpr = 24 / (p.threads / 64);
  return std::min(occ, by_sgpr);
}

// This is DELIBERATELY the conservative bound, kept as it was when the fuse-or-chain decision was measured: it is asked before the
// launch's GemmArgs exist, so it counts 64 x 64 (or 32 x 32) tiles by pick_gemm's own use_lds_gemm although the 128 x 64 instance
// would make half as many, and takes the smaller occupancy of the LDS and the 64 x 64 ring instance although pick_gemm may take
// the loader instances (one workgroup per CU, and only where the tiles are at most the CUs: inside this bound).  A launch this
// admits is resident whichever instance runs it; tightening it changes which layers fuse and needs measurements of its own.
bool exchange_fits(int bmode, int arith, int M, int N, int K, int lds_min_tiles, int xc_rt_max, int cus) {
  const bool lds_k = use_lds_gemm(M, N, K, lds_min_tiles);
  const int ts = lds_k ? 64 : 32;
  const long row_tiles = (M + ts - 1) / ts, tiles = row_tiles * ((N + ts - 1) / ts);
  if (row_tiles > xc_rt_max || row_tiles > 64) return false;
  // [BMODE][fragment | LDS kernel][arithmetic] and the ring instance [BMODE], filled on first use (one device per process in
  // practice; the kernels' resource use does not depend on the device)
  static int per_cu[2][2][3] = {{{-1, -1, -1}, {-1, -1, -1}}, {{-1, -1, -1}, {-1, -1, -1}}}, ring_pc[2] = {-1, -1};
  const int b = bmode ? 1 : 0, ar = arith_index(arith);
  int& pc = per_cu[b][lds_k ? 1 : 0][ar];
  if (pc < 0) pc = blocks_per_cu(gemm_instance(lds_k ? GK_LDS : GK_FRAG4, true, 0, b, ar));
  int per = pc;
  if (ar == 2 && lds_k) {  // the launch may take the LDS-DMA ring instance (68 KB of LDS): the smaller of the two answers
    if (ring_pc[b] < 0) ring_pc[b] = blocks_per_cu(gemm_instance(GK_RING, true, 0, b, 2));
    per = std::min(per, ring_pc[b]);
  }
  return per > 0 && tiles <= (long)per * cus;
}

int launch_gemm_group_tn(const GemmArgs* gs, int n, hipStream_t st) {
  int done = 0;
  while (done < n) {
    GemmGroup grp;
    memset(&grp, 0, sizeof(grp));
    // 64x64 LDS tiles when the group is large enough to fill the chip with them (measured: bench config 3, batch 1024)
    long big = 0;
    for (int k = 0; k < kMaxGroup && done + k < n; ++k)
      big += (long)((gs[done + k].N + 63) / 64) * ((gs[done + k].M + 63) / 64);
    const bool lds_tiles = g_knobs.group_lds && big >= 128 && gs[done].K >= 64;
    const int ts = lds_tiles ? 64 : 32;
    const int ar = gs[done].bf16;
    // 128 x 128 tiles (one workgroup per CU, half the operand bytes per flop, two accumulators per wavefront).  A CU takes in ~32 GB/s
    // whatever asks (LDS-DMA or register loads), so a launch is as long as its busiest CU's bytes: one 128 x 128 tile = 1 MB, two 64 x 64
    // tiles per CU = 1 MB as well but four per CU 2 MB.  The reference's model makes 105 + 4 tiles: with the split pass and the loader
    // wavefronts 38-40 us on a 128-CU share (64 x 64 ring tiles: 77) and config 2's step 0.310 against 0.316 ms on all 256 CUs, where
    // they leave 150 CUs idle -- so: whenever the tiles cover 40 % of the CUs the launch may use.
    int ring_tile = g_knobs.ring_tile;
    if (ring_tile >= 2 && lds_tiles && ar == 2) {
      long n128 = 0;
      for (int q = 0; q < kMaxGroup && done + q < n; ++q)
        if (ring_legal(1, 1, gs[done + q])) n128 += (long)((gs[done + q].N + 127) / 128) * ((gs[done + q].M + 127) / 128);
      if (10 * n128 < 4 * (long)(gs[done].cus > 0 ? gs[done].cus : device_cus())) ring_tile = 1;
    }
    int k = 0, tiles = 0;
    bool any_ring = false;
    for (; k < kMaxGroup && done + k < n; ++k) {
      const GemmArgs& g = gs[done + k];
      if (g.M <= 0 || g.N <= 0 || g.K <= 0) { set_error("grouped gemm: empty problem"); return LIPASR_EINVAL; }
      grp.g[k] = g;
      // arithmetic mode 2: the 128 x 128 two-accumulator ring tile for every problem it can take (ring_tile 1: the 64 x 64 ring tile)
      if (lds_tiles && ar == 2 && ring_legal(1, 1, g)) { grp.g[k].ring = ring_tile; any_ring = true; }
      const int tp = grp.g[k].ring >= 2 ? 128 : ts;
      grp.tile_start[k] = tiles;
      tiles += ((g.N + tp - 1) / tp) * ((g.M + tp - 1) / tp);
    }
    grp.n = k;
    grp.tile_start[k] = tiles;
    const GemmTable& t = gemm_table();
    const void* fn = lds_tiles ? t.grouped_lds[arith_index(ar)] : t.grouped_frag[arith_index(ar)];
    int threads = lds_tiles ? 512 : 256;
    size_t lds = lds_tiles ? lds_gemm_bytes(kLdsBKMax) : frag_gemm_bytes(4);
    if (any_ring) {
      fn = t.grouped_ring;
      // 160 KB of dynamic LDS (the split-pass tile: the whole CU) where the device grants it, else the tile that splits per fragment
      if (ring_tile == 2 && !ensure_dyn_lds(fn, ring128s_bytes())) {  // (never seen on gfx950)
        ring_tile = 3;
        for (int q = 0; q < k; ++q) if (grp.g[q].ring == 2) grp.g[q].ring = 3;
      }
      lds = std::max(ring_gemm_bytes(), ring_tile == 2 ? ring128s_bytes() : ring_tile == 3 ? ring128_bytes() : (size_t)0);
      threads = ring_tile == 2 ? 512 + 64 * kR128Loaders : 512;  // (loader wavefronts: the split-pass tile only)
      ++g_group_launches[2][2];
      ++g_group_ring_launches[ring_tile];
      for (int q = 0; q < k; ++q) ++g_group_ring_problems[grp.g[q].ring & 3];
    } else {
      ++g_group_launches[lds_tiles ? 1 : 0][arith_index(ar)];
    }
    (void)ensure_dyn_lds(fn, lds);
    void* args[] = {&grp};
    (void)hipLaunchKernel(fn, dim3(tiles), dim3(threads), args, lds, st);
    LP_LAUNCH_CHECK();
    done += k;
  }
  return LIPASR_OK;
}

GemmArgs gemm_args(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, int epi) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.epi = epi;
  g.xcd_map = g_knobs.xcd_map;
  g.sa = g.sb = 1.0f;
  return g;
}

}  // namespace lipasr

using namespace lipasr;

extern "C" {

long lipasr_debug_gemm_launches(int kind, int exchange, int amode, int bmode, int arith, int epi) {
  if (kind < 0 || kind >= GK_KINDS || (exchange | amode | bmode) & ~1 || arith < 0 || arith > 2 || epi < -1 || epi >= kEpiCount) return -1;
  if (!gemm_table().fn[kind][exchange][amode][bmode][arith]) return -1;
  const long* c = g_gemm_launches[kind][exchange][amode][bmode][arith];
  if (epi >= 0) return c[epi];
  long n = 0;
  for (int e = 0; e < kEpiCount; ++e) n += c[e];
  return n;
}

long lipasr_debug_group_launches(int family, int arith, int variant) {
  if (family < 0 || family > 2 || arith < 0 || arith > 2) return -1;
  if (family < 2) return variant == -1 ? g_group_launches[family][arith] : -1;
  if (arith != 2 || variant < -1 || variant > 3) return -1;  // the ring kernel is a mode-2 kernel
  return variant == -1 ? g_group_launches[2][2] : g_group_ring_problems[variant];
}

long lipasr_debug_launch_count(int kind) {
  if (kind == 0) return lipasr_debug_gemm_launches(GK_RING2, 1, 0, 0, 2, -1) + lipasr_debug_gemm_launches(GK_RING2, 1, 0, 1, 2, -1);
  return kind == 1 ? g_group_ring_launches[2] : -1;
}

int lipasr_debug_gemm_mode(int mode) {  // the bits: GemmKnobs (gemm.h)
  GemmKnobs k;
  k.gemm_mode = mode & 3;
  k.split_dw0 = (mode >> 2) & 1;
  k.group_lds = !((mode >> 3) & 1);
  k.xcd_map = (mode >> 4) & 1;
  k.no_ring = (mode >> 5) & 1;
  k.ring_tile = ((mode >> 6) & 1) ? 1 : ((mode >> 7) & 1) ? 3 : 2;
  k.ring2 = !((mode >> 8) & 1);
  k.ring_x1 = !((mode >> 9) & 1);
  g_knobs = k;
  return LIPASR_OK;
}

// the stand-alone product in arithmetic `arith`: the checks and the launch of lipasr_gemm_f32 / _f16x2 / lipasr_debug_gemm (`fn` names
// the entry in the error text)
static int gemm_entry(const char* fn, lipasr_handle_t h, int arith, int transA, int transB, int M, int N, int K, const float* A, int lda,
                      const float* B, int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream) {
  LP_CHECK_ARG(h && A && B && C, "%s: null argument", fn);
  LP_CHECK_ARG(arith >= 0 && arith <= 2, "%s: arithmetic mode %d (0 = exact fp32, 1 = bf16 operands, 2 = fp16 two-plane split)", fn, arith);
  LP_CHECK_ARG(M > 0 && N > 0 && K > 0, "%s: empty problem %dx%dx%d", fn, M, N, K);
  LP_CHECK_ARG(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && ldc >= N, "%s: leading dimension too small", fn);
  GemmArgs g = gemm_args(A, lda, B, ldb, C, ldc, M, N, K, EPI_STORE);
  g.bf16 = arith;
  if (arith == 2) {
    int ea = 0, eb = 0;
    LP_CHECK_ARG(scale_a > 0.0f && scale_b > 0.0f && frexpf(scale_a, &ea) == 0.5f && frexpf(scale_b, &eb) == 0.5f,
                 "%s: the scales must be powers of two (got %g, %g)", fn, (double)scale_a, (double)scale_b);
    g.sa = scale_a;
    g.sb = scale_b;
    g.zeros = h->zeros;
  }
  return launch_gemm(transA ? 1 : 0, transB ? 0 : 1, g, S(stream));
}

int lipasr_gemm_f32(lipasr_handle_t h, int transA, int transB, int M, int N, int K, const float* A, int lda,
                    const float* B, int ldb, float* C, int ldc, lipasr_stream_t stream) {
  return gemm_entry("lipasr_gemm_f32", h, 0, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, 1.0f, 1.0f, stream);
}

int lipasr_debug_gemm(lipasr_handle_t h, int arith, int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B,
                      int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream) {
  return gemm_entry("lipasr_debug_gemm", h, arith, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, scale_a, scale_b, stream);
}

int lipasr_gemm_f16x2(lipasr_handle_t h, int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B,
                      int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream) {
  return gemm_entry("lipasr_gemm_f16x2", h, 2, transA, transB, M, N, K, A, lda, B, ldb, C, ldc, scale_a, scale_b, stream);
}

}  // extern "C"
