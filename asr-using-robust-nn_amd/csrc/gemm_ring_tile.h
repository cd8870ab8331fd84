// K2: the 64x64 LDS-DMA ring tile (gemm_ring_tile) with its DMA and fragment helpers.  Used by gemm_ring.hip, gemm_ring_group.hip
// (the 64x64 ring problems of a grouped launch) and gemm_ring2.hip (dma16, ring_frag).
#pragma once
#include "gemm_lds_tile.h"

namespace lipasr {

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
// the k (inside a k-step) of the 16 bytes that ring_src's address names: the lanes with k >= K fetch zeros in the last k-step
template <int MODE>
__device__ __forceinline__ int ring_koff(const int wave, const int lane) {
  return MODE == 1 ? 4 * wave + (lane >> 4) : 4 * ((lane & 7) ^ (((8 * wave + (lane >> 3)) >> 1) & 7));
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
  const int koff_a = ring_koff<AMODE>(wave, lane);
  const int koff_b = ring_koff<BMODE>(wave, lane);
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
        ka[q] = ring_koff<AMODE>(w, lane);
        kb[q] = ring_koff<BMODE>(w, lane);
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

}  // namespace lipasr
