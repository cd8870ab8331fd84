// K2, the grouped weight-gradient launch of arithmetic mode 2 (gemm_ring_grouped_kernel): the two 128x128 LDS-DMA ring tiles, with
// the 64x64 ring tile and the 64x64 LDS tile for the problems of a group that cannot take them, and its registration in the GemmTable.
#include "gemm_ring_tile.h"
#include <algorithm>

namespace lipasr {

// ---------------------------------------------------------------------------------------------
// The weight-gradient tile of arithmetic mode 2: 128 x 128 outputs per workgroup, TWO accumulators per wavefront.
// The 64 x 64 ring tile (gemm_ring_tile.h) issues ~75 instructions per wavefront and k-step for 3 matrix instructions (one A and one B fragment
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

// one launch holds 64 x 64 tiles beside its ring tile (GemmArgs::ring: 1 the 64 x 64 ring tile, 2 the split-pass tile, 3 the tile that
// splits per fragment): the larger LDS size; the loader wavefronts belong to the split-pass tile only
void register_gemm_ring_group(GemmTable& t) {
  t.grouped_ring = reinterpret_cast<const void*>(gemm_ring_grouped_kernel);
  t.grouped_ring_shape[1] = {64, 64, 512, ring_gemm_bytes()};
  t.grouped_ring_shape[2] = {128, 128, 512 + 64 * kR128Loaders, std::max(ring_gemm_bytes(), ring128s_bytes())};
  t.grouped_ring_shape[3] = {128, 128, 512, std::max(ring_gemm_bytes(), ring128_bytes())};
}

}  // namespace lipasr
