// K2, the 128x64 exchange ring tile of arithmetic mode 2 (gemm_ring2_tile), its kernel and its registration in the GemmTable.
#include "gemm_ring_tile.h"

namespace lipasr {

// ---------------------------------------------------------------------------------------------
// The exchange-epilogue GEMMs of arithmetic mode 2 on 128 x 64 tiles (round 5): forward (A = activations, row-major; B = kernel,
// k-major) and input-gradient (B = kernel, K-contiguous) launches whose 64 x 64 tiling would put two or more workgroups on every CU
// of the plan's share.  What bounds the ring kernels on a CU share is the LDS-DMA fill rate of a CU (~32 GB/s: probe 3 of the
// weight-gradient tile in gemm_ring_group.hip), so what counts is bytes per CU: a 128 x 64 tile moves 24 KB per k-step for the work of two 64 x 64
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
    float t1[4], t2[4];
    bnx_row4(g, step, gm4[p4] < g.M, gm4[p4], gn, accv, xpre[p4], val[p4], av[p4], t1, t2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c1[e] += t1[e];
      c2[e] += t2[e];
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

void register_gemm_ring2(GemmTable& t) {
  t.shape[GK_RING2] = {128, 64, 512 + 64 * kR2Loaders, ring2_bytes()};
  t.fn[GK_RING2][1][0][0][2] = reinterpret_cast<const void*>(gemm_ring2_kernel<0>);
  t.fn[GK_RING2][1][0][1][2] = reinterpret_cast<const void*>(gemm_ring2_kernel<1>);
}

}  // namespace lipasr
