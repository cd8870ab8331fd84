// K2, the 32x32 fragment tile: gemm_tile, its kernels (one problem per launch, and the grouped weight-gradient launch) and their
// registration in the GemmTable.  The choice of an instance and the launchers are gemm.hip.
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
#include "gemm_device.h"

namespace lipasr {

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
      bnx_row4(g, step, gm1[0] < g.M, gm1[0], gn, accv, xpre, val[0], av[0], c1, c2);
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
      float o[4], dm[4];
      epilogue_dropout4(g, step, gm, gn, dm);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t1 = 0.0f, t2 = 0.0f;
        o[e] = (gn + e < g.N) ? epilogue_elem(g, dm[e], gm, gn + e, v[e], t1, t2) : 0.0f;
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

constexpr size_t frag_gemm_bytes(int nw) { return (size_t)(nw * 32 * 32 + 4 * 8 * 8) * sizeof(float); }

template <int A, int B, int AR> static void reg_frag(GemmTable& t) {
  t.fn[GK_FRAG4][0][A][B][AR] = reinterpret_cast<const void*>(gemm_f32_kernel<A, B, 4, AR>);
  t.fn[GK_FRAG16][0][A][B][AR] = reinterpret_cast<const void*>(gemm_f32_kernel<A, B, 16, AR>);
  if constexpr (A == 0) t.fn[GK_FRAG4][1][0][B][AR] = reinterpret_cast<const void*>(gemm_f32_kernel<0, B, 4, AR, true>);  // the exchange epilogue: forward (NN) or input-gradient (NT) GEMMs only
  if constexpr (A == 1 && B == 1) t.grouped_frag[AR] = reinterpret_cast<const void*>(gemm_f32_grouped_kernel<1, 1, 4, AR>);
}
template <int AR> static void reg_frag_modes(GemmTable& t) {
  reg_frag<0, 0, AR>(t); reg_frag<0, 1, AR>(t); reg_frag<1, 0, AR>(t); reg_frag<1, 1, AR>(t);
}

void register_gemm_frag(GemmTable& t) {
  t.shape[GK_FRAG4] = {32, 32, 64 * 4, frag_gemm_bytes(4)};
  t.shape[GK_FRAG16] = {32, 32, 64 * 16, frag_gemm_bytes(16)};
  t.grouped_frag_shape = t.shape[GK_FRAG4];
  reg_frag_modes<0>(t); reg_frag_modes<1>(t); reg_frag_modes<2>(t);
}

}  // namespace lipasr
