// K2: the 64x64 LDS tile (gemm_lds_tile) and the epilogue of a 64x64 tile held as eight 32x32 accumulators (lds_tile_epilogue), which
// the LDS-DMA ring tile shares.  Used by gemm_lds.hip, gemm_ring.hip (the epilogue) and gemm_ring_group.hip (the problems of a
// grouped launch that are not ring-legal).
#pragma once
#include "gemm_device.h"

namespace lipasr {

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
      float t1[4], t2[4];
      bnx_row4(g, step, gm2[pass] < g.M, gm2[pass], gn, accv, xpre[pass], val[pass], av[pass], t1, t2);
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
      float o[4], dm[4];
      epilogue_dropout4(g, step, gm, gn, dm);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t1 = 0.0f, t2 = 0.0f;
        o[e] = (gn + e < g.N) ? epilogue_elem(g, dm[e], gm, gn + e, v[e], t1, t2) : 0.0f;
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

}  // namespace lipasr
