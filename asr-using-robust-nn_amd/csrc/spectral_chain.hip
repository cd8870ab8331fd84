// K3, the product chain: cst = W_m^T ... W_1^T (R x n_0, R = number of classes <= 32) by m-1 skinny steps P <- P * W_k^T, the leading
// small ones in one launch (chain_head_kernel).  The variant as a whole is described in spectral.hip.
#include "spectral.h"

namespace lipasr {

constexpr int kChainRowsPerWave = 1;
constexpr int kChainRowsPerBlock = 4 * kChainRowsPerWave;
constexpr size_t kChainLdsMax = 160 * 1024 - 512;  // chain_step_kernel's dynamic LDS (panel, row sums, Gram slots): the CU's 160 KiB less a margin

// ---------------------------------------------------------------------------------------------
// chain step: P_out[r][i] = sum_j P_in[r][j] * W[i][j],  i < n_rows, j < n_in, r < R
//   p_mode 0: P_in is R x n_in row-major
//   p_mode 1: P_in[r][j] = Wlast[j*R + r]   (P = W_m^T read straight from the last kernel)
//   p_mode 2: P_in = identity (R == n_in)    (single-layer model: P_out = W^T)
// emit_gram: also write this block's partial Gram  sum_i P_out[:,i] P_out[:,i]^T  (fp64, R*R)
// ---------------------------------------------------------------------------------------------
template <int RM>  // compile-time bound on R: keeps the unrolled body (and the instruction footprint) small
__global__ __launch_bounds__(256) void chain_step_kernel(const float* __restrict__ Pin, int p_mode,
                                                          const float* __restrict__ W, int n_rows, int n_in, int R,
                                                          float* __restrict__ Pout, int emit_gram,
                                                          double* __restrict__ gram_part) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Ps = reinterpret_cast<float*>(smem_raw);                      // [R][n_in]
  float* rowsum = Ps + (size_t)R * n_in;                               // [4][32]
  double* gsm = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(rowsum + 4 * kMaxR) + 7) & ~uintptr_t(7));  // [4][R*R]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int total = R * n_in;
  // this wavefront's weight row starts its trip from L2/HBM before P is staged (first 1024 columns in registers)
  const bool vec = ((n_in & 3) == 0) && ((reinterpret_cast<uintptr_t>(W) & 15) == 0);
  const int i_pref = blockIdx.x * kChainRowsPerBlock + wave * kChainRowsPerWave;
  float4 wpre[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane * 4 + 256 * t;
    wpre[t] = (vec && i_pref < n_rows && j < n_in) ? *reinterpret_cast<const float4*>(W + (size_t)i_pref * n_in + j)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (p_mode == 0) {
    if ((total & 3) == 0 && (reinterpret_cast<uintptr_t>(Pin) & 15) == 0) {
      const float4* src = reinterpret_cast<const float4*>(Pin);
      float4* dst = reinterpret_cast<float4*>(Ps);
      const int t4 = total >> 2;
#pragma unroll 4
      for (int f = tid; f < t4; f += 256) dst[f] = src[f];
    } else {
      for (int f = tid; f < total; f += 256) Ps[f] = Pin[f];
    }
  } else if (p_mode == 1) {
    for (int f = tid; f < total; f += 256) {
      int j = f / R, r = f - j * R;
      Ps[r * n_in + j] = Pin[f];
    }
  } else {
    for (int f = tid; f < total; f += 256) {
      int r = f / n_in, j = f - r * n_in;
      Ps[f] = (r == j) ? 1.0f : 0.0f;
    }
  }
  const int RR = R * R;
  double gacc[(RM * RM + 63) / 64];
#pragma unroll
  for (int q = 0; q < (RM * RM + 63) / 64; ++q) gacc[q] = 0.0;
  __syncthreads();

  for (int rr = 0; rr < kChainRowsPerWave; ++rr) {
    const int i = blockIdx.x * kChainRowsPerBlock + wave * kChainRowsPerWave + rr;
    const bool live = i < n_rows;  // wave-uniform
    float acc[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) acc[r] = 0.0f;
    if (live) {
      const float* wrow = W + (size_t)i * n_in;
      if (vec) {
        int tt = 0;
        for (int j = lane * 4; j < n_in; j += 256, ++tt) {
          float4 w;
          if (rr == 0 && tt < 4) w = (tt == 0) ? wpre[0] : (tt == 1) ? wpre[1] : (tt == 2) ? wpre[2] : wpre[3];
          else w = *reinterpret_cast<const float4*>(wrow + j);
#pragma unroll
          for (int r = 0; r < RM; ++r) {
            if (r < R) {
              const float4 p = *reinterpret_cast<const float4*>(Ps + r * n_in + j);
              acc[r] = fmaf(w.x, p.x, acc[r]);
              acc[r] = fmaf(w.y, p.y, acc[r]);
              acc[r] = fmaf(w.z, p.z, acc[r]);
              acc[r] = fmaf(w.w, p.w, acc[r]);
            }
          }
        }
      } else {
        for (int j = lane; j < n_in; j += 64) {
          const float w = wrow[j];
#pragma unroll
          for (int r = 0; r < RM; ++r)
            if (r < R) acc[r] = fmaf(w, Ps[r * n_in + j], acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RM; ++r)
      if (r < R) acc[r] = wave_sum(acc[r]);
    if (live && lane == 0) {
#pragma unroll
      for (int r = 0; r < RM; ++r)
        if (r < R) Pout[(size_t)r * n_rows + i] = acc[r];
    }
    if (emit_gram) {
      // publish this row's R sums to the wave's LDS slot, then each lane adds its Gram entries
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RM; ++r)
          if (r < R) rowsum[wave * kMaxR + r] = live ? acc[r] : 0.0f;
      }
      __builtin_amdgcn_wave_barrier();
      __threadfence_block();
#pragma unroll
      for (int q = 0; q < (RM * RM + 63) / 64; ++q) {
        const int e = lane + 64 * q;
        if (e < RR) {
          const int a = e / R, b = e - a * R;
          gacc[q] += (double)rowsum[wave * kMaxR + a] * (double)rowsum[wave * kMaxR + b];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (emit_gram) {
#pragma unroll
    for (int q = 0; q < (RM * RM + 63) / 64; ++q) {
      const int e = lane + 64 * q;
      if (e < RR) gsm[wave * RR + e] = gacc[q];
    }
    __syncthreads();
    for (int e = tid; e < RR; e += 256)
      gram_part[(size_t)blockIdx.x * RR + e] = (gsm[e] + gsm[RR + e]) + (gsm[2 * RR + e] + gsm[3 * RR + e]);
  }
}

// ---------------------------------------------------------------------------------------------
// The first (small) chain steps in ONE launch.  The chain starts at the narrow end of the network: W_m^T is R x 64, the
// next kernels are 128 x 64, 256 x 128, 512 x 256 -- 0.7 MB of weights and 1.7 M multiply-adds that cost three dependent
// launches of 6-7 us each (round trips, not work).  Here every workgroup (512 threads) recomputes the leading products
// P_1 ... P_(n-1) in full in its own LDS and then its own 128 rows of the last fused step, which it writes out; the remaining
// (large) steps run as chain_step_kernel launches on that output.  Recomputing is only cheap on the matrix pipe: a step is
// P_next^T [rows x R] = W [rows x n_in] . P^T [n_in x R], one v_mfma_f32_16x16x4_f32 tile per 16 weight rows (exact fp32, an fmaf
// chain along k; R <= 16 in the tile's columns), the weight fragments of a tile loaded in one go and the next tile's -- of the next
// step too, they do not depend on P -- fetched while this one multiplies.  (A first version kept chain_step_kernel's
// arithmetic -- a wavefront per row, ten wave reductions per row -- and was bitwise equal to the separate launches, but
// 400 rows x 170 instructions per workgroup took 90 us; round 3's version ran all rows through ONE workgroup: +192 us.)
// The sums are associated differently from chain_step_kernel's, so the product differs from the per-step launches in the
// last bits (1e-7); every replica runs the same code.
// ---------------------------------------------------------------------------------------------
constexpr int kHeadMax = 3;
constexpr int kHeadQ = 16;   // k-blocks of 16 per tile row: n_in <= 256
typedef float head_f32x4 __attribute__((ext_vector_type(4)));
struct ChainHead {
  int n;                      // fused steps (>= 2)
  const float* W[kHeadMax];   // step s: n_rows[s] x n_in[s], row-major, n_in a multiple of 16
  int n_rows[kHeadMax];
  int n_in[kHeadMax];         // n_in[s + 1] == n_rows[s]
  const float* Wlast;         // P_0[r][j] = Wlast[j * R + r]
  int R;                      // <= 16
  float* Pout;                // R x n_rows[n - 1]
  int rows_per_block;         // of the last fused step (128: one tile per wavefront)
};

__device__ __forceinline__ void head_load(const float* __restrict__ W, int n_rows, int n_in, int i0, int lane, float4 (&a)[kHeadQ]) {
  const int row = i0 + (lane & 15);
  const float* p = W + (size_t)min(row, n_rows - 1) * n_in + 4 * (lane >> 4);
#pragma unroll
  for (int q = 0; q < kHeadQ; ++q) {
    if (16 * q < n_in) {
      a[q] = *reinterpret_cast<const float4*>(p + 16 * q);
      if (row >= n_rows) a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

// one 16-row tile: acc[reg] = P_next[r = lane & 15][i0 + 4 (lane >> 4) + reg].  T: [16][n_in + 4] in LDS, rows >= R zero
__device__ __forceinline__ head_f32x4 head_tile(const float4 (&a)[kHeadQ], const float* __restrict__ T, int n_in, int lane) {
  head_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* t = T + (lane & 15) * (n_in + 4) + 4 * (lane >> 4);
#pragma unroll
  for (int q = 0; q < kHeadQ; ++q) {
    if (16 * q < n_in) {
      const float4 b = *reinterpret_cast<const float4*>(t + 16 * q);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q].w, b.w, acc, 0, 0, 0);
    }
  }
  return acc;
}

__global__ __launch_bounds__(512) void chain_head_kernel(ChainHead a) {
  extern __shared__ __attribute__((aligned(16))) float hs[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = a.R;
  // the tile sequence of this wavefront: step s < n - 1: tiles wave, wave + 8, ... of n_rows[s] / 16; last step: the tiles of this
  // workgroup's rows.  The first tile's weights start their trip before P_0 is staged.
  float4 cur[kHeadQ], nxt[kHeadQ];
  const int last_i0 = blockIdx.x * a.rows_per_block, last_i1 = min(a.n_rows[a.n - 1], last_i0 + a.rows_per_block);
  auto first_tile = [&](int s) { return (s + 1 < a.n) ? 16 * wave : last_i0 + 16 * wave; };
  auto end_row = [&](int s) { return (s + 1 < a.n) ? a.n_rows[s] : last_i1; };
  if (first_tile(0) < end_row(0)) head_load(a.W[0], a.n_rows[0], a.n_in[0], first_tile(0), lane, cur);
  float* Pin = hs;
  {
    const int ld = a.n_in[0] + 4;
    for (int f = tid; f < 16 * ld; f += 512) Pin[f] = 0.0f;
    __syncthreads();
    const int total = R * a.n_in[0];
    for (int f = tid; f < total; f += 512) {
      const int j = f / R, r = f - j * R;
      Pin[r * ld + j] = a.Wlast[f];
    }
  }
  __syncthreads();
  for (int s = 0; s < a.n; ++s) {
    const int n_in = a.n_in[s], n_rows = a.n_rows[s];
    const bool last = (s + 1 == a.n);
    float* Pnext = Pin + 16 * (n_in + 4);
    const int ldn = n_rows + 4;
    if (!last) {  // rows >= R of the next panel stay zero (the tile's columns R .. 15 multiply them)
      for (int f = tid + R * ldn; f < 16 * ldn; f += 512) Pnext[f] = 0.0f;
    }
    const int e = end_row(s);
    for (int i0 = first_tile(s); i0 < e; i0 += 128) {
      // the weights of this wavefront's next tile -- of this step, or the first one of the next step
      const bool more = i0 + 128 < e;
      if (more) head_load(a.W[s], n_rows, n_in, i0 + 128, lane, nxt);
      else if (!last && first_tile(s + 1) < end_row(s + 1)) head_load(a.W[s + 1], a.n_rows[s + 1], a.n_in[s + 1], first_tile(s + 1), lane, nxt);
      const head_f32x4 acc = head_tile(cur, Pin, n_in, lane);
      const int r = lane & 15, ib = i0 + 4 * (lane >> 4);
      if (r < R) {
        if (!last) {
          *reinterpret_cast<float4*>(Pnext + r * ldn + ib) = make_float4(acc[0], acc[1], acc[2], acc[3]);  // (rows past n_rows: zero weights -> zeros, inside the padding)
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (ib + q < n_rows) a.Pout[(size_t)r * n_rows + ib + q] = acc[q];
        }
      }
#pragma unroll
      for (int q = 0; q < kHeadQ; ++q) cur[q] = nxt[q];
    }
    if (!last) {
      if (!(first_tile(s) < e) && first_tile(s + 1) < end_row(s + 1))  // this wavefront had no tile in step s: nobody fetched its next one
        head_load(a.W[s + 1], a.n_rows[s + 1], a.n_in[s + 1], first_tile(s + 1), lane, cur);
      __syncthreads();
      Pin = Pnext;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int g_chain_head = -1;  // lipasr_debug_chain_head: -1 the two leading steps when legal, 0 none, n > 0 at most n (<= 3)

template <int RM, K3Kernel ID>
static int launch_chain_step(int blocks, size_t lds, hipStream_t st, const float* pin, int p_mode, const float* Wk, int n_rows,
                             int n_in, int R, float* pout, int emit, double* gram) {
  LP_DYN_LDS(chain_step_kernel<RM>, lds);
  hipLaunchKernelGGL(chain_step_kernel<RM>, dim3(blocks), dim3(256), lds, st, pin, p_mode, Wk, n_rows, n_in, R, pout, emit, gram);
  k3_count(ID);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int launch_chain(lipasr_ctx* h, const float* const* Ws, const int* rows, const int* cols, int m, ChainScratch* cs, int* n_part_out,
                 hipStream_t st, bool want_gram, const float** p_final) {
  const int R = cols[m - 1];
  if (R > kMaxR) {
    set_error("product chain: last layer has %d outputs; the Gram eigen-solver handles at most %d", R, kMaxR);
    return LIPASR_EUNSUPPORTED;
  }
  int max_width = 0;
  for (int l = 0; l < m; ++l) max_width = rows[l] > max_width ? rows[l] : max_width;
  int rc = carve_chain_scratch(h, R, max_width, cs);
  if (rc != LIPASR_OK) return rc;

  const float* pin = Ws[m - 1];
  int p_mode = 1;
  int cur = 0;
  if (m == 1) {
    // P = W_1^T: run one step against the identity so the Gram falls out of the same kernel
    pin = nullptr;
    p_mode = 2;
  }
  int first_k = (m == 1) ? 0 : m - 2;
  // the leading small steps as one launch (chain_head_kernel): steps first_k ... first_k - n + 1, never the last step (k = 0,
  // which may emit the Gram partials); R <= 16, panels of <= 256 columns in multiples of 16
  if (m >= 4 && g_chain_head != 0 && R <= 16) {
    int n = 0;
    while (n < kHeadMax && first_k - n >= 1 && cols[first_k - n] <= 16 * kHeadQ && (cols[first_k - n] & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(Ws[first_k - n]) & 15) == 0)
      ++n;
    // measured (MI355X, reference widths, rocprofv3): two fused steps 7.2 us against 2 x 6.2, three 15.5 against 3 x 6.3 (the third
    // step's 96 extra matrix instructions per wavefront cost 8 us on the 4 CUs the launch occupies): two unless told otherwise
    if (n > (g_chain_head > 0 ? g_chain_head : 2)) n = (g_chain_head > 0 ? g_chain_head : 2);
    if (n >= 2) {
      ChainHead a;
      memset(&a, 0, sizeof(a));
      a.n = n;
      size_t lds_f = 0;
      for (int s2 = 0; s2 < n; ++s2) {
        a.W[s2] = Ws[first_k - s2];
        a.n_rows[s2] = rows[first_k - s2];
        a.n_in[s2] = cols[first_k - s2];
        lds_f += (size_t)16 * (a.n_in[s2] + 4);
      }
      a.Wlast = Ws[m - 1];
      a.R = R;
      a.Pout = cs->P[cur];
      a.rows_per_block = 128;
      const int blocks = (a.n_rows[n - 1] + a.rows_per_block - 1) / a.rows_per_block;
      const size_t lds = lds_f * sizeof(float);
      LP_DYN_LDS(chain_head_kernel, lds);
      hipLaunchKernelGGL(chain_head_kernel, dim3(blocks), dim3(512), lds, st, a);
      k3_count(K3_CHAIN_HEAD);
      LP_LAUNCH_CHECK();
      pin = cs->P[cur];
      p_mode = 0;
      cur ^= 1;
      first_k -= n;
    }
  }
  for (int k = first_k; k >= 0; --k) {
    // step k multiplies by W_k^T: rows of W_k are the new columns of P
    const int n_rows = rows[k];
    const int n_in = (m == 1) ? R : cols[k];
    const int emit = (k == 0 && want_gram) ? 1 : 0;
    const int blocks = (n_rows + kChainRowsPerBlock - 1) / kChainRowsPerBlock;
    const size_t lds = (size_t)R * n_in * sizeof(float) + 4 * kMaxR * sizeof(float) +
                       (emit ? (size_t)4 * R * R * sizeof(double) : 0) + 16;
    if (lds > kChainLdsMax) {
      set_error("product chain: %d x %d panel does not fit LDS", R, n_in);
      return LIPASR_EUNSUPPORTED;
    }
    if (emit && (size_t)blocks * R * R > cs->gram_cap_doubles) {
      set_error("product chain: Gram partials exceed scratch");
      return LIPASR_EUNSUPPORTED;
    }
    const float* Wk = (m == 1) ? Ws[0] : Ws[k];
    const auto step = R <= 12   ? launch_chain_step<12, K3_CHAIN_STEP_12>
                      : R <= 20 ? launch_chain_step<20, K3_CHAIN_STEP_20>
                                : launch_chain_step<32, K3_CHAIN_STEP_32>;
    rc = step(blocks, lds, st, pin, p_mode, Wk, n_rows, n_in, R, cs->P[cur], emit, cs->gram);
    if (rc != LIPASR_OK) return rc;
    if (emit) *n_part_out = blocks;
    if (k == 0 && p_final) *p_final = cs->P[cur];
    pin = cs->P[cur];
    p_mode = 0;
    cur ^= 1;
  }
  return LIPASR_OK;
}

}  // namespace lipasr

extern "C" int lipasr_debug_chain_head(int n) {
  lipasr::g_chain_head = n < 0 ? -1 : (n > lipasr::kHeadMax ? lipasr::kHeadMax : n);
  return LIPASR_OK;
}
