// K1 backward, short-window path (lipasr_mfcc_plan_vjp_short; gfx950): mel^T, |X|^2, STFT^T and overlap-add for the plans whose
// forward is dft_mel_kernel (stft_mel.hip: n_fft = win_length = 441, hop 220 of Speaker recognition, or any 32 <= n_fft <= 510),
// then the adjoint of the reflect padding.  Step 1 of the chain (DCT^T, top_db floor, dB -> mel) is mfcc_vjp_db_kernel of
// mfcc_vjp.h as it is; the resampler's adjoint is resample_vjp_kernel.  The plan glue is in mfcc.hip.
//
//   dft_vjp_kernel        one workgroup = kSvRows = 32 consecutive frame rows of the forward's virtual padded layout (clip c at
//                         c rpc hop, global row r at r hop, rows >= n_frames of a clip carry nothing), wavefront t = tile t:
//                           a. the rows' samples are staged in LDS with the reflection applied, their Gmel rows next to them;
//                           b. X = frames T on v_mfma_f32_32x32x2_f32 against the folded table, as the forward forms it
//                              (wavefront t owns bins 32 t .. 32 t + 31);
//                           c. GP[b] = sum_m W[m][b] Gmel[m] from the mel bank by bin, ascending m; Z = 2 GP X to LDS (re, im);
//                           d. the second contraction, over the bins, against the table with bins and samples exchanged:
//                              S[n] = sum_b Zre[b] Tre[n][b], A[n] = sum_b Zim[b] Tim[n][b] (wavefront t owns samples 32 t ..);
//                           e. the fold of the table undone: frame sample n gets S[n] + A[n], sample N - n gets S[n] - A[n];
//                              the rows that pair with themselves (n = 0, and n = N/2 for even N; c_n = 1/2 in the table)
//                              get 2 S[n].  The window is inside the table.  The frame gradients go to LDS, [row][N];
//                           f. position p of the workgroup's image sums the frames that cover it in ascending frame order;
//                              a frame whose cotangent row is all zero is left out (its samples receive exactly 0).
//   dft_vjp_fold_kernel   adds the (at most two) images that cover a padded position, in ascending workgroup order, and folds
//                         the two reflected flanks back: g_y[i] = gyp[i + pad] + gyp[pad - i] (1 <= i <= pad) + gyp[pad +
//                         2 (n_y - 1) - i] (n_y - 1 - pad <= i <= n_y - 2), pad = n_fft / 2 (the forward reflects once).
// No floating-point atomics, every sum in a fixed order: two runs give the same bits.
#include "mfcc_plan.h"

namespace lipasr {

// LDS of dft_vjp_kernel in floats: samples | Zre, Zim [32][nb + 1] (then the frame gradients [32][n_fft]) | Gmel [32][128] | flags
static size_t short_vjp_lds_floats(int n_fft, int hop, int n_tiles) {
  return (size_t)(kSvRows - 1) * hop + n_fft + 1 + 2 * (size_t)kSvRows * (n_tiles * 32 + 1) + (size_t)kSvRows * 128 + kSvRows;
}

__global__ __launch_bounds__(64 * kDftMaxTiles) void dft_vjp_kernel(ShortVjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sv[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, n_waves = nthreads >> 6;
  const int N = a.n_fft, nb = a.n_tiles * 32, ldz = nb + 1;  // (odd row stride: the A-operand reads of step d meet 32 banks)
  const int n_a = (kSvRows - 1) * a.hop + N + 1;
  float* xs = sv;                         // [n_a]
  float* zre = xs + n_a;                  // [32][ldz]
  float* zim = zre + kSvRows * ldz;       // [32][ldz]
  float* gms = zim + kSvRows * ldz;       // [32][128]
  int* nz = reinterpret_cast<int*>(gms + kSvRows * 128);  // [32]: the row's cotangent is not all zero
  float* gfr = zre;                       // [32][N] once step d has read Z (2 ldz > N)
  const int row0 = blockIdx.x * kSvRows;
  {
    // a. position g of the virtual padded layout, as dft_mel_kernel stages it (the clip index is found per element)
    const int stride = a.rpc * a.hop, pad = N / 2;
    const long g0 = (long)row0 * a.hop;
    for (int i = tid; i < n_a; i += nthreads) {
      const long g = g0 + i;
      const int c = (int)(g / stride);
      const int j = (int)(g - (long)c * stride);
      float v = 0.0f;
      if (c < a.batch && j < a.n_y + 2 * pad) {
        int k = j - pad;
        if (k < 0) k = -k;
        else if (k >= a.n_y) k = 2 * (a.n_y - 1) - k;
        v = a.y[(size_t)c * a.n_y + k];
      }
      xs[i] = v;
    }
    for (int r = wave; r < kSvRows; r += n_waves) {
      const int grow = row0 + r;
      const int clip = grow / a.rpc, frame = grow - clip * a.rpc;
      float v0 = 0.0f, v1 = 0.0f;
      if (grow < a.total_rows && frame < a.n_frames) {  // wave-uniform
        const float* src = a.gmel + ((size_t)clip * a.n_frames + frame) * 128;
        v0 = src[lane];
        v1 = src[lane + 64];
      }
      gms[r * 128 + lane] = v0;
      gms[r * 128 + lane + 64] = v1;
      const int any = __any(v0 != 0.0f || v1 != 0.0f);
      if (lane == 0) nz[r] = any;
    }
  }
  __syncthreads();
  const int li = lane & 31, kk = lane >> 5;
  const int ld = a.n_tiles * 64;
  rs_f32x16 re, im;
#pragma unroll
  for (int q = 0; q < 16; ++q) { re[q] = 0.f; im[q] = 0.f; }
  {
    // b. row n of the folded table meets x[n] + x[(N - n) mod N] (real part) and x[n] - x[(N - n) mod N] (imaginary part); n = 0
    // meets x[N], one past the frame, under a zero weight, and the padded rows n > N/2 are zero (dft_mel_kernel)
    const float* bp = a.table + (size_t)kk * ld + wave * 64 + li;
    const float* fw = xs + li * a.hop + kk;
    const float* bw = xs + li * a.hop + N - kk;
    const int ks = a.k_rows / 2;  // a multiple of kDftGroup
    for (int s0 = 0; s0 < ks; s0 += kDftGroup) {
#pragma unroll
      for (int u = 0; u < kDftGroup; ++u) {
        const int s = s0 + u;
        const float* q_ = bp + (size_t)(2 * s) * ld;
        const float br = q_[0], bi = q_[32];
        const float p_ = fw[2 * s], m_ = bw[-2 * s];
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(p_ + m_, br, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(p_ - m_, bi, im, 0, 0, 0);
      }
    }
  }
  {
    // c. C layout: row (frame) = (q & 3) + 8 (q >> 2) + 4 kk, column (bin) = li
    const int b = wave * 32 + li;
    const int eo = a.melt_off[b], el = a.melt_len[b];  // (bins past N/2: no filter, X = 0)
    float gp[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) gp[q] = 0.0f;
    for (int e = 0; e < el; ++e) {
      const int m = a.melt_m[eo + e];
      const float w = a.melt_w[eo + e];
#pragma unroll
      for (int q = 0; q < 16; ++q) gp[q] = fmaf(w, gms[((q & 3) + 8 * (q >> 2) + 4 * kk) * 128 + m], gp[q]);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = (q & 3) + 8 * (q >> 2) + 4 * kk;
      const float g2 = 2.0f * gp[q];
      zre[r * ldz + b] = g2 * re[q];
      zim[r * ldz + b] = g2 * im[q];
    }
  }
  __syncthreads();
  rs_f32x16 sa, aa;
#pragma unroll
  for (int q = 0; q < 16; ++q) { sa[q] = 0.f; aa[q] = 0.f; }
  {
    // d. A operand: lane (li, kk) holds Z[row li][bin 2 s + kk]; B operand: the table's weights of sample 32 wave + li for that bin
    const float* tp = a.table_t + (size_t)kk * ld + wave * 64 + li;
    const float* zr = zre + li * ldz + kk;
    const float* zi = zim + li * ldz + kk;
    const int ks = nb / 2;  // a multiple of 16
    for (int s0 = 0; s0 < ks; s0 += kDftGroup) {
#pragma unroll
      for (int u = 0; u < kDftGroup; ++u) {
        const int s = s0 + u;
        const float* q_ = tp + (size_t)(2 * s) * ld;
        sa = __builtin_amdgcn_mfma_f32_32x32x2f32(zr[2 * s], q_[0], sa, 0, 0, 0);
        aa = __builtin_amdgcn_mfma_f32_32x32x2f32(zi[2 * s], q_[32], aa, 0, 0, 0);
      }
    }
  }
  __syncthreads();  // every wavefront has read Z: the buffer becomes the frame gradients
  {
    // e. column = sample n of the folded table
    const int n = wave * 32 + li;
    if (n <= N / 2) {
      const bool self = (n == 0) || (2 * n == N);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float* g = gfr + ((q & 3) + 8 * (q >> 2) + 4 * kk) * N;
        if (self) {
          g[n] = 2.0f * sa[q];
        } else {
          g[n] = sa[q] + aa[q];
          g[N - n] = sa[q] - aa[q];
        }
      }
    }
  }
  __syncthreads();
  // f. image position p <- frames r with 0 <= p - r hop < N, ascending
  float* img = a.part + (size_t)blockIdx.x * a.seg;
  for (int p = tid; p < a.seg; p += nthreads) {
    const int r_lo = p >= N ? (p - N) / a.hop + 1 : 0, r_hi = min(kSvRows - 1, p / a.hop);
    float acc = 0.0f;
    for (int r = r_lo; r <= r_hi; ++r)
      if (nz[r]) acc += gfr[r * N + p - r * a.hop];
    img[p] = acc;
  }
}

// padded position q of clip u: the images of workgroups w - 1 and w that cover it, in that order
__device__ __forceinline__ float sv_gyp(const float* __restrict__ part, int n_wgs, int seg, int span, long base, int q) {
  const long g = base + q;
  const int w = (int)(g / span), off = (int)(g - (long)w * span);
  float s = 0.0f;
  if (w >= 1 && w - 1 < n_wgs && off + span < seg) s = part[(size_t)(w - 1) * seg + span + off];
  if (w < n_wgs) s += part[(size_t)w * seg + off];
  return s;
}

__global__ __launch_bounds__(256) void dft_vjp_fold_kernel(const float* __restrict__ part, int n_wgs, int seg, int hop, int n_fft, int rpc,
                                                            int n_y, float* __restrict__ gy) {
  const int u = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_y) return;
  const int pad = n_fft / 2, span = kSvRows * hop;
  const long base = (long)u * rpc * hop;
  float s = sv_gyp(part, n_wgs, seg, span, base, i + pad);
  if (i >= 1 && i <= pad) s += sv_gyp(part, n_wgs, seg, span, base, pad - i);
  if (i >= n_y - 1 - pad && i <= n_y - 2) s += sv_gyp(part, n_wgs, seg, span, base, pad + 2 * (n_y - 1) - i);
  gy[(size_t)u * n_y + i] = s;
}

int short_vjp_geometry(int n_fft, int hop, int rpc, int n_tiles, int batch, int* n_wgs, int* seg) {
  // the fold adds two images per padded position: an image of 32 frames must not reach past the next one
  if (n_fft > (kSvRows + 1) * hop) {
    set_error("lipasr_mfcc_plan_vjp_short: n_fft %d with hop %d: more than two workgroup images of %d frames would overlap "
              "(the backward pass needs n_fft <= %d hop)", n_fft, hop, kSvRows, kSvRows + 1);
    return LIPASR_EUNSUPPORTED;
  }
  const size_t lds = short_vjp_lds_floats(n_fft, hop, n_tiles) * sizeof(float);
  if (lds > 160 * 1024) {
    set_error("lipasr_mfcc_plan_vjp_short: n_fft %d with hop %d needs %zu bytes of LDS for %d frames (160 KiB per workgroup)", n_fft, hop,
              lds, kSvRows);
    return LIPASR_EUNSUPPORTED;
  }
  *n_wgs = (int)(((long)batch * rpc + kSvRows - 1) / kSvRows);
  *seg = (kSvRows - 1) * hop + n_fft;
  return LIPASR_OK;
}

int launch_short_vjp(const ShortVjpArgs& a, hipStream_t st) {
  int n_wgs, seg;
  const int rc = short_vjp_geometry(a.n_fft, a.hop, a.rpc, a.n_tiles, a.batch, &n_wgs, &seg);
  if (rc != LIPASR_OK) return rc;
  const size_t lds = short_vjp_lds_floats(a.n_fft, a.hop, a.n_tiles) * sizeof(float);
  LP_DYN_LDS(dft_vjp_kernel, lds);
  ShortVjpArgs k = a;
  k.seg = seg;
  hipLaunchKernelGGL(dft_vjp_kernel, dim3(n_wgs), dim3(64 * a.n_tiles), lds, st, k);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_DFT];
  hipLaunchKernelGGL(dft_vjp_fold_kernel, dim3((a.n_y + 255) / 256, a.batch), dim3(256), 0, st, a.part, n_wgs, seg, a.hop, a.n_fft, a.rpc,
                     a.n_y, a.gy);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_DFT_FOLD];
  return LIPASR_OK;
}

}  // namespace lipasr
