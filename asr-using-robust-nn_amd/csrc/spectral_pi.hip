// K3, the per-layer variant: power iteration on W^T W, all layers batched in each launch (described in spectral.hip).
#include "spectral.h"

namespace lipasr {

// ---------------------------------------------------------------------------------------------
// power iteration, all layers per launch
// ---------------------------------------------------------------------------------------------
struct PiArgs {
  int n_layers;
  const float* W[LIPASR_MAX_LAYERS];
  int rows[LIPASR_MAX_LAYERS];
  int cols[LIPASR_MAX_LAYERS];
  float* v[LIPASR_MAX_LAYERS];   // [cols]
  float* u[LIPASR_MAX_LAYERS];   // [rows]
  int blk_u[LIPASR_MAX_LAYERS + 1];  // block prefix for the u kernel (8 rows per block)
  int blk_v[LIPASR_MAX_LAYERS + 1];  // block prefix for the v kernel (32 columns per block)
  int clamp;
};

constexpr int kPiMaxDim = 8192;

__device__ __forceinline__ int find_layer(const int* prefix, int n, int blk) {
  int l = 0;
  while (l + 1 < n && blk >= prefix[l + 1]) ++l;
  return l;
}

__device__ __forceinline__ float start_vec(int j) {
  // fixed, strictly positive start vector (Perron direction for the clamped kernels)
  return 1.0f + 0.001f * (float)((((unsigned)j * 2654435761u) >> 24) & 255u);
}

__device__ __forceinline__ float block_sum_256(float x, float* red) {
  x = wave_sum(x);
  const int tid = threadIdx.x;
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// u = max(W,0)? * (v / ||v||)
__global__ __launch_bounds__(256) void pi_u_kernel(PiArgs a, int cold) {
  __shared__ __attribute__((aligned(16))) float vs[kPiMaxDim];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = find_layer(a.blk_u, a.n_layers, blockIdx.x);
  const int rows = a.rows[l], cols = a.cols[l];
  const float* W = a.W[l];
  float ss = 0.0f;
  for (int j = tid; j < cols; j += 256) {
    const float x = cold ? start_vec(j) : a.v[l][j];
    vs[j] = x;
    ss = fmaf(x, x, ss);
  }
  const float nv2 = block_sum_256(ss, red);
  const float inv = nv2 > 0.0f ? 1.0f / sqrtf(nv2) : 0.0f;
  const bool vec = ((cols & 3) == 0) && ((reinterpret_cast<uintptr_t>(W) & 15) == 0);
  const int row0 = (blockIdx.x - a.blk_u[l]) * 8 + wave * 2;
  for (int rr = 0; rr < 2; ++rr) {
    const int i = row0 + rr;
    if (i >= rows) break;  // wave-uniform
    const float* wrow = W + (size_t)i * cols;
    float acc = 0.0f;
    if (vec) {
      for (int j = lane * 4; j < cols; j += 256) {
        float4 w = *reinterpret_cast<const float4*>(wrow + j);
        const float4 p = *reinterpret_cast<const float4*>(vs + j);
        if (a.clamp) { w.x = fmaxf(w.x, 0.f); w.y = fmaxf(w.y, 0.f); w.z = fmaxf(w.z, 0.f); w.w = fmaxf(w.w, 0.f); }
        acc = fmaf(w.x, p.x, acc); acc = fmaf(w.y, p.y, acc); acc = fmaf(w.z, p.z, acc); acc = fmaf(w.w, p.w, acc);
      }
    } else {
      for (int j = lane; j < cols; j += 64) {
        float w = wrow[j];
        if (a.clamp) w = fmaxf(w, 0.f);
        acc = fmaf(w, vs[j], acc);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) a.u[l][i] = acc * inv;
  }
}

// v = max(W,0)?^T u   (unnormalised; the next pi_u normalises)
__global__ __launch_bounds__(256) void pi_v_kernel(PiArgs a) {
  __shared__ float us[kPiMaxDim];
  __shared__ float part[8][33];
  const int tid = threadIdx.x, cx = tid & 31, ry = tid >> 5;
  const int l = find_layer(a.blk_v, a.n_layers, blockIdx.x);
  const int rows = a.rows[l], cols = a.cols[l];
  const float* W = a.W[l];
  for (int i = tid; i < rows; i += 256) us[i] = a.u[l][i];
  __syncthreads();
  const int j = (blockIdx.x - a.blk_v[l]) * 32 + cx;
  float acc = 0.0f;
  if (j < cols) {
#pragma unroll 4
    for (int i = ry; i < rows; i += 8) {
      float w = W[(size_t)i * cols + j];
      if (a.clamp) w = fmaxf(w, 0.f);
      acc = fmaf(w, us[i], acc);
    }
  }
  part[ry][cx] = acc;
  __syncthreads();
  if (ry == 0 && j < cols) {
    float s = ((part[0][cx] + part[1][cx]) + (part[2][cx] + part[3][cx])) +
              ((part[4][cx] + part[5][cx]) + (part[6][cx] + part[7][cx]));
    a.v[l][j] = s;
  }
}

// sigma_l = ||u_l|| (u = W v_hat); optionally W_l <- max(W_l,0) * c / (sigma_l + eps).  blockIdx.y = layer.
__global__ __launch_bounds__(256) void pi_finish_kernel(PiArgs a, double c, int do_scale, float* __restrict__ sigmas_out) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int l = blockIdx.y;
  const int rows = a.rows[l], cols = a.cols[l];
  float ss = 0.0f;
  for (int i = tid; i < rows; i += 256) {
    const float x = a.u[l][i];
    ss = fmaf(x, x, ss);
  }
  const float s2 = block_sum_256(ss, red);
  const float sigma = sqrtf(s2);
  if (blockIdx.x == 0 && tid == 0) sigmas_out[l] = sigma;
  if (!do_scale) return;
  const double f = c / ((double)sigma + kEps);
  float* w = const_cast<float*>(a.W[l]);
  const size_t n = (size_t)rows * cols;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n; i += stride) {
    const float x = fmaxf(w[i], 0.0f);
    w[i] = (float)((double)x * f);
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int fill_pi_args(PiArgs* a, lipasr_ctx* h, const float* const* Ws, const int* rows, const int* cols, int n_layers,
                        float* v_state, int clamp) {
  size_t u_floats = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (rows[l] > kPiMaxDim || cols[l] > kPiMaxDim) {
      set_error("power iteration: kernel %d is %dx%d; dimensions above %d are not supported", l, rows[l], cols[l],
                kPiMaxDim);
      return LIPASR_EUNSUPPORTED;
    }
    u_floats += (rows[l] + 3) & ~3;
  }
  float* u_scratch = carve_pi_left(h, u_floats);
  if (!u_scratch) return LIPASR_EUNSUPPORTED;
  a->n_layers = n_layers;
  a->clamp = clamp;
  size_t voff = 0, uoff = 0;
  a->blk_u[0] = 0;
  a->blk_v[0] = 0;
  for (int l = 0; l < n_layers; ++l) {
    a->W[l] = Ws[l];
    a->rows[l] = rows[l];
    a->cols[l] = cols[l];
    a->v[l] = v_state + voff;
    a->u[l] = u_scratch + uoff;
    voff += cols[l];
    uoff += (rows[l] + 3) & ~3;
    a->blk_u[l + 1] = a->blk_u[l] + (rows[l] + 7) / 8;
    a->blk_v[l + 1] = a->blk_v[l] + (cols[l] + 31) / 32;
  }
  return LIPASR_OK;
}

static int run_power_iteration(PiArgs& a, int warm, int iters, hipStream_t st) {
  const int nbu = a.blk_u[a.n_layers], nbv = a.blk_v[a.n_layers];
  int cold = warm ? 0 : 1;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(pi_u_kernel, dim3(nbu), dim3(256), 0, st, a, cold);
    k3_count(K3_PI_U);
    LP_LAUNCH_CHECK();
    cold = 0;
    hipLaunchKernelGGL(pi_v_kernel, dim3(nbv), dim3(256), 0, st, a);
    k3_count(K3_PI_V);
    LP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pi_u_kernel, dim3(nbu), dim3(256), 0, st, a, cold);
  k3_count(K3_PI_U);
  LP_LAUNCH_CHECK();
  if (cold) {
    // iters == 0 on a cold start: still leave a defined warm-start vector behind
    hipLaunchKernelGGL(pi_v_kernel, dim3(nbv), dim3(256), 0, st, a);
    k3_count(K3_PI_V);
    LP_LAUNCH_CHECK();
  }
  return LIPASR_OK;
}

// sigma only: one workgroup per layer; with the rescaling 64 per layer
static int launch_pi_finish(const PiArgs& a, double c, int do_scale, float* sigmas_out, hipStream_t st) {
  hipLaunchKernelGGL(pi_finish_kernel, dim3(do_scale ? 64 : 1, a.n_layers), dim3(256), 0, st, a, c, do_scale, sigmas_out);
  k3_count(K3_PI_FINISH);
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

int launch_power_iteration(lipasr_ctx* h, const float* const* Ws, const int* rows, const int* cols, int n_layers, float* v_state,
                           int clamp, int warm, int iters, double c, int do_scale, float* sigmas_out, hipStream_t st) {
  PiArgs a;
  int rc = fill_pi_args(&a, h, Ws, rows, cols, n_layers, v_state, clamp);
  if (rc != LIPASR_OK) return rc;
  rc = run_power_iteration(a, warm, iters, st);
  if (rc != LIPASR_OK) return rc;
  return launch_pi_finish(a, c, do_scale, sigmas_out, st);
}

}  // namespace lipasr
