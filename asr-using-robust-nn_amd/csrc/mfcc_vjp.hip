// K1 backward for clips of one length: the instances of the kernels in mfcc_vjp.h that read no length array, and the launchers
// (plan_vjp in mfcc.hip is the one chain that calls them; lipasr_mfcc_plan_resample_vjp runs the last alone).  With per-clip
// lengths the launchers hand over to mfcc_vjp_ragged.hip.
#include "mfcc_vjp.h"
#include "mfcc_plan.h"

namespace lipasr {

__global__ __launch_bounds__(256) void copy_cut_kernel(const float* __restrict__ gy, int n_y, float* __restrict__ gx, int n_samp) {
  const int u = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j < n_samp) gx[(size_t)u * n_samp + j] = j < n_y ? gy[(size_t)u * n_y + j] : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// LDS of mfcc_vjp_db_kernel: the cotangent of one clip
static int vjp_db_lds(const MfccVjpArgs& a, size_t* lds) {
  const int Tc = std::min(a.n_frames, a.L);
  *lds = (size_t)kNMfcc * Tc * sizeof(float);
  if (*lds > 40 * 1024) {
    set_error("lipasr_mfcc_plan_vjp: utterance_length %d with %d frames needs %zu bytes of LDS", a.L, a.n_frames, *lds);
    return LIPASR_EUNSUPPORTED;
  }
  return LIPASR_OK;
}

int launch_mfcc_vjp_db(const MfccVjpArgs& a, hipStream_t st) {
  size_t lds;
  const int rc = vjp_db_lds(a, &lds);
  if (rc != LIPASR_OK) return rc;
  hipLaunchKernelGGL(mfcc_vjp_db_kernel<false>, dim3(a.batch), dim3(256), lds, st, a);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_DB];
  return LIPASR_OK;
}

int launch_mfcc_vjp(const MfccVjpArgs& a, hipStream_t st, const int* n_valid, int sr_in, int n_samp_max) {
  if (n_valid) {
    size_t lds;
    const int rc = vjp_db_lds(a, &lds);
    return rc != LIPASR_OK ? rc : launch_mfcc_vjp_ragged(a, lds, n_valid, sr_in, n_samp_max, st);
  }
  const int rc = launch_mfcc_vjp_db(a, st);
  if (rc != LIPASR_OK) return rc;
  const dim3 fold_grid((a.n_y + 255) / 256, a.batch);
  hipLaunchKernelGGL(stft_vjp_kernel<false>, dim3(a.n_groups, a.batch), dim3(256), 0, st, a);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_STFT];
  hipLaunchKernelGGL(stft_vjp_fold_kernel<false>, fold_grid, dim3(256), 0, st, a.part, a.n_groups, a.n_y, a.gy, n_valid, n_samp_max, sr_in,
                     a.n_frames);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_FOLD];
  return LIPASR_OK;
}

int launch_resample_vjp(const ResampleVjpArgs& a, const float* gy, float* gx, int batch, hipStream_t st) {
  if (a.identity) {
    hipLaunchKernelGGL(copy_cut_kernel, dim3((a.n_samp + 255) / 256, batch), dim3(256), 0, st, gy, a.n_y, gx, a.n_samp);
    LP_LAUNCH_CHECK();
    ++g_k1_vjp_launches[K1V_COPY_CUT];
    return LIPASR_OK;
  }
  const int threads = std::min(1024, ((a.down + 63) / 64) * 64), zs = (a.down + threads - 1) / threads;
  const int nq = (a.n_samp + a.down - 1) / a.down;
  const int span = a.t0max - a.t0min + a.nt;  // window of one q'
  constexpr int kQ = kVjResampleQ;
  K1VjpKernel kid = K1V_RESAMPLE_Q8;
  const size_t lds8 = (size_t)((kQ - 1) * a.up + span) * sizeof(float), lds1 = (size_t)span * sizeof(float);
  if (lds8 <= 60 * 1024) {
    const dim3 grid((nq + kQ - 1) / kQ, batch, zs);
    const int win = (int)(lds8 / sizeof(float));
    if (a.nv) return launch_resample_vjp_ragged(a, gy, gx, grid, threads, lds8, win, true, st);
    hipLaunchKernelGGL((resample_vjp_kernel<kQ, false>), grid, dim3(threads), lds8, st, gy, a.n_y, a.n_valid, gx, a.n_samp, a.up, a.down,
                       a.ht, a.t0, a.nt, a.t0min, win, VjNoClip{});
    kid = K1V_RESAMPLE_Q8;
  } else if (lds1 <= 60 * 1024) {
    if (a.nv) return launch_resample_vjp_ragged(a, gy, gx, dim3(nq, batch, zs), threads, lds1, span, false, st);
    hipLaunchKernelGGL((resample_vjp_kernel<1, false>), dim3(nq, batch, zs), dim3(threads), lds1, st, gy, a.n_y, a.n_valid, gx, a.n_samp,
                       a.up, a.down, a.ht, a.t0, a.nt, a.t0min, span, VjNoClip{});
    kid = K1V_RESAMPLE_Q1;
  } else {
    set_error("lipasr_mfcc_plan_resample_vjp: ratio %d/%d needs a %zu-byte window; unsupported", a.up, a.down, lds1);
    return LIPASR_EUNSUPPORTED;
  }
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[kid];
  return LIPASR_OK;
}

}  // namespace lipasr
