// K1 backward for clips of different lengths in one launch (lipasr_mfcc_plan_vjp_ragged): the RAGGED instances of the kernels
// in mfcc_vjp.h, in a translation unit of their own (see the note there).
#include "mfcc_vjp.h"
#include "mfcc_plan.h"

namespace lipasr {

int launch_mfcc_vjp_ragged(const MfccVjpArgs& a, size_t lds, const int* n_valid, int sr_in, int n_samp_max, hipStream_t st) {
  MfccVjpRaggedArgs r;
  static_cast<MfccVjpArgs&>(r) = a;
  r.n_valid = n_valid; r.sr_in = sr_in; r.n_samp_max = n_samp_max;
  hipLaunchKernelGGL(mfcc_vjp_db_kernel<true>, dim3(a.batch), dim3(256), lds, st, r);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_DB_RAGGED];
  hipLaunchKernelGGL(stft_vjp_kernel<true>, dim3(a.n_groups, a.batch), dim3(256), 0, st, r);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_STFT_RAGGED];
  hipLaunchKernelGGL(stft_vjp_fold_kernel<true>, dim3((a.n_y + 255) / 256, a.batch), dim3(256), 0, st, a.part, a.n_groups, a.n_y, a.gy,
                     n_valid, n_samp_max, sr_in, a.n_frames);
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[K1V_FOLD_RAGGED];
  return LIPASR_OK;
}

// q8: the kVjResampleQ-outputs-per-thread form (else one)
int launch_resample_vjp_ragged(const ResampleVjpArgs& a, const float* gy, float* gx, dim3 grid, int threads, size_t lds, int win, bool q8,
                               hipStream_t st) {
  const VjClip clip{a.nv, a.sr_in};
  if (q8) {
    hipLaunchKernelGGL((resample_vjp_kernel<kVjResampleQ, true>), grid, dim3(threads), lds, st, gy, a.n_y, a.n_valid, gx, a.n_samp, a.up,
                       a.down, a.ht, a.t0, a.nt, a.t0min, win, clip);
  } else {
    hipLaunchKernelGGL((resample_vjp_kernel<1, true>), grid, dim3(threads), lds, st, gy, a.n_y, a.n_valid, gx, a.n_samp, a.up, a.down, a.ht,
                       a.t0, a.nt, a.t0min, win, clip);
  }
  LP_LAUNCH_CHECK();
  ++g_k1_vjp_launches[q8 ? K1V_RESAMPLE_Q8_RAGGED : K1V_RESAMPLE_Q1_RAGGED];
  return LIPASR_OK;
}

}  // namespace lipasr
