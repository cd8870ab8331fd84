// The dense-classifier plan, shared by mlp.hip (the plan itself), mlp_train.hip (the training step), mlp_infer.hip (predict, attacks,
// class gradients), optim.hip (Adam, projections) and bounds.hip, and what the three mlp units share among themselves.
#pragma once
#include "common.h"

namespace lipasr {

struct MlpLayer {
  int n_in = 0, n_out = 0;
  bool bn = false, nonneg = false;
  float dropout = 0.f;
  // offsets in floats into the flat trainable buffer (params / grads / adam m, v)
  size_t offW = 0, offb = 0, offg = 0, offbe = 0;
  // offsets in floats into bnstate
  size_t offmm = 0, offmv = 0;
  // offsets in floats into the plan workspace
  size_t offA = 0;     // post-ReLU activations [max_batch][n_out]            (hidden layers)
  size_t offH = 0;     // post-BN/dropout activations = next layer's input     (== offA if neither)
  size_t offMean = 0;  // saved batch mean [n_out], rstd follows at offMean + n_out (BN layers)
  size_t offDz = 0;    // gradient at this layer's pre-activation [max_batch][n_out] (kept for the grouped dW launch)
};

constexpr float kBnMomentum = 0.99f;  // Keras BatchNormalization defaults (train_constraints.py:68)
constexpr float kBnEps = 1e-3f;

// Test hook (lipasr_debug_k2_launches): launches since load per kernel of the training step that is not a GEMM, counted on the
// host where the launch happens.  The ids are part of the ABI (include/lipasr.h): append, never renumber.
enum K2Kernel { K2_BN_FWD = 0, K2_DROPOUT_FWD, K2_BN_BWD, K2_PART_REDUCE, K2_SOFTMAX_CE, K2_SOFTMAX_VJP, K2_SOFTMAX_VJP_ONEHOT,
                K2_ADAM_NONNEG, K2_STEP_INC, K2_KERNELS };
extern long g_k2_launches[K2_KERNELS];  // mlp.hip

// rows of the column partials [2][row tiles][width]: the *_STATS epilogues leave one slab per 32-row tile at the most
inline int part_row_tiles(int max_batch) { return (max_batch + 31) / 32; }

}  // namespace lipasr

struct lipasr_mlp {
  lipasr_ctx* ctx = nullptr;
  int n_layers = 0;
  int max_batch = 0;
  int max_width = 0;
  lipasr::MlpLayer L[LIPASR_MAX_LAYERS];
  size_t n_params = 0, n_state = 0;
  float* ws = nullptr;  // workspace
  size_t ws_floats = 0;
  size_t offLogits = 0, offProb = 0, offDzLast = 0, offG0 = 0, offG1 = 0, offPart = 0;
  int compute_bf16 = 0;  // lipasr_mlp_set_compute: 0 exact fp32, 1 GEMM operands rounded to bf16 at the MFMA, 2 fp16 two-plane split (fp32 accumulate)
  float last_inv_batch = 1.0f;  // the loss-gradient bound of the last training forward (mode 2's gradient scale in lipasr_mlp_train_dw0)
  int lds_min_tiles = 0;  // lipasr_mlp_set_gemm_tiles: training GEMMs take the LDS-tiled kernel from this many 64x64 tiles (0 = default)
  // Round 5: training-mode BatchNorm inside the GEMM that produces its input (gemm.hip, "exchange epilogue").  The row tiles
  // of a 32- (or 64-) column block hand each other their column partial sums through memory INSIDE the launch, so the apply
  // kernels and their launch boundaries go.  Per BatchNorm layer and direction: granules {tag, value} and two control words
  // per 32-column block.
  int fuse_bn = 1;        // lipasr_mlp_set_fuse_bn: 0 = the launch chain (GEMM + apply kernel), the parity reference
  int cu_budget = 0;      // lipasr_mlp_set_cu_budget: CUs the stream this plan runs on may use (0 = all of the device)
  int n_cus = 0;
  int xc_rt_max = 0;      // row tiles the granule regions hold (<= 64)
  unsigned long long* xc_gran = nullptr;
  unsigned* xc_ctrl = nullptr;
  unsigned* amax = nullptr;  // device words [layer]: max |dz_layer| of the current step as float bits (arithmetic mode 2's gradient scales)
  int* xc_err = nullptr;  // device word: an exchange gave up (a workgroup of its column block never became resident)
  size_t xc_gran_off[2][LIPASR_MAX_LAYERS] = {};  // [forward | backward][layer], in granules
  size_t xc_ctrl_off[2][LIPASR_MAX_LAYERS] = {};  // in 32-bit words
};

// What mlp.hip defines for mlp_train.hip and mlp_infer.hip; it stays out of the library's exported symbols.
namespace lipasr {
struct GemmArgs;  // gemm.h
enum OperandKind { OP_ACT = 0, OP_WEIGHT = 1, OP_GRAD = 2 };
#pragma GCC visibility push(hidden)
int plan_cus(const lipasr_mlp* m);  // the CUs the plan's stream may use
// arithmetic mode, CU budget and the fp16 range scales of mode 2 by operand kind; g0: bound of the gradient at the logits
void set_arith(GemmArgs& g, const lipasr_mlp* m, int kind_a, int kind_b, float g0 = 1.0f, bool training = true);
// an entry point's prologue: "null plan", "batch outside [1, max_batch]" and, for a plan with BatchNorm state, "bnstate is null";
// check_batch: the first two, for the entry points that take no bnstate
int check_batch(const char* fn, const lipasr_mlp* m, int batch);
int check_call(const char* fn, const lipasr_mlp* m, int batch, const float* bnstate);
#pragma GCC visibility pop
}  // namespace lipasr
