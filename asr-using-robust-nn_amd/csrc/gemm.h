// The dense classifier's GEMM interface: what a launch is told (GemmArgs, its epilogues and dropout arguments), the grouped
// launch's argument block, and the host entry points of gemm.hip that the plan (mlp_train.hip, mlp_infer.hip) calls.  The choice of a kernel
// (pick_gemm) and the launchers live in gemm.hip; the tile kernels live in one translation unit per family (gemm_frag.hip,
// gemm_lds.hip, gemm_ring.hip, gemm_ring_group.hip, gemm_ring2.hip), each of which registers its instances in the GemmTable.
#pragma once
#include "mlp.h"

namespace lipasr {

enum Epi {
  EPI_STORE = 0,
  EPI_BIAS = 1,
  EPI_BIAS_RELU = 2,
  EPI_BIAS_RELU_BN = 3,
  EPI_DZ_INFER = 4,
  EPI_SIGNSTEP = 5,
  EPI_BIAS_RELU_STATS = 6,  // training forward: a = relu(acc + b) and per-tile column sums of a, a^2
  EPI_DH_STATS = 7,         // training backward: g = acc * dropout and per-tile column sums of g, g * xhat
  EPI_DZ_NOBN = 8,          // training backward through Dropout -> ReLU without BatchNorm
  EPI_BIAS_SOFTMAX_CE = 9,  // last layer (N <= 32, one column tile): logits, softmax, CE loss and (p - y) / B in one
  EPI_BIAS_RELU_BNX = 10,   // round 5, training forward: a = relu(acc + b), BatchNorm statistics exchanged between the row tiles of
                            // the column block inside the launch, h = dropout(BN(a)) -- no apply kernel
  EPI_DH_BNX = 11           // round 5, training backward: g = acc * dropout, sums of g, g xhat exchanged, dz = BN/ReLU backward
};

// ---------------------------------------------------------------------------------------------
// dropout multiplier: 0 or 1/(1-rate), Philox keyed by (seed; element/4, layer, step)
// ---------------------------------------------------------------------------------------------
struct DropArgs {
  int mode;  // 0 off, 1 philox, 2 external
  float rate;
  uint64_t seed;
  const int* step_dev;
  int layer;
  const float* mask;
};

__device__ __forceinline__ float dropout_mult(const DropArgs& d, int step, size_t e) {
  if (d.mode == 0 || d.rate <= 0.0f) return 1.0f;
  if (d.mode == 2) return d.mask ? d.mask[e] : 1.0f;
  uint32_t o[4];
  Philox::gen(d.seed, (uint64_t)(e >> 2), (uint32_t)d.layer, (uint32_t)step, o);
  const float u = Philox::u01(o[e & 3]);
  return u > d.rate ? 1.0f / (1.0f - d.rate) : 0.0f;
}

// The multipliers of the four consecutive elements (row, col .. col + 3) of a row-major [.][ld] tensor with N valid columns;
// columns >= N get 0 and are neither drawn nor read.  Every epilogue walks its rows in such groups, col % 4 == 0, and the four
// elements of a group whose first index is a multiple of 4 share their Philox counter (e >> 2) and take its four outputs in order:
// ONE generator call gives the same four masks as four calls of dropout_mult that keep one output each.  (The row base is
// row * ld with ld a run-time value, so the compiler could not see the four counters as equal: it emitted four generators and a
// select chain per group -- 344 vector instructions, 76 of them v_mad_u64_u32, against 110 and 19 now)  The test is written on ld and col,
// not on the index, so that it is wave-uniform; whatever fails it -- ld % 4 != 0, a ragged last group -- keeps the call per element.
__device__ __forceinline__ void dropout_mult4(const DropArgs& d, int step, int row, int ld, int col, int N, float (&m)[4]) {
  const size_t e0 = (size_t)row * ld + col;
  if (d.mode == 1 && d.rate > 0.0f && ((ld & 3) == 0) && ((col & 3) == 0) && col + 3 < N) {
    uint32_t o[4];
    Philox::gen(d.seed, (uint64_t)(e0 >> 2), (uint32_t)d.layer, (uint32_t)step, o);
    const float keep = 1.0f / (1.0f - d.rate);
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = Philox::u01(o[k]) > d.rate ? keep : 0.0f;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = (col + k < N) ? dropout_mult(d, step, e0 + k) : 0.0f;
}


struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  int M, N, K, lda, ldb, ldc;
  int epi;
  const float* bias;
  const float* gamma;
  const float* beta;
  const float* mmean;
  const float* mvar;
  float* aux;        // EPI_BIAS_RELU_BN: optional post-ReLU store; EPI_DZ_INFER: post-ReLU activations (read)
  const float* x0;   // EPI_SIGNSTEP
  float* x_adv;
  float alpha, eps;
  float* part;             // *_STATS: [2][gridDim.y][N] per-row-tile column partial sums
  const float* save_mean;  // EPI_DH_STATS: batch mean [N], rstd at +N
  DropArgs drop;           // EPI_DH_STATS / EPI_DZ_NOBN
  int ones_row;            // AMODE 1 only: row M-1 of op(A) is all ones (bias gradient = column sums of B)
  float* extra_out;        // its output row goes here instead of C
  // EPI_BIAS_SOFTMAX_CE (softmax_ce_kernel's softmax and first argmax, and the cross-entropy, fused): labels in, the rest optional outputs
  const float* y;          // [M][N] one-hot
  float inv_batch;
  float* prob;             // [M][N]
  float* dz;               // [M][N] (p - y) * inv_batch
  float* loss_rows;        // [M]
  float* correct_rows;     // [M]
  // 0: exact fp32 (v_mfma_f32_32x32x2_f32).  1: operands rounded to bf16 (RNE) at the MFMA, fp32 accumulate
  // (v_mfma_f32_32x32x16_bf16): BASELINE config 2's arithmetic; memory stays fp32.
  int bf16;
  const unsigned* sa_dyn;  // arithmetic mode 2: the operand's largest magnitude (float bits, written by its producer's epilogue): the
  const unsigned* sb_dyn;  // scale is derived from it at run time (gradients: their size is not known beforehand); else sa / sb
  unsigned* amax_out;      // EPI_DH_BNX: max |dz| of this launch is folded into this word (atomic max of float bits)
  unsigned* amax_zero;     // forward launches: workgroup (0, 0) clears this word (the backward pass of the same step fills it)
  float sa, sb;       // arithmetic mode 2: powers of two that bring op(A) and B into fp16's range before the split (the accumulator is divided by sa sb)
  int lds_min_tiles;  // host side only: 64x64 tiles from which launch_gemm takes the LDS-tiled kernel (0 = the default)
  const float* zeros; // >= 16 bytes of zeros in device memory (the ring kernel's source for k >= K in the last k-step), or null
  int cus;            // host side: CUs the launch may use (the plan's budget; 0 = unknown, the whole device)
  int ring;           // host side / grouped launch: this problem takes the LDS-DMA ring tile (mode 2, ring_legal)
  int xcd_map;        // 1: workgroup -> tile by xcd_tile() (a compact patch of the tile grid per XCD); 0: blockIdx as it comes
  // EPI_BIAS_RELU_BNX / EPI_DH_BNX (the exchange epilogue)
  unsigned long long* xc_gran;  // [32-column block][xc_rt_max][128] {tag, value}
  unsigned* xc_ctrl;            // [32-column block][32]: word 0 generation, word 1 arrivals
  int* xc_err;
  int xc_rt_max;
  int Bstat;                    // rows the statistics are taken over
  float grad_scale;             // EPI_DH_BNX: factor on dgamma / dbeta
  float* h_out;                 // EPI_BIAS_RELU_BNX: BatchNorm + dropout output (C receives the post-ReLU activations)
  float* mmean_w;               // EPI_BIAS_RELU_BNX: moving statistics (updated by row tile 0), saved batch mean | rstd
  float* mvar_w;
  float* save_w;
  float* dgamma;                // EPI_DH_BNX
  float* dbeta;
};

// ReLU and its backward mask that keep a NaN.  fmaxf returns its other argument and NaN > 0 is false, so a poisoned pre-activation
// (a NaN input, or inf - inf after an operand left fp16's range in arithmetic mode 2) became 0 in the forward pass and the step
// went on with a finite loss and finite gradients; Keras' ReLU passes the NaN on, and so does the oracle (a NaN activation times
// the mask (a > 0) is NaN).  The same bits as fmaxf(t, 0) and (a > 0 ? d : 0) for every other value.
__device__ __forceinline__ float relu_keep_nan(const float t) {
  const float a = fmaxf(t, 0.0f);
  return t != t ? t : a;
}
__device__ __forceinline__ float relu_mask_keep_nan(const float a, const float d) { return a > 0.0f ? d : (a != a ? a : 0.0f); }

// mode 2, operands whose size is not known beforehand (gradients): the producer's epilogue leaves max |x| as float bits; the
// scale 2^(14 - e) with max = f 2^e, f in [0.5, 1), puts the largest value in [2^13, 2^14) -- a factor 4 under fp16's 65504
// The maximum lives in kAmaxSlots words, one per 64-byte line: 2048 wavefronts folding their maxima into ONE word cost the backward
// kernels 10-22 us each (atomics execute at the memory side, one address serialises them); spread over 64 lines they run side by
// side, and a consumer reads the 64 words with one coalesced... strided load per wavefront and a wave maximum.
constexpr int kAmaxSlots = 64, kAmaxStride = 16;  // words
__device__ __forceinline__ float scale_from_amax(const unsigned* p, const float fallback) {
  if (!p) return fallback;
  const float a = wave_max(__uint_as_float(p[(threadIdx.x & 63) * kAmaxStride]));
  if (!(a > 0.0f) || !(a < INFINITY)) return 1.0f;  // all zero, or NaN / inf (which then propagate as they should)
  int e = 0;
  (void)frexpf(a, &e);
  return ldexpf(1.0f, 14 - e);
}
__device__ __forceinline__ void amax_publish(unsigned* out, float m) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) {
    const unsigned w = (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    atomicMax(out + (w & (kAmaxSlots - 1)) * kAmaxStride, __float_as_uint(m));  // (non-negative floats order like their bits; NaN is the largest)
  }
}
// workgroup (0, 0) of a forward launch clears the words the backward pass of the same step will fold into
__device__ __forceinline__ void amax_clear(unsigned* out) {
  if (threadIdx.x < kAmaxSlots) out[threadIdx.x * kAmaxStride] = 0u;
}

// Several independent GEMMs of one (AMODE, BMODE) in ONE launch: the six weight-gradient GEMMs of a training step
// (outputs from 880x1024 down to 64x10, all with K = batch) fill the chip together instead of running as six
// mostly latency-bound launches.  Block b belongs to the problem whose tile range contains it.
constexpr int kMaxGroup = 8;
struct GemmGroup {
  int n;
  int tile_start[kMaxGroup + 1];
  GemmArgs g[kMaxGroup];
};

// ---- host side (gemm.hip)
// lipasr_debug_gemm_mode(mode): A/B-timing and profiling knobs, never a different backend.  mode 0 (every field at its default
// below) is what ships; the bits are decoded in that one function and documented here.
struct GemmKnobs {
  int gemm_mode = 0;       // bits 0-1: 0 auto, 1 split-K kernel only, 2 LDS kernel wherever it is legal (profiling knob)
  bool split_dw0 = false;  // bit 2: the first layer's weight gradient as its own launch
  bool group_lds = true;   // bit 3 clears it: the grouped launch on 32x32 fragment tiles (round 2)
  int xcd_map = 0;         // bit 4 SETS it (round 5: measured, not kept): the XCD-aware blockIdx -> tile map of xcd_tile().
                           // Same box, interleaved: config 2 0.3177 with it against 0.3148 without, config 3 0.3653 against 0.3625; the counters
                           // (TCC hit 67 % on the weight-gradient launch either way) say the operand panels are not what misses.
  bool no_ring = false;    // bit 5: arithmetic mode 2 on the register-staged tiles only (no LDS-DMA ring)
  int ring_tile = 2;       // weight-gradient group: 2 = the 128 x 128 tile with the split pass, 1 = the 64 x 64 ring tile (bit 6),
                           // 3 = the 128 x 128 tile that splits per fragment (bit 7)
  bool ring2 = true;       // bit 8 clears it: no 128 x 64 exchange tiles
  bool ring_x1 = true;     // bit 9 clears it: no loader-wavefront instance for exchange launches of one workgroup per CU
};
const GemmKnobs& gemm_knobs();

enum GemmKind { GK_FRAG4 = 0, GK_FRAG16, GK_LDS, GK_RING, GK_RING_X1, GK_RING2, GK_KINDS };

// what pick_gemm chose: the instance, one workgroup's output tile (grid = ceil(N / tile_n) x ceil(M / tile_m)), the launch shape
struct GemmPick {
  int kind;  // GemmKind
  int tile_m, tile_n, threads;
  size_t lds_bytes;
  const void* fn;
};

// Every instantiated GEMM kernel, indexed by what the templates are parameterised on; null = not instantiated.  A family's
// translation unit takes the addresses of the kernels it instantiates and reports their launch shapes beside them (the threads
// and LDS bytes are the constants its __launch_bounds__ and LDS carving are written with: the host side restates none of them).
struct GemmShape {
  int tile_m, tile_n, threads;
  size_t lds_bytes;
};
struct GemmTable;
// (internal to the library: not among its dynamic symbols)
__attribute__((visibility("hidden"))) void register_gemm_frag(GemmTable& t);        // gemm_frag.hip: GK_FRAG4, GK_FRAG16, grouped_frag
__attribute__((visibility("hidden"))) void register_gemm_lds(GemmTable& t);         // gemm_lds.hip: GK_LDS, grouped_lds
__attribute__((visibility("hidden"))) void register_gemm_ring(GemmTable& t);        // gemm_ring.hip: GK_RING, GK_RING_X1
__attribute__((visibility("hidden"))) void register_gemm_ring_group(GemmTable& t);  // gemm_ring_group.hip: grouped_ring
__attribute__((visibility("hidden"))) void register_gemm_ring2(GemmTable& t);       // gemm_ring2.hip: GK_RING2
struct GemmTable {
  const void* fn[GK_KINDS][2][2][2][3] = {};  // [kind][exchange epilogue][AMODE][BMODE][arithmetic]
  GemmShape shape[GK_KINDS] = {};
  const void* grouped_frag[3] = {}, *grouped_lds[3] = {}, *grouped_ring = nullptr;  // weight-gradient groups (AMODE 1, BMODE 1)
  GemmShape grouped_frag_shape = {}, grouped_lds_shape = {};
  GemmShape grouped_ring_shape[4] = {};  // by the launch's ring tile (GemmArgs::ring: 1, 2 or 3; ring 0 is no ring tile, [0] stays empty)
  // Built once, by gemm.hip's gemm_table(); nothing else constructs one.  The body sits here, and not in gemm.hip, so that the
  // constructor stays the inline (weak) function it was and the library's dynamic symbol list does not change.
  GemmTable() {
    register_gemm_frag(*this);
    register_gemm_lds(*this);
    register_gemm_ring(*this);
    register_gemm_ring_group(*this);
    register_gemm_ring2(*this);
  }
};

// amode / bmode: 1 = the operand is k-major in memory (P[k ld + i])
int pick_gemm(int amode, int bmode, const GemmArgs& g, GemmPick* out);  // the choice only: launches nothing, counts nothing
int launch_gemm(int amode, int bmode, const GemmArgs& g, hipStream_t st);
int launch_gemm_group_tn(const GemmArgs* gs, int n, hipStream_t st);  // up to kMaxGroup weight-gradient style GEMMs (AMODE 1, BMODE 1) per grid
GemmArgs gemm_args(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, int epi);
// row tiles of a launch = the leading extent of the *_STATS epilogues' column partials
int gemm_row_tiles(int amode, int bmode, const GemmArgs& g);
// may the (M, N, K) GEMM of a plan take the exchange epilogue (EPI_*_BNX)?  bmode 1: forward, 0: input gradient
bool exchange_fits(int bmode, int arith, int M, int N, int K, int lds_min_tiles, int xc_rt_max, int cus);

}  // namespace lipasr
