/*
 * lipasr.h -- C ABI of liblipasr.so: the MI355X (gfx950) hot path of
 * fmazilu/ASR-using-robust-NN behind plain pointers and sizes.
 *
 * The reference has no FFI: its hot path sits behind Python duck-typed protocols
 * (Keras Callback / Constraint, ART estimator / attack, librosa calls).  Every
 * entry point below cites the reference interface (file:line, relative to
 * "/root/reference/Voice digit recogniton/") whose arithmetic it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * lipasr_version(): 770. ABI history: 300 (round 3) -> round 4 added lipasr_flag_signal / lipasr_flag_wait and
 * lipasr_debug_chain_head without a bump -> 500: lipasr_flag_wait reports and keeps waiting (see its comment), plus the
 * round-5 entry points marked "(round 5)" below (lipasr_gemm_f16x2, lipasr_mlp_set_fuse_bn / _set_cu_budget / _exchange_errors,
 * lipasr_debug_launch_count).  510: the Lp attack entry points lipasr_lp_step, lipasr_lp_ball_init, lipasr_mlp_attack_step_lp.
 * 520: the backward pass of the MFCC stage, lipasr_mfcc_plan_vjp and lipasr_mfcc_plan_resample_vjp.
 * 530: clips of different lengths in one launch for the backward pass and the split forward: lipasr_mfcc_plan_vjp_ragged,
 * lipasr_mfcc_plan_resample_ragged, lipasr_mfcc_plan_from_22k_ragged.
 * 540: test hooks of the GEMM selector: lipasr_debug_gemm (the stand-alone product in any arithmetic mode), lipasr_debug_gemm_launches
 * and lipasr_debug_group_launches (launch counters per kernel instance).
 * 550: the backward pass of the short-window MFCC plans (n_fft = win_length = 441, hop 220 of Speaker recognition):
 * lipasr_mfcc_plan_vjp_short.
 * 560: lipasr_mlp_adam_project_product_signal (the optimizer step that also raises a lipasr_flag_wait counter when it starts).
 * 570: the DolphinAttack chain (ultrasonic AM generator and microphone model): lipasr_dolphin_create / _destroy / _bandpass /
 * _generate / _record / _generate_recorded and the host-only lipasr_dolphin_table.
 * 580: the local Lipschitz read-out: lipasr_mlp_jacobian (every class gradient from one forward pass) and lipasr_jacobian_sigma
 * (spectral norm and singular vectors of a stack of class gradients, per sample).
 * 590: the psychoacoustic masking threshold and the imperceptible attack's loss: lipasr_psy_create / _destroy / _psd / _threshold /
 * _prepare / _loss_grad / _step and the host-only lipasr_psy_table.
 * 600: one DeepFool iteration for a batch, lipasr_deepfool_step.
 * 610: randomized smoothing: lipasr_smooth_expand (noisy copies of every row), lipasr_smooth_vote (argmax histogram per clip) and
 * the host-only lipasr_smooth_noise_host.
 * 620: the genetic black-box attack: lipasr_genetic_breed (one generation's children), lipasr_genetic_select (fitness, elite and
 * parent draws per clip) and the host-only lipasr_genetic_breed_host.
 * 630: test hook of the K3 projections: lipasr_debug_k3_launches (launch counters per kernel).
 * 640: test hooks of the MFCC forward pass: lipasr_debug_k1_launches (launch counters per kernel instance) and
 * lipasr_debug_mfcc_stage (the dB tile, the frame maxima or the resampled signal a plan's last forward call left behind).
 * 650: Auto-PGD: lipasr_apgd_loss (cross-entropy or DLR with its gradient at the logits), lipasr_apgd_step (one iteration with a
 * step size, best point and checkpoint decisions per row) and the host-only lipasr_debug_apgd_path.
 * 660: Square Attack: lipasr_square_init (the stripe start), lipasr_square_step (one query's bookkeeping and the next proposal) and
 * the host-only lipasr_square_init_host / lipasr_square_step_host.
 * 670: HopSkipJump: lipasr_hsj_expand (the perturbed copies), lipasr_hsj_accumulate (the two fp64 sums), lipasr_hsj_direction,
 * lipasr_hsj_search (one query of the start, the step-size halving or the bisection), their _host twins and lipasr_debug_hsj_path.
 * 680: the over-the-air channel: lipasr_room_apply (every clip through every room impulse response of a bank), lipasr_room_vjp (its
 * exact adjoint, summed over the rooms) and their _host twins.
 * 690: test hooks of the MFCC backward pass: lipasr_debug_k1_vjp_launches (launch counters per kernel instance),
 * lipasr_debug_mfcc_vjp_stage (Gmel or g_y that a plan's last backward call left behind) and lipasr_debug_mfcc_stage_put (a dB tile
 * or frame maxima of the caller's INTO the plan, for a backward call with flags bit 0).
 * 700: universal adversarial perturbations: lipasr_universal_shifts (a shift per row), lipasr_universal_apply (one noise vector on
 * every row), lipasr_universal_reduce (the gradient rows summed back onto the noise, in fp64 and in a fixed order),
 * lipasr_universal_step (the step and projection of the noise) and their _host twins.
 * 710: certified robustness by bound propagation (IBP and CROWN-IBP): lipasr_mlp_bounds, lipasr_mlp_bounds_workspace, their _host
 * twins and the test hook lipasr_debug_bounds_launches.
 * 720: the time-warp operator: lipasr_warp_apply (every clip resampled under K triples of shift, rate and gain),
 * lipasr_warp_param_vjp (the derivative with respect to the three parameters), their _host twins, the host-only
 * lipasr_warp_table_host and the test hook lipasr_debug_warp_launches.
 * 730: test hooks of the training step's own kernels: lipasr_debug_k2_launches (launch counters per kernel) and
 * lipasr_debug_mlp_stage (an activation, the saved statistics, a gradient, the logits or the probabilities that a classifier plan's
 * last call left behind).  The NonNeg clamp of lipasr_mlp_adam_nonneg keeps a NaN weight (it wrote 0 before).
 * 740: input-transformation defences over audio: lipasr_defence_apply (a chain of median, FIR and bit-depth stages in one launch),
 * lipasr_defence_vjp (the chain's vector-Jacobian product in one launch), their _host twins and the test hook
 * lipasr_debug_defence_launches.
 * 750: IBP certified training: lipasr_mlp_bounds_grad (the backward pass of the interval bounds with respect to the parameters),
 * lipasr_mlp_bounds_grad_workspace, their _host twins and the test hook lipasr_debug_bounds_grad_launches.
 * 760: CROWN-IBP certified training: lipasr_mlp_bounds_crown_grad (the backward pass of the relaxation with respect to the parameters),
 * lipasr_mlp_bounds_crown_grad_workspace, their _host twins and the test hook lipasr_debug_bounds_crown_grad_launches.
 * (lipasr_version(): 760 was the last library without the entry points below.)
 * 770: training for randomized smoothing: lipasr_mlp_train_fwd / lipasr_mlp_train_bwd (the training step with the loss gradient
 * supplied from outside), lipasr_smooth_loss (the Gaussian-noise / MACER loss over the noisy copies of every clip with its gradient at
 * the logits), the host-only lipasr_smooth_loss_host and lipasr_smooth_probit_host, and the test hook lipasr_debug_smooth_loss_launches.
 *
 * Conventions
 *   - every function returns int: 0 = LIPASR_OK, negative = LIPASR_E*; nothing
 *     throws across the ABI; lipasr_last_error() returns a thread-local message.
 *   - all array pointers are DEVICE pointers owned by the caller unless the
 *     parameter is documented "host".  The library allocates only per-handle /
 *     per-plan workspaces (tables, scratch) at create/plan time, never inside a
 *     launch function, so every launch function may be captured in a HIP graph.
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered; no
 *     launch function synchronises the device.
 *   - a handle / plan is re-entrant across handles, NOT thread-safe per handle:
 *     one handle per GPU per process (one process per GPU under data parallel).
 *     The K3 entry points (projections, norms, lipasr_sv_clip) share the handle's 4 MiB
 *     scratch: issue them on ONE stream per handle.  Classifier and MFCC plans own their
 *     workspaces, so different plans may run on different streams.
 *   - Dense kernels use the Keras layout W(in, out), y = x @ W, row-major.
 */
#ifndef LIPASR_H
#define LIPASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIPASR_OK            0
#define LIPASR_EINVAL       -1   /* bad argument (null pointer, size, unsupported shape) */
#define LIPASR_ENOMEM       -2   /* device allocation failed */
#define LIPASR_EHIP         -3   /* a HIP runtime call failed (message has hipGetErrorString) */
#define LIPASR_EUNSUPPORTED -4   /* valid request outside what the kernels implement */
#define LIPASR_ESTATE       -5   /* call order violated (e.g. mfcc before mfcc_plan) */

#define LIPASR_MAX_LAYERS   16
#define LIPASR_N_MFCC       20   /* librosa.feature.mfcc default n_mfcc */
#define LIPASR_N_MELS       128
#define LIPASR_N_FFT        2048
#define LIPASR_HOP          512
#define LIPASR_SR           22050 /* librosa.load default sr */

typedef struct lipasr_ctx* lipasr_handle_t;
typedef struct lipasr_mlp* lipasr_mlp_t;
typedef struct lipasr_mfcc* lipasr_mfcc_t;
typedef struct lipasr_dolphin* lipasr_dolphin_t;
typedef struct lipasr_psy* lipasr_psy_t;
typedef void* lipasr_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------ core */
int lipasr_version(void);
const char* lipasr_last_error(void);
/* device: HIP device ordinal.  Allocates the handle's scratch workspace. */
int lipasr_create(int device, lipasr_handle_t* out);
int lipasr_destroy(lipasr_handle_t h);

/* HIP-event timer on an explicit stream (bench.py times the stream the kernels run on). */
int lipasr_timer_create(lipasr_handle_t h, int* timer_id);
int lipasr_timer_start(lipasr_handle_t h, int timer_id, lipasr_stream_t stream);
int lipasr_timer_stop(lipasr_handle_t h, int timer_id, lipasr_stream_t stream);
/* synchronises on the stop event; host float out */
int lipasr_timer_elapsed_ms(lipasr_handle_t h, int timer_id, float* ms_host);

/* Device-side ordering between two streams: `flag` is an int in device memory (start at 0, raise monotonically).
 * lipasr_flag_signal stores `value` when the stream reaches it; lipasr_flag_wait holds its stream until *flag >= value (a
 * one-wavefront kernel that polls).  After timeout_ms it REPORTS (*err = 1) and keeps waiting: the ordering is never given up
 * because a peer was slow (round 4 let the stream go on there).  After 4 x timeout_ms it gives up (*err = 2) so that a signal
 * that can never come drains the queue instead of hanging it; a wait that finds *err == 2 when its own timeout passes leaves at
 * once.  `err` is an int the kernel writes with system scope: device memory, or pinned host memory the caller reads without
 * synchronising (what lipasr/pipeline.py does at the top of every step).  Cheaper on the waiting stream than hipEventRecord +
 * hipStreamWaitEvent.  The two streams must be able to run concurrently (e.g. disjoint CU masks, or spare wave slots: the
 * waiting wavefront holds one); under a tool that serialises kernels across streams (rocprofv3 --pmc) use events. */
int lipasr_flag_signal(lipasr_handle_t h, int* flag, int value, lipasr_stream_t stream);
int lipasr_flag_wait(lipasr_handle_t h, const int* flag, int value, int timeout_ms, int* err, lipasr_stream_t stream);

/* HIP-graph capture of any sequence of launch functions issued on `stream`. */
int lipasr_graph_begin(lipasr_handle_t h, lipasr_stream_t stream);
int lipasr_graph_end(lipasr_handle_t h, lipasr_stream_t stream, int* graph_id);
int lipasr_graph_launch(lipasr_handle_t h, int graph_id, lipasr_stream_t stream);
int lipasr_graph_destroy(lipasr_handle_t h, int graph_id);

/* A HIP stream restricted to the CUs whose bits are set in cu_mask (HOST array of n_words 32-bit words, bit i of
 * word w = CU 32 w + i; hipExtStreamCreateWithCUMask).  The end-to-end step runs the MFCC kernels and the
 * classifier's many short dependent kernels on two streams; confining the MFCC stream to part of the chip keeps the
 * rest free for the latency-bound chain (DESIGN.md, step level).  Destroy with lipasr_stream_destroy. */
int lipasr_stream_create_masked(lipasr_handle_t h, const uint32_t* cu_mask, int n_words, lipasr_stream_t* out);
int lipasr_stream_destroy(lipasr_handle_t h, lipasr_stream_t stream);

/* ------------------------------------------------------------------ K3: Lipschitz projections
 * Ws: HOST array of n_layers DEVICE pointers to Dense kernels W_l (rows[l] x cols[l], row-major,
 * rows = in, cols = out).  Scalars come back in DEVICE memory (no host sync). */

/* sigma_max(W) by power iteration on W^T W  -- replaces np.linalg.norm(w, ord=2) at
 * Constraints.py:24, extract_features_construct_dataset.py:158, train_constraints.py:58.
 * v_state: device [cols] warm-start vector (in/out); warm=0 starts from a fixed positive vector.
 * iters: number of (W v, W^T u) round trips before the final W v.  clamp_nonneg!=0 evaluates
 * max(W,0) (the matrix norm_constraint projects, Constraints.py:23). */
int lipasr_sigma_max(lipasr_handle_t h, const float* W, int rows, int cols, float* v_state, int warm,
                     int iters, int clamp_nonneg, float* sigma_out, lipasr_stream_t stream);

/* norm_constraint.on_batch_end (Constraints.py:27-33) with get_projection (:22-25) for every
 * layer: W <- max(W,0) * rho^(1/m) / (sigma_max(max(W,0)) + 2.22e-16), m = n_layers (:15-20).
 * v_state: device [sum(cols)] (layer l's vector at offset sum(cols[0..l-1])).
 * sigmas_out: device [n_layers], the pre-scaling sigma_max of each clamped kernel. */
int lipasr_project_per_layer(lipasr_handle_t h, float* const* Ws, const int* rows, const int* cols,
                             int n_layers, float rho, float* v_state, int warm, int iters,
                             float* sigmas_out, lipasr_stream_t stream);

/* simple_norm_constraint.on_batch_end (Constraints.py:171-189) with get_projection (:158-169):
 * visits order[0..n_order-1] (HOST array of layer indices, duplicates allowed; the caller builds
 * it from affected_layers_indices exactly as :173-189 iterates), each visited kernel
 * W <- W * (rho / (||W_m^T...W_1^T||_2 + 2.22e-16))^(1/m) with the product norm re-evaluated
 * after every visit.  The product norm is computed ONCE on the device (chain of skinny GEMMs +
 * Gram eigenvalue) and advanced in closed form, which is what the sequential re-evaluation
 * amounts to.  norms_out: device [n_order+1]: product norm before each visit
 * and after the last.  Requires cols[n_layers-1] <= 32 (the class dimension). */
int lipasr_project_product(lipasr_handle_t h, float* const* Ws, const int* rows, const int* cols,
                           int n_layers, float rho, const int* order, int n_order,
                           float* norms_out, lipasr_stream_t stream);

/* ||W_m^T ... W_1^T||_2 -- get_lipschitz_constrained's numerator
 * (extract_features_construct_dataset.py:188-194). sigma_out: device [1]. */
int lipasr_product_norm(lipasr_handle_t h, const float* const* Ws, const int* rows, const int* cols,
                        int n_layers, float* sigma_out, lipasr_stream_t stream);

/* customConstraint.__call__ (Constraints.py:43-46): W <- max(W,0) * rho / (||max(W,0)||_F + eps).
 * tf.norm(w, ord=2) with axis=None is the Frobenius norm. */
int lipasr_frobenius_project(lipasr_handle_t h, float* W, size_t n, float rho, lipasr_stream_t stream);

/* max_j sqrt(var_j)/gamma_j -- one BatchNorm's correction factor
 * (extract_features_construct_dataset.py:181-184). out: device [1]. */
int lipasr_bn_correction(lipasr_handle_t h, const float* gamma, const float* var, int n, float* out,
                         lipasr_stream_t stream);

/* norm_constraint_FISTA's singular-value steps (Constraints.py:78-79 `svd(T)` for the constraint
 * read-out, :86-88 `svd(Yt / gam, full_matrices=False); clip(s1, 0, rho); dot(u1 * s1, v1)`):
 * X is device [R][n] row-major with R <= 32 (the class dimension).  out (device [R][n], may alias
 * X, may be NULL) receives U min(S, hi) V^T; svals_out (device [R], may be NULL) the singular
 * values in descending order.  Thin SVD through the fp64 Gram matrix X X^T (Jacobi). */
int lipasr_sv_clip(lipasr_handle_t h, const float* X, int R, int n, float hi, float* out, float* svals_out,
                   lipasr_stream_t stream);

/* ------------------------------------------------------------------ K4: sign step
 * ART FastGradientMethod / ProjectedGradientDescent update (attacks.py:506-510, 657-661),
 * norm=inf, no clip_values: x_adv <- x0 + clip(x_adv + alpha*sign(g) - x0, -eps, +eps), in place.
 * NaN gradients count as 0.  eps = +inf gives the plain FGSM step. */
int lipasr_sign_step(lipasr_handle_t h, float* x_adv, const float* x0, const float* g, size_t n,
                     float alpha, float eps, lipasr_stream_t stream);

/* ------------------------------------------------------------------ K4 in any norm (ART FastGradientMethod / ProjectedGradientDescent,
 * norm=1, 2 or inf).  `norm` is 1.0f, 2.0f or +INFINITY; anything else returns LIPASR_EINVAL.  tol = 1e-7 (ART's 10e-8).
 * lipasr_lp_step: one step plus projection, in place on x_adv [rows][n] (any n), per row:
 *   g   <- g with NaN entries set to 0
 *   d   <- sign(g) (inf) | g / (sum|g| + tol) (1) | g / (||g||_2 + tol) (2)
 *   x'  <- x_adv + alpha d             (a negative alpha descends: the targeted attack, ART's (1 - 2 targeted) factor)
 *   x_adv <- x0 + clip(x' - x0, -eps, eps) (inf) | x0 + (x' - x0) min(1, eps / (||x' - x0||_p + tol)) (1, 2);  eps = +inf: x'
 * Under norm 1 and 2 a row whose gradient norm is not finite (a +-inf entry) takes no step and is only projected; under norm
 * inf a +-inf entry steps by its sign (as lipasr_sign_step does).  One wavefront per row, reductions in a fixed order:
 * bit-identical on every run; norm inf gives lipasr_sign_step's bits. */
int lipasr_lp_step(lipasr_handle_t h, float* x_adv, const float* x0, const float* g, int rows, int n, float norm, float alpha,
                   float eps, lipasr_stream_t stream);
/* ART's random start (random_sphere(rows, n, eps, norm), the num_random_init of FGM / PGD): x_adv <- x0 + delta, delta
 * uniform on [-eps, eps]^n (inf), uniform in the L2 ball (2: eps U^(1/n) a / |a|, a Gaussian -- the law of ART's gammainc
 * form), or ART's L1 draw (1: radius eps sqrt(U), split as r E_i / sum E_j with exponential E_i and random signs -- the gaps
 * of sorted uniforms, not uniform in the L1 ball).  Philox keyed like the dropout masks: key seed + rank x golden ratio,
 * counter (element group, row, *counter_dev) -- counter_dev is a device int (NULL counts as 0) read by the kernel, so a
 * replayed graph draws afresh whenever the caller's counter moves, and equal (seed, *counter_dev, rank) give equal bits.
 * eps finite and >= 0. */
int lipasr_lp_ball_init(lipasr_handle_t h, float* x_adv, const float* x0, int rows, int n, float norm, float eps, uint64_t seed,
                        const int* counter_dev, int rank, lipasr_stream_t stream);

/* ------------------------------------------------------------------ A2: StandardScaler
 * sklearn StandardScaler().fit_transform (train_constraints.py:28-31, attacks.py:61-63):
 * per-feature mean and population std over N rows (accumulated in fp64), scale 1 for constant
 * features.  mean_out/scale_out: device double [F]. */
int lipasr_scaler_fit(lipasr_handle_t h, const float* x, int n_rows, int n_feat, double* mean_out,
                      double* scale_out, lipasr_stream_t stream);
int lipasr_scaler_apply(lipasr_handle_t h, const float* x, int n_rows, int n_feat, const double* mean,
                        const double* scale, float* out, lipasr_stream_t stream);

/* ------------------------------------------------------------------ K2: fp32 MFMA GEMM (exact fp32 fma chains)
 * C[M,N] = op(A)[M,K] * op(B)[K,N]; transA=0: A is [M][lda]; transA=1: A is [K][lda] (A^T stored);
 * transB=0: B is [K][ldb]; transB=1: B is [N][ldb]. */
int lipasr_gemm_f32(lipasr_handle_t h, int transA, int transB, int M, int N, int K, const float* A,
                    int lda, const float* B, int ldb, float* C, int ldc, lipasr_stream_t stream);

/* (round 5) The same product in the classifier's third arithmetic mode (lipasr_mlp_set_compute(plan, 2)): every operand value,
 * multiplied by scale_a / scale_b (powers of two that bring it inside fp16's range: |x scale| <= 65504, and best >= 2^-3),
 * is split into two fp16 planes and three of the four cross terms run on v_mfma_f32_32x32x16_f16 with fp32 accumulation:
 * 2^-21 per product where the exact mode's fma chain has 2^-24, at a quarter of the matrix time.  Large well-aligned problems
 * (K a multiple of 32, leading dimensions multiples of 4, 16-byte aligned bases) take the LDS-DMA ring kernel. */
int lipasr_gemm_f16x2(lipasr_handle_t h, int transA, int transB, int M, int N, int K, const float* A, int lda,
                      const float* B, int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream);

/* ------------------------------------------------------------------ K2/K5: the dense classifier plan
 * get_model() of train_constraints.py:63-88 / train_google_dataset.py:49-74 as data:
 * n_layers Dense layers, widths[0..n_layers]; hidden layers are Dense(relu) [-> BatchNorm]
 * [-> Dropout(rate)], the last is Dense(softmax).  bn/dropout entries for the last layer are
 * ignored.  nonneg[l] != 0 puts Keras NonNeg on kernel l.
 *
 * Flat buffers (caller-owned, fp32):
 *   params / grads / adam_m / adam_v : n_params floats, per layer [W | b | gamma | beta], every
 *       segment start aligned to 4 floats (pad floats are zero and stay zero).  `grads` is the
 *       data-parallel all-reduce buffer.
 *   bnstate : n_state floats, per BN layer [moving_mean | moving_var].
 */
#define LIPASR_SEG_W      0
#define LIPASR_SEG_B      1
#define LIPASR_SEG_GAMMA  2
#define LIPASR_SEG_BETA   3
#define LIPASR_SEG_MMEAN  4  /* in bnstate */
#define LIPASR_SEG_MVAR   5  /* in bnstate */

int lipasr_mlp_create(lipasr_handle_t h, int n_layers, const int* widths, const int* bn,
                      const float* dropout, const int* nonneg, int max_batch, lipasr_mlp_t* out);
int lipasr_mlp_destroy(lipasr_mlp_t m);
int lipasr_mlp_sizes(lipasr_mlp_t m, size_t* n_params, size_t* n_state);
/* offset (in floats) and element count of one segment; count 0 if the layer has no such segment */
int lipasr_mlp_segment(lipasr_mlp_t m, int layer, int kind, size_t* offset, size_t* count);

/* dropout_mode: 0 = off, 1 = Philox mask from (seed, *step_dev, layer, element), 2 = masks given:
 * dropout_masks is a HOST array of n_layers DEVICE pointers (or NULL entries) to [batch][width]
 * multipliers (0 or 1/(1-rate)). */
typedef struct lipasr_dropout_cfg {
  int mode;
  uint64_t seed;
  const int* step_dev;              /* device int, may be NULL (counts as 0) */
  const float* const* masks;        /* host array of device pointers, mode 2 */
} lipasr_dropout_cfg;

/* One training-mode forward + loss + backward: Keras train_step up to the optimizer
 * (train_constraints.py:94-105 with get_model :63-88): Dense/ReLU, BatchNorm with batch statistics
 * (momentum .99, eps 1e-3; moving stats updated in bnstate), inverted dropout, softmax +
 * categorical cross-entropy from logits, gradient (p - y) * inv_batch at the logits.
 * inv_batch = 1/global batch (data parallel: the all-reduce SUMS per-replica grads).
 * Outputs: grads (flat, overwritten), loss_rows [batch] (-sum y log p per row), correct_rows
 * [batch] (1.0 where argmax p == argmax y), probs [batch][classes] (may be NULL). */
int lipasr_mlp_train_fwd_bwd(lipasr_mlp_t m, const float* params, float* bnstate, const float* x,
                             const float* y_onehot, int batch, float inv_batch,
                             const lipasr_dropout_cfg* dropout, float* grads, float* loss_rows,
                             float* correct_rows, float* probs, lipasr_stream_t stream);

/* Data-parallel form of lipasr_mlp_train_fwd_bwd (no reference counterpart: train_constraints.py:91-105 is one
 * process): the same kernels in two calls, so that the gradient all-reduce of everything but the first layer's kernel
 * runs while that kernel's gradient -- 56 % of the bytes and the last thing a backward pass can start -- is still being
 * computed.  _head: forward, loss, the whole dX chain and every gradient except [dW_0 | db_0]; _dw0: those two.
 * lipasr_mlp_grad_split: the first `late_floats` floats of `grads` belong to _dw0, the rest is final after _head. */
int lipasr_mlp_train_fwd_bwd_head(lipasr_mlp_t m, const float* params, float* bnstate, const float* x,
                                  const float* y_onehot, int batch, float inv_batch,
                                  const lipasr_dropout_cfg* dropout, float* grads, float* loss_rows,
                                  float* correct_rows, float* probs, lipasr_stream_t stream);
int lipasr_mlp_train_dw0(lipasr_mlp_t m, const float* x, int batch, float* grads, lipasr_stream_t stream);
int lipasr_mlp_grad_split(lipasr_mlp_t m, size_t* late_floats);

/* The training step with the loss gradient supplied from outside (ours: Keras fuses softmax cross-entropy into train_step,
 * train_constraints.py:94-105; a loss over SEVERAL rows -- lipasr_smooth_loss over the noisy copies of a clip -- has a gradient at
 * the logits that is no (p - y) / B of one row).  The same kernels as lipasr_mlp_train_fwd_bwd in two calls, counted under the same
 * ids of lipasr_debug_gemm_launches / lipasr_debug_group_launches / lipasr_debug_k2_launches; no kernel of their own.
 *   _train_fwd: the forward pass of lipasr_mlp_train_fwd_bwd as it stands: training-mode BatchNorm (moving statistics in bnstate
 *     updated), dropout, every activation and saved statistic kept in the plan's workspace.  The last GEMM's epilogue runs without
 *     labels: it leaves the logits and the probabilities in the workspace (lipasr_debug_mlp_stage 5 and 6) and writes neither a loss
 *     nor a gradient; the plan's gradient slot at the logits (stage 3 of the last layer) keeps what the last plain step left there.
 *     logits_out [batch][classes] receives a copy of the logits (a device-to-device copy on `stream`, no kernel).  The logits, the
 *     probabilities, the activations, the saved statistics and bnstate equal bit for bit what lipasr_mlp_train_fwd_bwd leaves for the
 *     same inputs, in every arithmetic mode and with lipasr_mlp_set_fuse_bn 0 and 1.
 *   _train_bwd: the dX chain and the weight gradients of lipasr_mlp_train_fwd_bwd (the first layer's as the plain entry launches
 *     it), reading dz [batch][classes], the caller's gradient at the logits, where the plain step reads its own (p - y) * inv_batch.
 *     It relies on the workspace of the lipasr_mlp_train_fwd JUST BEFORE it on the same plan and stream, with the same x, params,
 *     batch and dropout -- as lipasr_mlp_train_dw0 relies on lipasr_mlp_train_fwd_bwd_head; nothing checks it.  grads is overwritten.
 *     dz_bound: the caller's promise max |dz| <= dz_bound (finite, > 0, else LIPASR_EINVAL).  It stands wherever the plain step uses
 *     inv_batch as the bound of the gradient at the logits: arithmetic mode 2 (the fp16 planes) derives the scale of dz from it, a
 *     dz beyond 256 dz_bound leaves fp16's range there and turns the gradients inf / NaN (loud); a later lipasr_mlp_train_dw0 reads
 *     it too.  Exact fp32 and bf16 ignore it.  dz given as (p - y) * inv_batch with dz_bound = inv_batch reproduces
 *     lipasr_mlp_train_fwd_bwd's grads bit for bit.
 * Refusals: those of lipasr_mlp_train_fwd_bwd (null plan or argument, batch outside [1, max_batch], bnstate null for a plan with
 * BatchNorm, dropout mode).  Not built: the synchronized-BatchNorm segments and the head / dw0 split of data parallelism. */
int lipasr_mlp_train_fwd(lipasr_mlp_t m, const float* params, float* bnstate, const float* x, int batch,
                         const lipasr_dropout_cfg* dropout, float* logits_out /* [batch][classes] */, lipasr_stream_t stream);
int lipasr_mlp_train_bwd(lipasr_mlp_t m, const float* params, const float* x, const float* dz /* [batch][classes] */, int batch,
                         float dz_bound, const lipasr_dropout_cfg* dropout, float* grads, lipasr_stream_t stream);

/* Synchronized BatchNorm under data parallelism (opt-in, for runs that must reproduce the single-device statistics of
 * train_constraints.py:68-83 exactly; the default is per-replica statistics): lipasr_mlp_train_fwd_bwd cut into
 * segments that end right after each GEMM whose epilogue leaves BatchNorm column partial sums -- sums of a and a^2 in the
 * forward pass, of g and g xhat in the backward pass -- i.e. before the kernel that consumes them.  The caller runs
 * segment 0 .. n-1 in order and, after segment s, SUM-all-reduces the first lipasr_mlp_train_segment_exchange(m, batch, s)
 * floats of `part` across the ranks (0 floats after the last).  part: caller-owned device buffer of
 * lipasr_mlp_part_floats(m) floats; stat_batch: rows of the GLOBAL batch (the statistics' denominator);
 * stat_grad_scale: 1 / world (dgamma / dbeta are computed from the already-global sums and are summed again by the
 * gradient all-reduce).  The reference model has 5 BatchNorm layers: 11 segments, 10 exchanges of <= 64 kB. */
int lipasr_mlp_train_segments(lipasr_mlp_t m, int* n_segments);
int lipasr_mlp_train_segment_exchange(lipasr_mlp_t m, int batch, int seg, size_t* floats);
int lipasr_mlp_part_floats(lipasr_mlp_t m, size_t* floats);
int lipasr_mlp_train_segment(lipasr_mlp_t m, int seg, const float* params, float* bnstate, const float* x,
                             const float* y_onehot, int batch, float inv_batch,
                             const lipasr_dropout_cfg* dropout, float* grads, float* loss_rows,
                             float* correct_rows, float* probs, float* part, int stat_batch,
                             float stat_grad_scale, lipasr_stream_t stream);

/* K5: Keras Adam (optimizer='adam', train_constraints.py:94) then NonNeg (:67-85) in one launch
 * over the flat buffers: g' = g*grad_scale; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 * w -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps); then w = w*[w>=0] on NonNeg kernels.
 * step_dev: device int holding the number of updates already applied; t = *step_dev + 1 and the
 * counter is incremented in-stream after the update. */
int lipasr_mlp_adam_nonneg(lipasr_mlp_t m, float* params, const float* grads, float* adam_m,
                           float* adam_v, int* step_dev, float lr, float beta1, float beta2, float eps,
                           float grad_scale, lipasr_stream_t stream);

/* Projections over the plan's kernels inside `params` (same semantics as the generic entry points). */
/* One optimizer step as train_constraints.py:94-105 runs it -- Adam, NonNeg, then the
 * simple_norm_constraint callback -- as ONE call: lipasr_mlp_adam_nonneg followed by
 * lipasr_mlp_project_product, with the step counter advanced inside the projection's own
 * single-workgroup kernel instead of a separate launch.  Same results as the two calls. */
int lipasr_mlp_adam_project_product(lipasr_mlp_t m, float* params, const float* grads, float* adam_m,
                                    float* adam_v, int* step_dev, float lr, float beta1, float beta2,
                                    float eps, float grad_scale, float rho, const int* order,
                                    int n_order, float* norms_out, lipasr_stream_t stream);
/* The same call, which also does what lipasr_flag_signal(flag, value) in front of it would do: the first thread of the Adam
 * kernel stores `value` to `flag` (release, device scope) when the kernel starts.  By then everything `stream` ran before --
 * a training step's forward and backward pass, i.e. every read of the step's input batch -- has finished, so a pipeline whose
 * other stream waits (lipasr_flag_wait) to refill that batch's buffer needs no one-wavefront signal launch at the end of the
 * step, on its critical stream.  flag == NULL: exactly lipasr_mlp_adam_project_product. */
int lipasr_mlp_adam_project_product_signal(lipasr_mlp_t m, float* params, const float* grads, float* adam_m,
                                           float* adam_v, int* step_dev, float lr, float beta1, float beta2,
                                           float eps, float grad_scale, float rho, const int* order,
                                           int n_order, float* norms_out, int* flag, int value,
                                           lipasr_stream_t stream);
int lipasr_mlp_project_product(lipasr_mlp_t m, float* params, float rho, const int* order, int n_order,
                               float* norms_out, lipasr_stream_t stream);
int lipasr_mlp_project_per_layer(lipasr_mlp_t m, float* params, float rho, float* v_state, int warm,
                                 int iters, float* sigmas_out, lipasr_stream_t stream);
int lipasr_mlp_product_norm(lipasr_mlp_t m, const float* params, float* sigma_out, lipasr_stream_t stream);

/* Arithmetic of the plan's GEMMs (forward, dX, dW; training and inference).  mode 0 (default): exact
 * fp32 on v_mfma_f32_32x32x2_f32 -- the parity path (logits within 1e-3 of the reference-precision
 * oracle).  mode 1: operands rounded to bf16 (round-to-nearest-even) at the matrix instruction,
 * fp32 accumulation, on v_mfma_f32_32x32x16_bf16 -- BASELINE config 2's "bf16"; parameters,
 * activations, statistics, the loss, Adam and the projections stay fp32.  Takes effect from the
 * next launch; re-capture HIP graphs after changing it. */
int lipasr_mlp_set_compute(lipasr_mlp_t m, int mode);  /* 0 exact fp32, 1 bf16 operands, 2 (round 5) fp16 two-plane split: see lipasr_gemm_f16x2 */

/* Kernel choice of the training pass's forward and dX GEMMs: from `lds_min_tiles` 64x64 output tiles on, the LDS-tiled
 * kernel instead of the 32x32 register-fragment one (0 = the built-in 224, about one tile per CU of a whole MI355X).  A
 * pipeline that confines the classifier to part of the chip lowers it (lipasr/pipeline.py: 128 on 160 CUs).  The two
 * kernels split K differently, so results agree to fp32 rounding, not bit for bit.  Takes effect from the next launch;
 * re-capture HIP graphs after changing it. */
int lipasr_mlp_set_gemm_tiles(lipasr_mlp_t m, int lds_min_tiles);

/* (round 5) Training-mode BatchNorm (train_constraints.py:68 ff.: BatchNormalization() after every hidden Dense) INSIDE the GEMM
 * that produces its input: the row tiles of a column block exchange their column partial sums through memory during the launch
 * (8-byte {tag, value} granules) and every tile normalises the values it still holds, forward and backward -- the ten
 * bn_apply_* launches of a step and their round trips go.  Bitwise reproducible (fixed summation order, no float atomics), equal
 * to the launch chain up to the order of the partial sums (1e-6).  mode 1 (default): wherever the launch's whole grid can be
 * resident on the CUs the plan may use and the batch has at most 64 row tiles; mode 0: the launch chain everywhere (the parity
 * reference).  Not used with synchronized BatchNorm (lipasr_mlp_train_segment).  The residency argument assumes that the plan's
 * stream has its CUs to itself while a launch runs (one process per GPU, the library's contract): two processes that run large
 * fused launches on ONE GPU at the same time can each hold slots the other waits for -- the exchanges then give up after 2 s and
 * report through lipasr_mlp_exchange_errors; such a set-up wants mode 0. */
int lipasr_mlp_set_fuse_bn(lipasr_mlp_t m, int mode);
/* (round 5) How many CUs the stream this plan is launched on may use (a CU-masked stream: lipasr_stream_create_masked);
 * 0 = all of the device (default).  The exchange above spins until its column block's workgroups have all published, so the
 * library must know how many can be resident: a plan run on a masked stream WITHOUT this call may stall (each exchange gives up
 * after 2 s and sets the error count below; it never hangs the queue). */
int lipasr_mlp_set_cu_budget(lipasr_mlp_t m, int n_cus);
/* (round 5) errors_host (HOST int): non-zero if an exchange gave up since the last call (then the results of that step are
 * not valid); synchronises with the device and clears the word. */
int lipasr_mlp_exchange_errors(lipasr_mlp_t m, int* errors_host);

/* model.predict (train_constraints.py:109, attacks.py:344): inference mode (BN moving statistics,
 * no dropout).  probs and/or logits [batch][classes], either may be NULL. */
int lipasr_mlp_predict(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x,
                       int batch, float* probs, float* logits, lipasr_stream_t stream);

/* ART TensorFlowV2Classifier.loss_gradient in inference mode: dx = d mean_b CE(f(x_b), y_b) / dx. */
int lipasr_mlp_input_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x,
                          const float* y_onehot, int batch, float* dx, lipasr_stream_t stream);

/* ART TensorFlowV2Classifier.class_gradient and the vector-Jacobian product the optimisation-based
 * attacks are built on (SaliencyMapMethod, CarliniL2Method, CarliniLInfMethod call sites at
 * attacks.py:538-645): dx[b] = sum_c v[b][c] * d out_c(x_b) / dx in inference mode, where out is the
 * model output -- the softmax probabilities (on_logits = 0; what ART differentiates for a Keras model
 * that ends in softmax) or the logits (on_logits = 1).  v: device [batch][classes] (a one-hot row gives
 * one class gradient).  probs_out (device [batch][classes], may be NULL) receives softmax(f(x)). */
int lipasr_mlp_output_vjp(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x,
                          const float* v, int on_logits, int batch, float* probs_out, float* dx,
                          lipasr_stream_t stream);

/* (ours: the reference has no such read-out)  The Jacobian of the model output in inference mode,
 *     J_b[c][k] = d out_c(x_b) / d x_b[k],   jac[b * stride_b + c * stride_c + k]   (strides in floats),
 * out = the logits (on_logits = 1) or the softmax probabilities (on_logits = 0), the two meanings lipasr_mlp_output_vjp has;
 * C = classes, 1 <= C <= 32 (more: LIPASR_EINVAL), n = the input width.  Row c carries what lipasr_mlp_output_vjp gives for the
 * one-hot vector e_c, from ONE forward pass instead of C: n_layers (1 + C) GEMM launches.  Both [batch][C][n] (stride_c >= n,
 * stride_b >= C stride_c) and class-major [C][batch][n] (stride_b >= n, stride_c >= batch stride_b) are accepted; other strides
 * are LIPASR_EINVAL.  probs_out (device [batch][classes], may be NULL) receives softmax(f(x)). */
int lipasr_mlp_jacobian(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x, int on_logits,
                        int batch, float* probs_out /* may be NULL */, float* jac, long stride_b, long stride_c,
                        lipasr_stream_t stream);

/* (ours)  The local Lipschitz constant: per sample b the spectral norm of the classes x n matrix J_b laid out as above (any
 * non-negative strides; 1 <= classes <= 32),
 *     sigma[b] = ||J_b||_2 (the largest singular value),  u[b][.] its left singular vector [classes],  v[b][.] the right one [n]:
 * v_b is the direction in input space along which the output moves fastest.  Conventions:
 *   - ||u|| = ||v|| = 1; the sign is fixed so that the component of u of largest magnitude is positive (lowest index on a tie);
 *   - J_b identically zero: sigma = 0, u = 0, v = 0; nothing is ever non-finite for finite input;
 *   - a NaN or inf anywhere in J_b: sigma[b] = NaN for that sample only (its u, v are written, with zeros);
 *   - when the two largest singular values coincide, u, v are some unit pair with J v = sigma u;
 *   - a column of J_b whose entries are all zero has v exactly 0 (a ragged clip's padding stays out of the direction);
 *   - J_b 2^k gives sigma 2^k and the same u, v (the kernel works on J_b scaled by a power of two, so that the ~1e-30
 *     Jacobians of a saturated softmax do not underflow when squared).
 * u and v may be NULL.  One launch, one workgroup per sample, no workspace, no atomics: two runs give the same bits.
 * batch == 0 or n == 0 return LIPASR_OK (n == 0: sigma and u are zeroed). */
int lipasr_jacobian_sigma(lipasr_handle_t h, const float* jac, int batch, int classes, int n, long stride_b, long stride_c,
                          float* sigma /* [batch] */, float* u /* [batch][classes] or NULL */,
                          float* v /* [batch][n] or NULL */, lipasr_stream_t stream);

/* (ours: the reference has no minimal-perturbation attack; the iteration is ART's art.attacks.evasion.DeepFool, restated from its
 * published implementation)  One DeepFool iteration for a batch, in place on x, in one launch.  jac: the class gradients J_b[c][k]
 * at jac[b * stride_b + c * stride_c + k] (any non-negative strides in floats: [batch][classes][n] or the class-major view, the
 * layouts lipasr_jacobian_sigma accepts); out: the logits or probabilities at x, whichever jac differentiates; label[b]: the class
 * the row started in; allowed[b]: bit k set = class k may be the target (NULL = every class).  Per row b, with c = label[b]:
 *   - any out[b][.] NaN or inf, or label[b] outside [0, classes): state -1, x[b] untouched, dist = NaN, target = -1;
 *   - argmax out[b] (lowest index on a tie) != c, the row has left its class: state 0, x[b] untouched bit for bit, dist = 0,
 *     target = that argmax;
 *   - otherwise, for every k != c with bit k of allowed[b] set:  w_k = J_k - J_c,  f_k = out_k - out_c,
 *         rho_k = |f_k| / (||w_k||_q + tol),   q = 2 for norm 2, q = 1 for norm inf,   tol = 1e-7 (ART's 10e-8),
 *     l = argmin rho_k, lowest index on a tie.  A class whose ||w_k|| is NaN or inf (a NaN or inf in J_k or J_c) is never chosen;
 *     when no class is left (classes == 1, an empty mask, a NaN in row c): state -1, x[b] untouched, dist = NaN, target = -1;
 *   - the step:  norm 2:  r = |f_l| / (||w_l||_2^2 + tol) w_l;   norm inf:  r = |f_l| / (||w_l||_1 + tol) sign(w_l), sign(0) = 0;
 *         x[b] <- clamp(x[b] + (1 + overshoot) r, clip_lo, clip_hi)     (-INFINITY / +INFINITY = no clipping),
 *     dist[b] = rho_l (the distance to the linearised boundary, before the overshoot), target[b] = l, state[b] = 1.
 *     A column where w_l is exactly 0 keeps the bits of x before clipping: a ragged clip's padding never moves.
 * overshoot = 0 is ART's iteration; the paper's is 0.02.  norm: 2.0f or +INFINITY, anything else LIPASR_EINVAL; 1 <= classes <= 32,
 * more is LIPASR_EINVAL; overshoot >= 0 and clip_lo <= clip_hi or LIPASR_EINVAL.  The differences w, their squares (or magnitudes)
 * and the sums are fp64, lane-serial then a fixed-order tree: ||w_k|| is right to 1e-6 relative for any finite fp32 J (a ~1e-30
 * Jacobian of a saturated softmax included), and two runs give the same bits.  dist is rounded to fp32 (+inf above its range).
 * One workgroup per row, no workspace, no atomics, nothing waits on another workgroup.  dist, target and state may be NULL.
 * batch == 0 returns LIPASR_OK; n == 0 too, with dist (= |f_l| / tol), target and state filled. */
int lipasr_deepfool_step(lipasr_handle_t h, const float* jac, long stride_b, long stride_c, const float* out /* [batch][classes] */,
                         const int* label /* [batch] */, const uint32_t* allowed /* [batch] or NULL */, int batch, int classes,
                         int n, float norm, float overshoot, float clip_lo, float clip_hi, float* x /* [batch][n] */,
                         float* dist /* [batch] or NULL */, int* target /* [batch] or NULL */, int* state /* [batch] or NULL */,
                         lipasr_stream_t stream);

/* (ours: the reference sweeps add_white_noise over sigmas, attacks.py:73-86, 335-339; CERTIFY and PREDICT of Cohen, Rosenfeld,
 * Kolter 2019 turn the same draws into a guarantee per clip)  The noisy copies of randomized smoothing, written once, in one launch.
 * Row b * draws + j of out, element k, with nv = min(max(n_valid[b], 0), n) (n_valid NULL: nv = n):
 *   - k < nv:   out = clamp(fmaf(sigma, z, x[b][k]), clip_lo, clip_hi)   (-INFINITY / +INFINITY = no clipping),
 *               z = normal4(seed, k >> 2, clip0 + b, draw0 + j)[k & 3]: the Philox4x32-10 block with key seed and counter
 *               (k >> 2 low, k >> 2 high = 0, clip0 + b, draw0 + j), Box-Muller on its two pairs;
 *   - k >= nv:  the bits of x[b][k], untouched and unclamped: a ragged clip's padding never moves.
 * The draw is a pure function of (seed, clip index, draw index, element): it depends on neither batch nor draws nor on where a
 * chunk starts, so chunks of any size reproduce one big call bit for bit.  clip0 = 0, draw0 = 0, draws = 1 are the counters of
 * lipasr_add_noise_f32 mode 0: one draw is the reference's white-noise attack (to the rounding of one fused multiply-add).
 * sigma = 0 returns x in value.  A NaN in x stays a NaN.  x and out must not overlap.
 * sigma < 0 or non-finite, clip_lo > clip_hi, a negative size, or more than 2^31 - 1 output rows: LIPASR_EINVAL; batch, draws or
 * n equal to 0: LIPASR_OK with nothing written; null pointers are refused before the device is touched.
 * Any n, any alignment of x and out (float4 where a row starts on 16 bytes, scalars otherwise; the values do not depend on it).
 * One workgroup per output row, no workspace, no atomics: two runs give the same bits. */
int lipasr_smooth_expand(lipasr_handle_t h, const float* x /* [batch][n] */, const int* n_valid /* [batch] or NULL */, int batch,
                         int n, int draws, uint32_t clip0, uint32_t draw0, float sigma, uint64_t seed, float clip_lo, float clip_hi,
                         float* out /* [batch * draws][n] */, lipasr_stream_t stream);

/* The votes of randomized smoothing: per clip b, the histogram of the argmax over rows b * draws .. b * draws + draws - 1 of logits
 * [batch * draws][classes], ADDED to counts[b][0 .. classes] (int32, [batch][classes + 1]): the caller zeroes counts, and calls
 * accumulate across chunks.  Per row: the largest entry wins, the lowest index on a tie, +inf is a maximum like any other (a row of
 * -inf votes for class 0); a row with any NaN goes to bin `classes` and to no class.  One launch, one workgroup per clip, which
 * alone touches counts[b][.]; per-wave counts by ballot and popcount, summed through LDS in a fixed order; no global atomics: two
 * runs give the same bits.  1 <= classes <= 32, otherwise LIPASR_EINVAL; batch == 0 or draws == 0 return LIPASR_OK. */
int lipasr_smooth_vote(lipasr_handle_t h, const float* logits, int batch, int draws, int classes,
                       int* counts /* [batch][classes + 1] */, lipasr_stream_t stream);

/* Host-only (no GPU needed): z_out[k] = normal4(seed, k >> 2, clip, draw)[k & 3] for k = 0 .. n - 1, the draws lipasr_smooth_expand
 * adds to clip `clip`, draw `draw` (the host's logf / sinf / cosf: equal to the device's to a few units in the last place). */
int lipasr_smooth_noise_host(uint64_t seed, uint32_t clip, uint32_t draw, int n, float* z_out /* host [n] */);

/* (ours: the reference measures accuracy under add_white_noise, attacks.py:73-86, 335-339, and trains on clean rows only)  The loss
 * of training FOR randomized smoothing over the noisy copies of every clip, with its gradient at the logits, in one launch:
 * Gaussian-noise training of the smoothed classifier (lam = 0) and MACER (Zhai et al., ICLR 2020; lam > 0).  Rows b * draws ..
 * b * draws + draws - 1 of logits are the copies of clip b (lipasr_smooth_expand's layout).  Everything is computed in fp64 from the
 * fp32 logits and rounded once to fp32 on store.  Per clip, y = label[b], m = draws, j a copy, c a class:
 *   p_j = softmax(z_j), s_j = softmax(beta z_j) (both max-subtracted);  p^ = mean_j p_j,  q = mean_j s_j  (summed in the order of j)
 *   L_C = -log p^_y = log m - logsumexp_j (z_jy - logsumexp_c z_jc), finite for any finite logits;
 *         dL_C/dz_jc = -w_j (d_cy - p_jc),  w_j = exp(log p_jy - logsumexp_j log p_jy)
 *   A = argmax_c q_c,  B = argmax_{c != y} q_c (the lowest index on a tie),  xi = Phi^-1(q_y) - Phi^-1(q_B),
 *         Phi^-1(0) = -inf, Phi^-1(1) = +inf; classes == 1: there is no B, q_B counts as 0 and xi = +inf
 *   the robust term is ACTIVE iff lam > 0, classes > 1, A == y, 0 < q_B, q_y < 1 and xi <= gamma:
 *         L_R = (sigma / 2) (gamma - xi) if active, else 0
 *         dxi/dz_jc = (beta / m) [a_y s_jy (d_cy - s_jc) - a_B s_jB (d_cB - s_jc)],  a_c = sqrt(2 pi) exp(Phi^-1(q_c)^2 / 2)
 *   (d_cc - p_jc is taken as the sum of the OTHER classes' p_jk in the order of k, which does not cancel when p_jc is close to 1)
 *   loss[b] = L_C + lam L_R;  dz = scale (dL_C/dz - lam (sigma / 2) dxi/dz)  (the second term only where active);
 *   correct[b] = 1.0 where argmax_c p^_c == y (the lowest index on a tie), else 0.0;
 *   radius[b] = (sigma / 2) xi where A == y and sigma > 0 (+inf is possible), else 0: the soft radius MACER maximises.
 * lam = 0 and draws = 1: loss is the plain cross-entropy of the row and dz = scale (p - onehot(y)).
 * A NaN or inf in any logit of a clip, or a label outside [0, classes): NaN in loss[b] and in every dz row of that clip, correct 0,
 * radius 0; the other clips are untouched.
 * LIPASR_EINVAL, before the device is touched: classes outside 1..32, draws outside 1..64, a negative clips, sigma < 0, lam < 0,
 * gamma <= 0, beta <= 0, any of them or scale not finite; then a null handle; clips == 0 returns LIPASR_OK with nothing written;
 * then null logits, label, dz or loss.  correct and radius may be NULL.  logits and dz may be the same buffer.
 * Phi^-1 is Wichura's AS 241 (PPND16, 1e-16 relative) in fp64.  One launch, one workgroup of 64 threads per clip with the clip's
 * logits, both softmaxes and its gradient rows in LDS, a lane per copy for the rows and a lane per class for the means; sums in a
 * fixed order, no atomics, no workspace, nothing waits on another workgroup: two runs give the same bits.
 * _host: the same arithmetic text compiled for the host (host pointers, no handle, no stream): it differs from the device by the
 * last places of libm's exp / log / sqrt.  lipasr_smooth_probit_host: out[i] = Phi^-1(q[i]) as the kernel computes it (n >= 0).
 * lipasr_debug_smooth_loss_launches (test hook): launches since load of 0 the loss kernel, 1 lipasr_smooth_expand's kernel; -1 for
 * an unknown id. */
int lipasr_smooth_loss(lipasr_handle_t h, const float* logits /* [clips * draws][classes] */, const int* label /* [clips] */,
                       int clips, int draws, int classes, float sigma, float lam, float gamma, float beta, float scale,
                       float* dz /* [clips * draws][classes] */, float* loss /* [clips] */, float* correct /* [clips] or NULL */,
                       float* radius /* [clips] or NULL */, lipasr_stream_t stream);
int lipasr_smooth_loss_host(const float* logits, const int* label, int clips, int draws, int classes, float sigma, float lam,
                            float gamma, float beta, float scale, float* dz, float* loss, float* correct, float* radius);
int lipasr_smooth_probit_host(const double* q /* host [n] */, int n, double* out /* host [n] */);
int lipasr_debug_smooth_loss_launches(int id);

/* (ours: the reference's black-box side is three noise sweeps, attacks.py:73-86, 145-294, none of which looks at the model's answer;
 * this is the genetic algorithm of Alzantot, Balaji, Srivastava 2018, which needs scores only)  One generation's children, written
 * once, in one launch.  Row b * pop + p of pop_out is child p of clip b; gen(seed; lo, hi0, hi1) below is the Philox4x32-10 block
 * with key seed and counter (lo low word, lo high word, hi0, hi1).
 *   - parents (a, c) = parents[b][p], both indices into the clip's members in pop_in (an index outside [0, pop) is clamped into it);
 *     c < 0: the child is member a of pop_in, copied verbatim (no draw, no clamp): the elite, and clips that are finished.
 *     pop_in == NULL (then parents must be NULL too): both parents are x0[b] -- the initial population.
 *   - per quad q = k >> 2 one block o = gen(seed; q, clip0 + b, generation * 256 + p); word e serves element k = 4 q + e:
 *     bit 0 picks the parent (0: a, 1: c), and the element mutates iff (o[e] >> 8) < mutate_thresh -- the caller passes
 *     round(p_mut * 2^24), so the decision is integer-exact (0: never, 2^24: always; more is LIPASR_EINVAL);
 *   - a mutating element takes child = fmaf(step, v, picked), v = 2 u01(m[e]) - 1 in (-1, 1] (exact in fp32),
 *     m = gen(seed; q | 1 << 63, clip0 + b, generation * 256 + p), u01(w) = ((w >> 8) + 1) / 2^24;
 *   - then, for k < nv = min(max(n_valid[b], 0), n) (n_valid NULL: nv = n): clamp to [x0 - eps, x0 + eps] (the two bounds rounded
 *     to fp32), then to [clip_lo, clip_hi] (-INFINITY / +INFINITY: no clamp); k >= nv: the bits of x0[b][k], whatever the parents
 *     hold -- of a copied child as well.  A NaN stays a NaN.
 * The draws are a pure function of (seed, clip index, generation, member, element): chunks of any size at any clip0 reproduce one
 * big call bit for bit, and lipasr_genetic_breed_host gives the same bits on the host (one shared inline function, no libm but a
 * fused multiply-add).  Any n, any alignment of x0, pop_in and pop_out (float4 where a row starts on 16 bytes, scalars otherwise;
 * the values do not depend on it).  One workgroup per output row, no workspace, no atomics.
 * 2 <= pop <= 64, generation < 2^24, step and eps finite and >= 0, clip_lo <= clip_hi, batch * pop <= 2^31 - 1, pop_out overlapping
 * neither pop_in nor x0, or LIPASR_EINVAL; batch or n equal to 0: LIPASR_OK with nothing written; null pointers are refused before
 * the device is touched. */
int lipasr_genetic_breed(lipasr_handle_t h, const float* x0 /* [batch][n] */, const int* n_valid /* [batch] or NULL */,
                         const float* pop_in /* [batch][pop][n] or NULL */, const int* parents /* [batch][pop][2] or NULL */,
                         int batch, int pop, int n, uint32_t clip0, uint32_t generation, uint64_t seed, uint32_t mutate_thresh,
                         float step, float eps, float clip_lo, float clip_hi, float* pop_out /* [batch][pop][n] */,
                         lipasr_stream_t stream);

/* Host-only (no GPU needed): lipasr_genetic_breed on host arrays, the same inline function in a plain loop -- the CPU-side pin of the
 * counters above.  Same checks, same bits. */
int lipasr_genetic_breed_host(const float* x0, const int* n_valid, const float* pop_in, const int* parents, int batch, int pop, int n,
                              uint32_t clip0, uint32_t generation, uint64_t seed, uint32_t mutate_thresh, float step, float eps,
                              float clip_lo, float clip_hi, float* pop_out);

/* The selection of one generation: per clip b, from rows b * pop .. b * pop + pop - 1 of logits [batch * pop][classes] and the class
 * y = labels[b]:
 *   - fitness[b][p] = max_{c != y} z_c - z_y (targeted: z_y - max_{c != y} z_c), the difference taken in fp64 and rounded once;
 *     -inf for a row with any NaN, for a NaN difference (inf - inf), for a label outside [0, classes) and, untargeted, for
 *     classes = 1;
 *   - best[b] = the argmax of the fitness, the lowest index on a tie;
 *   - done[b] is sticky: a clip that arrives with done[b] != 0 keeps its best and its done; otherwise, where fitness[best] > 0,
 *     done[b] = generation + 1 -- with one select per generation, counted from 0, the number of populations evaluated up to and
 *     including the one that succeeded.  A clip that is done (on arrival or now) gets parents[p] = (p, -1) for every p, which
 *     freezes its population under lipasr_genetic_breed; so does a clip none of whose members has a fitness above -inf;
 *   - every other clip: w_p = expf((fit_p - max) / temperature) (the argument in fp64, 0 for fit_p = -inf), the inclusive sums of w in
 *     index order in fp64 by a wave scan of fixed order; child 0 gets (best, -1), the elite; child p >= 1 draws u_a, u_c =
 *     u01 of words 0 and 1 of gen(seed; p | 1 << 62, clip0 + b, generation * 256), and each parent is the first index whose
 *     inclusive sum is >= u * total (a member of weight 0 is never drawn).
 * One wavefront per clip, lane p owns member p; no global atomics, no other workgroup touches a clip's outputs: two runs give the
 * same bits.  1 <= classes <= 32, 2 <= pop <= 64, temperature finite and > 0, generation < 2^24, or LIPASR_EINVAL; batch == 0
 * returns LIPASR_OK. */
int lipasr_genetic_select(lipasr_handle_t h, const float* logits, const int* labels /* [batch] */, int batch, int pop, int classes,
                          int targeted, float temperature, uint32_t clip0, uint32_t generation, uint64_t seed,
                          float* fitness /* [batch][pop] */, int* best /* [batch] */, int* done /* [batch] */,
                          int* parents /* [batch][pop][2] */, lipasr_stream_t stream);

/* (ours: the reference's strongest first-order attack is fixed-step PGD on the cross-entropy; this is Auto-PGD of Croce & Hein 2020,
 * "Reliable evaluation of adversarial robustness with an ensemble of diverse parameter-free attacks", ART's
 * AutoProjectedGradientDescent)  The objective to MAXIMISE and its gradient at the logits, per row of logits [batch][classes], in one
 * launch; y = labels[b].  The arithmetic is fp64 on the fp32 logits, rounded once.
 *   - loss_type 0, cross-entropy.  Untargeted: f = logsumexp(z) - z_y, dz = softmax(z) - e_y.  Targeted (the label is the target):
 *     f = -(logsumexp(z) - z_t), dz = e_t - softmax(z).  (logsumexp as m + log1p(sum_{c != argmax} exp(z_c - m)) and the entry at the
 *     label as -+ sum_{c != y} softmax_c: neither cancels.)
 *   - loss_type 1, the Difference-of-Logits-Ratio, untargeted only, classes >= 3.  pi sorts z in descending order, the lowest index
 *     first on ties; o = argmax_{i != y} z_i (the lowest index on a tie).  D = z_pi1 - z_pi3 + 1e-12, N = z_y - z_o, f = -N / D;
 *     dz gets -1/D at y, +1/D at o, +N/D^2 added at pi1 and -N/D^2 added at pi3; the contributions add where indices coincide.
 *     With targeted != 0, or fewer than 3 classes: LIPASR_EINVAL.
 *   - hit[b] = 1 if argmax z (the lowest index on a tie) != y when untargeted, == t when targeted; else 0.
 *   - a NaN or +-inf anywhere in a row, or a label outside [0, classes): f = NaN, dz = 0 and hit = 0 for that row only; nothing is
 *     read out of bounds.
 * 1 <= classes <= 32, loss_type 0 or 1, or LIPASR_EINVAL; batch == 0 returns LIPASR_OK; null pointers are refused before the device
 * is touched.  One thread per row, every sum over the classes in index order: two runs give the same bits.  No atomics, no
 * workspace. */
int lipasr_apgd_loss(lipasr_handle_t h, const float* logits /* [batch][classes] */, const int* labels /* [batch] */, int batch,
                     int classes, int loss_type, int targeted, float* f /* [batch] */, float* dz /* [batch][classes] */,
                     int* hit /* [batch] */, lipasr_stream_t stream);

#define LIPASR_APGD_FIRST 1 /* flags bit 0: the first iteration of a run (the state is initialised, a = 1) */
#define LIPASR_APGD_LAST  2 /* flags bit 1: bookkeeping only, after the last forward pass */
/* One Auto-PGD iteration for every row, in place, in one launch.  Row arrays [rows][n], float32: x (in/out, the iterate x_k), x_prev
 * (in/out, the previous iterate), x0 (in, the clean row), g (in, the gradient of f at x; NaN entries count as 0), x_best and g_best
 * (in/out, the best point and its gradient), x_adv (in/out, the most recent iterate that hit).  Per row: f and hit at x (from
 * lipasr_apgd_loss), n_valid or NULL (as lipasr_genetic_breed takes it: nv = min(max(n_valid, 0), n), NULL: nv = n), and the state
 * eta, f_best, f_prev, f_best_ckpt (float32), improved, reduced_last, fooled, halvings (int32).  Scalars: norm (2.0f or +INFINITY,
 * anything else LIPASR_EINVAL), eps (finite, >= 0), eta0 (finite, >= 0), clip_lo <= clip_hi (-INFINITY / +INFINITY: none), momentum
 * and rho (in [0, 1]; the paper's are 0.75 and 0.75), flags (LIPASR_APGD_FIRST | LIPASR_APGD_LAST) and ckpt_len (0: this iteration
 * is no checkpoint; otherwise the number of iterations since the previous checkpoint; never together with FIRST).
 * Per row, in this order:
 *   1. Bookkeeping at x.  With FIRST: eta = eta0, f_best = f_prev = f_best_ckpt = f, improved = reduced_last = fooled = halvings = 0,
 *      x_best <- x, g_best <- g (the state arrays and x_prev are not read).  Otherwise: if f > f_prev then improved++; then
 *      f_prev = f; if f > f_best then f_best = f, x_best <- x, g_best <- g.  A NaN f compares false everywhere; at FIRST it is
 *      stored as -inf.  In both cases hit sets fooled = 1 (sticky) and x_adv <- x.
 *   2. LAST: stop here; nothing else is written.
 *   3. Checkpoint (ckpt_len > 0).  Condition 1: improved < rho * ckpt_len (the product in fp64).  Condition 2: reduced_last == 0 &&
 *      f_best_ckpt == f_best.  If either holds: eta /= 2 and halvings++, the step below starts from (x_best, g_best) with
 *      x_prev := x_best -- the paper's Algorithm 1 leaves the momentum term after a restart open; here it is zero on that step --
 *      and reduced_last = 1.  If neither holds: reduced_last = 0, and the step starts from (x, g).  In either case improved = 0 and
 *      f_best_ckpt = f_best.
 *   4. The step from (xc, gc, xp): d = sign(gc) (inf; sign(0) = 0) or gc / (||gc||_2 + 1e-7) (2; a non-finite norm gives d = 0, as
 *      lipasr_lp_step does);  z = P(xc + eta d);  x_new = P(xc + a (z - xc) + (1 - a)(xc - xp)), a = 1 on FIRST and momentum
 *      otherwise;  P(v): u = clamp(v, clip_lo, clip_hi), then x0 + clamp(u - x0, -eps, eps) (inf) or
 *      x0 + (u - x0) min(1, eps / (||u - x0||_2 + 1e-7)) (2).  With x0 inside the clip range the result is inside both the ball and
 *      the range.  Then x_prev <- xc and x <- x_new.  The element-wise arithmetic and the norms are fp64 on the fp32 inputs and
 *      x_new is rounded once, so P returns the bits of a point that already is x0 +- eps.
 *   5. Padding.  Columns k >= nv take no part in any norm, and in every array written (x, x_prev, and x_best, g_best, x_adv where
 *      step 1 copies) they hold the bits of x0[k]: a ragged clip's padding never moves.  A row with nv == 0 only does step 1.
 * Any n, any alignment: a thread owns the same elements whatever the alignment (float4 loads where n is a multiple of 4 and all
 * seven row arrays sit on 16 bytes, scalars otherwise), so the values do not depend on it.  One wavefront per row with the step's
 * four row arrays in registers up to n = 2 048, one workgroup per row with the row held once in registers up to n = 22 528 (the
 * three dependent norms through LDS), a re-reading form of the same arithmetic beyond; lipasr_debug_apgd_path names the instance.
 * Every reduction runs in a fixed order: two runs give the same bits.  No atomics, no workspace, nothing waits on another
 * workgroup.  rows == 0 or n == 0 return LIPASR_OK; null pointers (n_valid excepted) are refused before the device is touched; two
 * arrays that overlap, one of them written, are LIPASR_EINVAL. */
int lipasr_apgd_step(lipasr_handle_t h, float* x, float* x_prev, const float* x0, const float* g, float* x_best, float* g_best,
                     float* x_adv, const float* f /* [rows] */, const int* hit /* [rows] */, const int* n_valid /* [rows] or NULL */,
                     float* eta, float* f_best, float* f_prev, float* f_best_ckpt, int* improved, int* reduced_last, int* fooled,
                     int* halvings, int rows, int n, float norm, float eps, float eta0, float clip_lo, float clip_hi, float momentum,
                     float rho, int flags, int ckpt_len, lipasr_stream_t stream);
/* Host-only (no GPU needed): the instance lipasr_apgd_step takes for rows of n floats.  Bits 0-2: 0 .. 3 a wavefront per row with
 * 1 / 2 / 4 / 8 quads per lane (n <= 256, 512, 1 024, 2 048); 4 .. 6 a workgroup per row with 4 / 8 / 11 quads per thread
 * (n <= 8 192, 16 384, 22 528); 7 the re-reading fallback.  Bit 3: float4 loads (aligned != 0: every row array on 16 bytes, and n a
 * multiple of 4); it changes the loads inside an instance, never the instance.  n <= 0: -1. */
int lipasr_debug_apgd_path(int n, int aligned);

/* (ours: the reference has no score-based search; this is Square Attack of Andriushchenko, Croce, Flammarion, Hein 2020, "Square
 * Attack: a query-efficient black-box adversarial attack via random search", the L-inf form, ART's SquareAttack, restated from the
 * paper and from memory of ART: parity unpinned)  A random search over sign patterns, one query per iteration.
 * Row geometry.  A row is height x width, n = height * width, element (r, c) at r * width + c (MFCC rows: height the coefficient axis,
 * width the frame axis).  n_valid goes with height == 1 only (a non-NULL n_valid with height > 1 is LIPASR_EINVAL): nv =
 * min(max(n_valid[b], 0), n) as lipasr_genetic_breed takes it, NULL: nv = n; elements k >= nv carry the bits of x0 in every buffer at
 * all times.
 * Perturbed value.  Every perturbed element is v(s) = min(max(fl(x0 + s eps), clip_lo), clip_hi) with s = +1 or -1 (-INFINITY /
 * +INFINITY: no clamp; a NaN stays a NaN).
 * gen(seed; lo, hi0, hi1) is the Philox4x32-10 block with key seed and counter (lo low word, lo high word, hi0, hi1).
 *
 * lipasr_square_init writes the paper's vertical-stripe start into x_best AND x_cand: column c gets one sign for all its rows, bit
 * c & 31 of word (c >> 5) & 3 of gen(seed; (c >> 7) | 1 << 62, clip0 + b, restart << 24) (1: s = -1), and win[b] = (0, 0, 0, 0).
 * restart < 256, eps finite and >= 0, clip_lo <= clip_hi, height * width <= 2^31 - 1, or LIPASR_EINVAL. */
int lipasr_square_init(lipasr_handle_t h, const float* x0 /* [batch][height * width] */, const int* n_valid /* [batch] or NULL */,
                       int batch, int height, int width, uint32_t clip0, uint32_t restart, uint64_t seed, float eps, float clip_lo,
                       float clip_hi, float* x_best, float* x_cand, int* win /* [batch][4] */, lipasr_stream_t stream);

#define LIPASR_SQUARE_LAST 1 /* flags bit 0: the last query of a run: bookkeeping only, no new proposal */
/* One launch per query: finishes proposal `it` and writes proposal it + 1.  logits [batch][classes] are the model's outputs at
 * x_cand; y = labels[b].  Per row, in this order:
 *   1. loss = z_y - max_{c != y} z_c in fp32, one subtraction (targeted: its negative, y the class to reach); classes == 1: +inf; a
 *      NaN anywhere in the row: NaN; a label outside [0, classes): +inf.
 *   2. it == 0 (the stripe start; win is empty): loss_best = loss, a NaN stored as +INFINITY.  it > 0: where the row was not done on
 *      arrival and loss < loss_best (strict; a NaN never wins), the elements inside win[b] = (r, c, h, w) are copied from x_cand to
 *      x_best and loss_best = loss; otherwise the same elements are copied back from x_best to x_cand.  Only the window is touched:
 *      a step moves O(window) bytes, not O(n).
 *   3. done[b] is sticky: a row that arrives with done == 0 and now has loss_best < 0 gets done = it + 1, the number of queries it
 *      took, the start counted as query 1.
 *   4. A row that is done, a row with nv == 0, and every row under LIPASR_SQUARE_LAST gets no new proposal: win[b] = (0, 0, 0, 0)
 *      and x_cand equals x_best bit for bit.  Every other row draws proposal it + 1 from o = gen(seed; 0, clip0 + b,
 *      restart << 24 | (it + 1)): the window is win_h x win_w when n_valid == NULL, and 1 x clamp((nv * p_q + 2^23) >> 24, 1, nv)
 *      with n_valid, p_q = round(p * 2^24); its corner is uniform over the positions that keep it inside the row, or inside
 *      [0, nv): r = (o[0] * (height - h + 1)) >> 32, c = (o[1] * (width - w + 1)) >> 32 in 64-bit integers (with n_valid: nv for
 *      width); bit 0 of o[2] is the sign of the whole window (1: s = -1).  x_cand gets v(s) inside the window, win[b] its
 *      (r, c, h, w).
 * Everything is integer arithmetic, one fp32 add, two clamps and one fp32 subtract: draws and values are a pure function of (seed,
 * row index, restart, iteration), chunks of any size at any clip0 reproduce one big call bit for bit, and the host twins below give
 * the same bits.  One workgroup per row, no workspace, no atomics; any n, any alignment of the row buffers (scalar accesses: the
 * values never depend on it).
 * it < 2^24, restart < 256, 1 <= classes <= 32, 1 <= win_h <= height, 1 <= win_w <= width, p_q <= 2^24, flags within
 * LIPASR_SQUARE_LAST, eps finite and >= 0, clip_lo <= clip_hi, x_best overlapping neither x_cand nor x0 (nor x_cand x0), or
 * LIPASR_EINVAL; batch == 0 or n == 0: LIPASR_OK with nothing written; null pointers (n_valid excepted) are refused before the device
 * is touched. */
int lipasr_square_step(lipasr_handle_t h, const float* logits /* [batch][classes] */, const int* labels /* [batch] */,
                       const float* x0, const int* n_valid /* [batch] or NULL */, int batch, int classes, int height, int width,
                       int win_h, int win_w, uint32_t p_q, int targeted, uint32_t clip0, uint32_t restart, uint32_t it, int flags,
                       uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best, float* x_cand,
                       float* loss_best /* [batch] */, int* done /* [batch] */, int* win /* [batch][4] */, lipasr_stream_t stream);

/* Host-only (no GPU needed): the two calls above on host arrays, the same inline functions in plain loops -- the CPU-side pin of the
 * counters.  Same checks, same bits. */
int lipasr_square_init_host(const float* x0, const int* n_valid, int batch, int height, int width, uint32_t clip0, uint32_t restart,
                            uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best, float* x_cand, int* win);
int lipasr_square_step_host(const float* logits, const int* labels, const float* x0, const int* n_valid, int batch, int classes,
                            int height, int width, int win_h, int win_w, uint32_t p_q, int targeted, uint32_t clip0, uint32_t restart,
                            uint32_t it, int flags, uint64_t seed, float eps, float clip_lo, float clip_hi, float* x_best, float* x_cand,
                            float* loss_best, int* done, int* win);

/* ------------------------------------------------------------------ HopSkipJump (Chen, Jordan, Wainwright 2020)
 * The decision-based minimum-norm attack: it asks only "is this point adversarial?".  adversarial(z, y): argmax z != y (targeted:
 * == y), the lowest index on a tie; a row with a NaN logit or a label outside [0, classes) is NOT adversarial.  norm is 2.0f or
 * +INFINITY (else LIPASR_EINVAL).  Rows have any length and alignment: float4 where n is a multiple of 4 and every row buffer sits on
 * 16 bytes, scalars otherwise, never changing a value.  nv = clamp(n_valid[b], 0, n), or n when n_valid == NULL: elements at or beyond
 * nv keep the bits of the clean row in everything written.  clamp(v) = min(max(v, clip_lo), clip_hi) by comparisons (+-INFINITY: no
 * clamp).  No atomics, nothing waits on another workgroup, two runs give the same bits.
 *
 * lipasr_hsj_expand: row b * draws + j of out is clamp(fmaf(s, r, x[b])) with s = (float)((double)delta[b] / ||r||_2) (0 where the
 * draw is empty or delta[b] is not finite) and r the draw draw0 + j of iteration `it` of clip clip0 + b: element 4 q + e of r is word
 * e of the Philox block gen(seed; q | (draw0 + j) << 32, clip0 + b, tag << 28 | it), tag 2 / 3,
 *   norm inf: (k - 2^23) / 2^23 with k = (word >> 8) + 1, uniform on (-1, 1]; ||r||_2 = sqrt(sum (k - 2^23)^2) / 2^23, the sum in
 *             64-bit integers (n <= 2^17 or LIPASR_EINVAL): the bits of the host twin;
 *   norm 2:   normal4 (Box-Muller on the block); ||r||_2 from an fp64 sum.  logf / sinf / cosf differ between device and host.
 * Chunks of draws (draw0) and of clips (clip0) reproduce one big call bit for bit.  it < 2^24. */
int lipasr_hsj_expand(lipasr_handle_t h, const float* x /* [batch][n] */, const float* delta /* [batch] */,
                      const int* n_valid /* [batch] or NULL */, int batch, int n, int draws, uint32_t clip0, uint32_t it, uint32_t draw0,
                      uint64_t seed, float norm, float clip_lo, float clip_hi, float* out /* [batch * draws][n] */,
                      lipasr_stream_t stream);

/* logits [batch * draws][classes] are the model's outputs at the rows p [batch * draws][n] that lipasr_hsj_expand wrote around
 * x [batch][n].  phi_j = +1 where row j is adversarial, -1 otherwise.  Adds, in fp64 and in ascending j,
 *   sums[b][0][k] += p_j[k] - x[k],   sums[b][1][k] += phi_j (p_j[k] - x[k])        (k < nv; nothing is added beyond),
 *   counts[b][0] += draws,            counts[b][1] += the number of phi_j = +1,
 * to a workspace the caller zeroed before the first chunk of an iteration: chunks of draws add up to the bits of one call.
 * 1 <= classes <= 32, draws <= 16384 per call (phi sits in LDS, one byte per draw), batch <= 65535, or LIPASR_EINVAL. */
int lipasr_hsj_accumulate(lipasr_handle_t h, const float* logits, const int* labels /* [batch] */, const float* p, const float* x,
                          const int* n_valid, int batch, int classes, int n, int draws, int targeted,
                          double* sums /* [batch][2][n] */, int* counts /* [batch][2] */, lipasr_stream_t stream);

/* u [batch][n] from the workspace: with m = (2 counts[b][1] - counts[b][0]) / counts[b][0],
 *   g_k = fma(-m, sums[b][0][k], sums[b][1][k]); every phi +1: g = sums[b][0]; every phi -1: g = -sums[b][0]; no draws: g = 0;
 *   norm inf: u = sign(g) with sign(0) = 0 (a NaN: 0); norm 2: u = (float)(g / ||g||_2), the norm in fp64, lane-serial then a
 *   fixed-order tree, u = 0 where it is 0 or not finite.  u is 0 beyond nv. */
int lipasr_hsj_direction(lipasr_handle_t h, const double* sums, const int* counts, const int* n_valid, int batch, int n, float norm,
                         float* u /* [batch][n] */, lipasr_stream_t stream);

#define LIPASR_HSJ_START 0  /* mode: the start draws */
#define LIPASR_HSJ_HALVE 1  /* mode: the step-size halving */
#define LIPASR_HSJ_BISECT 2 /* mode: the bisection between x0 and the far point */
#define LIPASR_HSJ_FIRST 1  /* flags bit 0: opens a phase: no logits are read, the first candidate is written */
#define LIPASR_HSJ_LAST 2   /* flags bit 1 (START only): the last start draw: a row that is still not adversarial gives up */
/* One launch per query.  logits [batch][classes] are the model's outputs at x_cand (not read under LIPASR_HSJ_FIRST, may be NULL
 * then).  A row's scalars: fstate[b] = (lo, hi, mid, thresh, eps, dist, dist_best, dist_far), istate[b] = (active, found, ok, moved,
 * halvings, queries, 0, 0).  A row that is not active is left alone (outside FIRST); every active row counts one query per call.
 *   START | FIRST  reads istate[b][0] (the caller's: attack this row?) and sets everything else: x_adv = x_best = x0, the three
 *                  distances +inf, active = asked and nv > 0.  x_cand = start draw 0 (active) or x0.
 *   START          `draw` is the draw the logits belong to.  adversarial: x_far = x_cand, found = ok = 1, done.  Otherwise draw + 1
 *                  goes to x_cand, or under LAST the row gives up.  Start draw d, element 4 q + e: clamp(fmaf(u01(word e),
 *                  start_hi[b] - start_lo[b], start_lo[b])) to [start_lo[b], start_hi[b]], gen(seed; q | d << 32, clip0 + b, 1 << 28).
 *   HALVE | FIRST  active = found, ok = 0, halvings = 0, eps = dist * step_scale; x_cand = clamp(fmaf(eps, u, x_adv)).
 *   HALVE          adversarial: x_far = x_cand, ok = 1, done.  Otherwise halvings += 1; at max_halvings the row is done with ok = 0;
 *                  else eps *= 0.5 and x_cand is written again.
 *   BISECT | FIRST active = ok, moved = 0, lo = 0; norm 2: hi = 1, thresh = theta[b]; norm inf: dist_far = ||x_far - x0||_inf,
 *                  hi = dist_far, thresh = min(dist_far * theta[b], theta[b]).  Then as below from "finished?".
 *   BISECT         adversarial: hi = mid, moved = 1; otherwise lo = mid.  Finished (hi - lo <= thresh, or 0.5 (lo + hi) no longer
 *                  strictly inside): x_adv = P(hi) where moved, else the bits of x_far; dist = ||x_adv - x0|| in the attack's
 *                  norm (norm 2: fp64 sum, rounded once); where dist < dist_best, x_best = x_adv and dist_best = dist; done.
 *                  Otherwise mid = 0.5 (lo + hi) and x_cand = P(mid).  P(a) = clamp(fmaf(a, x_far, fmaf(-a, x0, x0))) for norm 2
 *                  and clamp(min(max(x_far, x0 - a), x0 + a)) for norm inf: x_adv is written by the function that wrote the
 *                  candidate the model called adversarial, with the same a.
 * 1 <= classes <= 32, max_halvings >= 1, step_scale finite and >= 0, clip_lo <= clip_hi, the row buffers not overlapping, or
 * LIPASR_EINVAL; batch == 0 or n == 0: LIPASR_OK with nothing written. */
int lipasr_hsj_search(lipasr_handle_t h, const float* logits, const int* labels, const float* x0, const int* n_valid,
                      const float* u /* [batch][n]; HALVE */, const float* start_lo /* [batch] */, const float* start_hi /* [batch] */,
                      const float* theta /* [batch] */, int batch, int classes, int n, int mode, int flags, int targeted,
                      uint32_t clip0, uint32_t draw, uint64_t seed, float norm, float step_scale, int max_halvings, float clip_lo,
                      float clip_hi, float* x_cand, float* x_far, float* x_adv, float* x_best, float* fstate /* [batch][8] */,
                      int* istate /* [batch][8] */, lipasr_stream_t stream);

/* Host-only (no GPU needed): the four calls above on host arrays, from the same inline functions in plain loops.  Same checks; the
 * same bits except where fp64 sums run in another order (the L2 norms) or the libm differs (the L2 draws). */
int lipasr_hsj_expand_host(const float* x, const float* delta, const int* n_valid, int batch, int n, int draws, uint32_t clip0,
                           uint32_t it, uint32_t draw0, uint64_t seed, float norm, float clip_lo, float clip_hi, float* out);
int lipasr_hsj_accumulate_host(const float* logits, const int* labels, const float* p, const float* x, const int* n_valid, int batch,
                               int classes, int n, int draws, int targeted, double* sums, int* counts);
int lipasr_hsj_direction_host(const double* sums, const int* counts, const int* n_valid, int batch, int n, float norm, float* u);
int lipasr_hsj_search_host(const float* logits, const int* labels, const float* x0, const int* n_valid, const float* u,
                           const float* start_lo, const float* start_hi, const float* theta, int batch, int classes, int n, int mode,
                           int flags, int targeted, uint32_t clip0, uint32_t draw, uint64_t seed, float norm, float step_scale,
                           int max_halvings, float clip_lo, float clip_hi, float* x_cand, float* x_far, float* x_adv, float* x_best,
                           float* fstate, int* istate);
/* Host-only: the instance lipasr_hsj_expand takes for rows of n elements -- the quads a thread holds (1, 2, 4, 8 in
 * workgroups of 256 threads up to n = 8 192; 4, 6 plus 32 in workgroups of 1 024 threads up to n = 24 576; 0: the draw is generated
 * twice) -- plus 64 where float4 accesses are taken. */
int lipasr_debug_hsj_path(int n, int aligned);

/* The over-the-air channel (lipasr/room.py, OverTheAirClassifier): a bank of room impulse responses rirs [rir_count][taps] (device)
 * between the loudspeaker and the microphone, as a batched FIR.  x is [clips][n]; out and g are [clips * rir_count][n], row
 * b * rir_count + j being clip b through room j.  n_valid [clips] (or NULL: n for every clip) holds POSITIONS IN THE ROW, not
 * samples at the file's rate; values are clamped to [0, n]; nv_b below is the clamped value.
 *   lipasr_room_apply:  out[b * R + j][t] = sum_{k = 0}^{min(t, taps - 1)} rirs[j][k] * x[b][t - k]   for t < nv_b, 0 for nv_b <= t < n.
 *   lipasr_room_vjp:    gx[b][s] = scale * sum_j sum_{k < taps, s + k < nv_b} rirs[j][k] * g[b * R + j][s + k]   for s < nv_b, 0 beyond:
 *                       the exact adjoint of lipasr_room_apply with the rooms summed in the same launch.
 * The response is causal, as long as its input and CUT at the end of the clip: the reverberant tail past nv_b is dropped, so that a
 * clip's length means the same thing on both sides of the channel (an MFCC stage behind it takes the same lengths).  x and g are
 * read only below nv_b.  Arithmetic: exact fp32 (v_mfma_f32_32x32x2_f32, one fma chain per output element, by room and then by
 * signal position upwards); no atomics, no workspace, one launch, nothing allocated or synchronised, so two runs give the same bits
 * and a clip's rows have the bits they would have if the clip were launched alone.  The signals are taken as finite: the zeros of
 * the banded operand are multiplied, not skipped.  Any n up to 2^30, any taps in [1, 8192], any alignment of every pointer (all
 * accesses are single floats).  LIPASR_OK without a launch when clips, rir_count or n is 0; LIPASR_EINVAL for taps outside
 * [1, 8192], a null pointer (n_valid excepted), a non-finite scale, or an output that overlaps an input -- all before the device is
 * touched. */
int lipasr_room_apply(const float* x, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n, float* out,
                      lipasr_stream_t stream);
int lipasr_room_vjp(const float* g, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n, float scale,
                    float* gx, lipasr_stream_t stream);
/* Host-only (no GPU needed): the same formulas on host arrays in plain loops, the fp32 accumulator taking the taps in (j, k)
 * order, each tap the exact product added and rounded to fp32.  Same checks. */
int lipasr_room_apply_host(const float* x, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n,
                           float* out);
int lipasr_room_vjp_host(const float* g, const int* n_valid, const float* rirs, int taps, int rir_count, int clips, int n,
                         float scale, float* gx);

/* Universal adversarial perturbations (lipasr/universal.py, attacks.UniversalPerturbation; ART's UniversalPerturbation in its
 * minibatch form): ONE perturbation `noise`, float32 [P], shared by every row of a batch.  Its period P >= 1 may equal the row
 * width n, be shorter (the snippet loops) or longer (a row sees a window of it).  offs [batch] (int32, or NULL: all zero) is a
 * shift per row: position k of row b is paired with noise[(k + offs[b]) mod P].  0 <= offs[b] < P is the caller's promise; the
 * kernels reduce ((offs[b] % P) + P) % P all the same, so that no value indexes outside noise.  n_valid [batch] (or NULL: n) holds
 * POSITIONS IN THE ROW, clamped to [0, n]; nv_b below is the clamped value.  Limits: batch <= 65535, n <= 2^17, P <= 2^17, else
 * LIPASR_EINVAL.  Every entry point refuses a null pointer (offs and n_valid excepted) before the device is touched, returns
 * LIPASR_OK with nothing written when batch, n or P is 0 (lipasr_universal_step: groups or P), allocates nothing and synchronises
 * nothing.  No atomics anywhere: two runs give the same bits. */
#define LIPASR_UNIVERSAL_GROUP 64 /* the rows whose sum one slab of lipasr_universal_reduce's output holds */

/* The shifts of rows clip0 .. clip0 + batch - 1 at iteration `it`, one launch: o = Philox4x32-10 with key `seed` and the counter
 * words (clip0 + b, 0, it, 0x554E4956), offs_out[b] = (uint64(o[0]) * P) >> 32, in [0, P).  A pure function of (seed, clip0 + b,
 * it, P): chunks at any clip0 reproduce one big call bit for bit. */
int lipasr_universal_shifts(lipasr_handle_t h, int batch, int P, uint32_t clip0, uint32_t it, uint64_t seed, int* offs_out /* [batch] */,
                            lipasr_stream_t stream);

/* out[b][k] = clamp(x[b][k] + noise[(k + offs[b]) mod P], clip_lo, clip_hi) for k < nv_b -- one fp32 add, then
 * v < lo ? lo : (v > hi ? hi : v), so that a NaN stays -- and the bits of x[b][k] for k >= nv_b.  One launch; every access is a single
 * float, consecutive lanes consecutive positions: any n, any alignment, one instance, so no value depends on the alignment.  out must overlap neither x nor noise, and clip_lo <= clip_hi, else LIPASR_EINVAL. */
int lipasr_universal_apply(lipasr_handle_t h, const float* x /* [batch][n] */, const float* noise /* [P] */, const int* offs,
                           const int* n_valid, int batch, int n, int P, float clip_lo, float clip_hi, float* out /* [batch][n] */,
                           lipasr_stream_t stream);

/* The adjoint of the broadcast, and the hot path: the gradient rows g [batch][n] summed back onto the period.  sums is
 * double [G][P], G = ceil(batch / LIPASR_UNIVERSAL_GROUP); it is WRITTEN, not added to (no memset).  sums[grp][p] is the fp64
 * sum, started at +0.0, of (double)g[b][k] over the rows b of group grp in ascending b and, within a row, over the positions
 * k < nv_b with (k + offs[b]) mod P == p in ascending k; a NaN entry counts as 0 (as in lipasr_lp_step).  Pure fp64 additions in
 * an order that is a function of (batch, P) alone -- never of the grid, the CU count or the alignment -- so the result is the
 * same bits on every run, the bits of the host twin and of a float64 loop in the stated order, and minibatches cut at multiples
 * of LIPASR_UNIVERSAL_GROUP give the slabs of one big call.  One launch of G x ceil(P / 256) independent workgroups: a lane owns one
 * period position and reads every row of its group as coalesced dwords from (p - offs[b]) mod P in strides of P.  sums must not
 * overlap g. */
int lipasr_universal_reduce(lipasr_handle_t h, const float* g /* [batch][n] */, const int* offs, const int* n_valid, int batch, int n,
                            int P, double* sums /* [G][P] */, lipasr_stream_t stream);

/* One step of the noise, in place.  G[p] = sum over grp of sums[grp][p], in ascending grp, in fp64.  `norm` is 2.0f or +INFINITY,
 * else LIPASR_EINVAL; alpha finite (a negative alpha descends: the targeted attack); eps >= 0, +inf: no projection.
 *   inf: noise[p] = clamp(noise[p] + alpha * sign(G[p]), -eps, eps), sign(0) = sign(NaN) = 0: the product is +-alpha or +-0 exactly,
 *        so this is all fp32 and exact.  Element-wise, ceil(P / 256) workgroups.
 *   2:   N = sqrt(sum_p G[p]^2) in fp64; d'[p] = noise[p] + (alpha * G[p]) / (N + 1e-7) in fp64, or noise[p] where N is not finite
 *        (such a call takes no step and only projects); M = sqrt(sum_p d'[p]^2); r = eps / (M + 1e-7);
 *        noise[p] = (float)(d'[p] * (r < 1 ? r : 1)), the factor being 1 under eps = +inf.  ONE launch of ONE workgroup of 1024
 *        threads: thread t adds its terms p = t, t + 1024, ... in ascending order into one fp64 partial, and the partials meet
 *        in block_sum_d's order (a butterfly per wavefront, then the 16 wavefronts in index order).  A second launch would cost
 *        more than the three passes one workgroup makes over P <= 2^17 positions whose partials sit in L2.
 * groups <= ceil(65535 / LIPASR_UNIVERSAL_GROUP); noise must not overlap sums. */
int lipasr_universal_step(lipasr_handle_t h, float* noise /* [P] */, const double* sums /* [groups][P] */, int groups, int P, float norm,
                          float alpha, float eps, lipasr_stream_t stream);

/* Host-only (no GPU needed): the same inline functions in plain loops, the same checks.  The same bits as the device entry
 * points everywhere except the norm-2 sums of lipasr_universal_step, which the host adds in ascending p. */
int lipasr_universal_shifts_host(int batch, int P, uint32_t clip0, uint32_t it, uint64_t seed, int* offs_out);
int lipasr_universal_apply_host(const float* x, const float* noise, const int* offs, const int* n_valid, int batch, int n, int P,
                                float clip_lo, float clip_hi, float* out);
int lipasr_universal_reduce_host(const float* g, const int* offs, const int* n_valid, int batch, int n, int P, double* sums);
int lipasr_universal_step_host(float* noise, const double* sums, int groups, int P, float norm, float alpha, float eps);

/* ---------------------------------------------------------------- certified robustness by bound propagation (ours)
 * The reference has no certificate.  For the classifier in inference mode,
 *     z_l = W_l h_{l-1} + b_l,  h_l = s_l relu(z_l) + t_l,  s = gamma / sqrt(var + 1e-3f), t = beta - s mean (s = 1, t = 0 without
 *     BatchNorm),  logits = z_L,
 * and the input set  { v : ||v - x_b||_p <= eps_b } /\ [clip_lo, clip_hi]^n  (p = norm: +INFINITY or 2.0f, else LIPASR_EINVAL; no clip
 * box: -INFINITY, +INFINITY), lipasr_mlp_bounds writes lower bounds of the margins  z_L[y_b] - z_L[k]  over the whole set:
 *   margin_ibp[b][k]    interval bounds (Gowal et al. 2018) through the hidden layers, then the difference row W_L[y_b] - W_L[k] on
 *                       the last hidden box (not the difference of two logit bounds);
 *   margin_crown[b][k]  (may be NULL: no backward pass) one backward linear-relaxation pass from that difference row down to the
 *                       input (CROWN-IBP, Zhang et al. 2020): an unstable ReLU takes the line hi / (hi - lo) (z - lo) where its
 *                       coefficient is negative and, where it is not, z if hi >= -lo and 0 otherwise; at the input the minimum of
 *                       the linear function over the box coordinate by coordinate, under norm 2 the larger of that and
 *                       Lambda . x - eps ||Lambda||_2;
 *   slack[b][k]         (may be NULL; needs margin_crown) what the backward pass subtracted for fp32 / fp64 rounding.
 * Column k = y_b holds +INFINITY (slack 0): the smallest entry of a row is its certificate, and the row is certified at eps_b when
 * max(margin_ibp, margin_crown) > 0 in every column.  The bounds hold for the REAL-arithmetic function of the fp32 parameters:
 * every fp32 sum is widened by gamma_{K+1} S + 2 (K + 1) 2^-149 (S = the sum of magnitudes, gamma_n = n 2^-24 / (1 - n 2^-24)),
 * every other step is made in fp64 and rounded outward ("Bound propagation").
 *   layer_lo / layer_hi (may be NULL): the boxes the forward pass kept, one span each:
 *       [ input box [batch][n_0] | z_1 [batch][n_1] | h_1 [batch][n_1] | z_2 | h_2 | ... ]  over the hidden layers 1 .. L - 1.
 *   Under norm 2 the first layer is centred on x with the radius min(|W_1|^T r, eps_b ||W_1[:, j]||_2), r the half-width of the box
 *   around x; the column norms are taken once per call.
 *   workspace: device floats, any 4-byte alignment, lipasr_mlp_bounds_workspace(m, batch) of them; the library keeps nothing
 *   between calls.  Widths <= 4096, classes <= 32, batch * classes <= 2^24: LIPASR_EINVAL otherwise, as for a null argument, a
 *   workspace that is too small, a clip box with clip_lo > clip_hi or a NaN, and an output or the workspace overlapping anything.
 * eps and y are device arrays: a row with a negative or NaN eps_b, a y_b outside [0, classes) or a NaN in x gets NaN margins and
 * touches no other row (the host twin, which can look, refuses the first two with LIPASR_EINVAL).
 * Launches: forward L + 1 (bounds_prep_kernel, L - 1 bounds_layer_kernel, bounds_head_kernel), backward L (L - 1
 * bounds_back_kernel, bounds_tail_kernel), L = n_layers; two device-to-device copies for layer_lo / layer_hi.  Every sum runs in
 * one order that depends on the shapes alone (no atomics): two calls give the same bits. */
int lipasr_mlp_bounds_workspace(lipasr_mlp_t m, int batch, size_t* floats);
int lipasr_mlp_bounds(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x /* [batch][n_0] */,
                      const float* eps /* [batch] */, float norm, float clip_lo, float clip_hi, const int* y /* [batch] */, int batch,
                      float* workspace, size_t workspace_floats, float* margin_ibp /* [batch][classes] */,
                      float* margin_crown /* may be NULL */, float* slack /* may be NULL */, float* layer_lo /* may be NULL */,
                      float* layer_hi /* may be NULL */, lipasr_stream_t stream);
/* Host-only (no GPU needed): the same inline functions in plain loops and in the same orders, the same checks, on a model given
 * by its widths [n_layers + 1] and BatchNorm flags [n_layers] (NULL: none) with params / bnstate in lipasr_mlp_create's layout.
 * The same values as the device entry point (a zero may differ in sign). */
int lipasr_mlp_bounds_workspace_host(int n_layers, const int* widths, int batch, size_t* floats);
int lipasr_mlp_bounds_host(int n_layers, const int* widths, const int* bn, const float* params, const float* bnstate, const float* x,
                           const float* eps, float norm, float clip_lo, float clip_hi, const int* y, int batch, float* workspace,
                           size_t workspace_floats, float* margin_ibp, float* margin_crown, float* slack, float* layer_lo,
                           float* layer_hi);
/* Test hook: launches since the library was loaded of 0 bounds_prep_kernel, 1 bounds_layer_kernel, 2 bounds_head_kernel,
 * 3 bounds_back_kernel, 4 bounds_tail_kernel, counted on the host where the launch happens; -1 for an unknown id. */
long lipasr_debug_bounds_launches(int kernel);

/* IBP certified training (Gowal et al. 2018; lipasr.bounds.IBPCrossentropy): the backward pass of the interval bounds with respect
 * to the parameters.  From what ONE lipasr_mlp_bounds call under norm +INFINITY wrote for (params, bnstate, y, batch) --
 * margin_ibp and the boxes layer_lo / layer_hi -- per row b
 *     u[b][k] = -margin_ibp[b][k] (k != y_b),  u[b][y_b] = 0,   loss_rows[b] = logsumexp_k u[b][k]
 * (the cross-entropy of the worst-case logits, the last layer elided into the difference rows as lipasr_mlp_bounds does) and
 *     grads = scale_old * grads + scale_new * d( sum_b loss_rows[b] ) / d params          (scale_old == 0: the old contents of grads are ignored)
 * over W, b, gamma and beta of every layer in lipasr_mlp_create's flat layout; the pad floats are not touched.  The running
 * BatchNorm statistics are constants, dropout is off.  Derivative conventions (torch's): relu'(0) = 0; d|w|/dw = 0 at 0; s >= 0
 * takes the branch that does not swap lo and hi; the difference W_L[j][y] - W_L[j][k] selects lo where it is > 0 and hi otherwise;
 * the widening and the outward roundings of the forward pass are constants; the input box carries no gradient.  Per hidden layer,
 * with c = (lo + hi) / 2 and r = (hi - lo) / 2 of its input box, gc = g_zlo + g_zhi, gr = g_zhi - g_zlo:
 *     dW[i][j] = sum_b c[b][i] gc[b][j] + sign(W[i][j]) sum_b r[b][i] gr[b][j],   db[j] = sum_b gc[b][j],
 *     g_lo, g_hi = (gc W^T -+ gr |W|^T) / 2, then through h = s relu(z) + t with the gates z_lo > 0 / z_hi > 0.
 * A row whose margins are NaN, or whose y_b is outside [0, classes), makes loss_rows[b] and the whole gradient NaN.
 *   workspace: device floats, any 4-byte alignment, lipasr_mlp_bounds_grad_workspace(m, batch) of them; nothing is kept between calls.
 *   LIPASR_EINVAL for a null argument, a workspace that is too small, grads / loss_rows / the workspace overlapping anything,
 *   widths > 4096, classes > 32 or batch * classes > 2^24.
 * Launches: 2 for one layer, else 3 (L - 1) + 1 -- bg_head_kernel, bg_head_dw_kernel (dW_L, db_L), and per hidden layer
 * bg_colsum_kernel (db, dgamma, dbeta), bg_wgrad_kernel (dW on v_mfma_f32_32x32x2_f32, both scales in its epilogue) and, above the
 * first, bg_back_kernel (W and |W| from one read, the gates of the layer below in its epilogue).  Every sum runs in one order that
 * the shapes fix (no atomics): two calls give the same bits.  Nothing allocates or synchronises. */
int lipasr_mlp_bounds_grad_workspace(lipasr_mlp_t m, int batch, size_t* floats);
int lipasr_mlp_bounds_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* margin_ibp /* [batch][classes] */,
                           const float* layer_lo, const float* layer_hi, const int* y /* [batch] */, int batch, float* workspace,
                           size_t workspace_floats, float scale_old, float scale_new, float* grads, float* loss_rows /* [batch] */,
                           lipasr_stream_t stream);
/* Host-only twins on widths and BatchNorm flags, as lipasr_mlp_bounds_host: the same inline functions in plain loops and in the
 * same orders, the same checks, the same values as the device entry point (a zero may differ in sign). */
int lipasr_mlp_bounds_grad_workspace_host(int n_layers, const int* widths, int batch, size_t* floats);
int lipasr_mlp_bounds_grad_host(int n_layers, const int* widths, const int* bn, const float* params, const float* bnstate,
                                const float* margin_ibp, const float* layer_lo, const float* layer_hi, const int* y, int batch,
                                float* workspace, size_t workspace_floats, float scale_old, float scale_new, float* grads,
                                float* loss_rows);
/* Test hook: launches since the library was loaded of 0 the two head kernels, 1 bg_wgrad_kernel, 2 bg_back_kernel,
 * 3 bg_colsum_kernel, counted on the host where the launch happens; -1 for an unknown id. */
long lipasr_debug_bounds_grad_launches(int kernel);

/* CROWN-IBP certified training (Zhang et al. 2020; lipasr.bounds.CrownIBPCrossentropy): the backward pass of the relaxation with
 * respect to the parameters.  From what ONE lipasr_mlp_bounds call under norm +INFINITY wrote for (params, bnstate, y, batch) with
 * margin_crown requested and the boxes kept, per row b and with beta in [0, 1]
 *     mixed[b][k] = (1 - beta) margin_ibp[b][k] + beta margin_crown[b][k]
 *     u[b][k] = -mixed[b][k] (k != y_b),  u[b][y_b] = 0,   loss_rows[b] = logsumexp_k u[b][k]
 *     grads = scale_old * grads + scale_new * d( sum_b loss_rows[b] ) / d params          (scale_old == 0: the old contents of grads are ignored)
 * in the layout and with the conventions of lipasr_mlp_bounds_grad.  margin_crown is differentiated along the chain
 * Lambda_l -> nu_l -> Lambda_{l-1} and through the pre-activation boxes that set the upper line of every unstable neuron; further
 * constants: the slack, the (1 + 2^-40) factors of that line.  Further conventions (torch's): a coefficient p < 0 takes the upper
 * line, anything else the lower one, whose slope carries no gradient; Lambda_0 > 0 selects lo of the input box, anything else hi.
 * A row whose margins are NaN, or whose y_b is outside [0, classes), makes loss_rows[b] and the whole gradient NaN.
 *   workspace: device floats, any 4-byte alignment, lipasr_mlp_bounds_crown_grad_workspace(m, batch) of them -- every level of the
 *   chain is kept, twice batch * classes * (n_0 + ... + n_{L-1}) floats and more; nothing is kept between calls.
 *   LIPASR_EINVAL for everything lipasr_mlp_bounds_grad refuses, a null margin_crown, and beta outside [0, 1] or NaN.
 * Launches with L layers: beta == 0 makes exactly the launches of lipasr_mlp_bounds_grad and writes its bits.  Otherwise 5 for
 * L = 1 and 10 (L - 1) + 3 for L >= 2: cg_soft_kernel (1), cg_relax_kernel (max(L - 1, 1)), bounds_back_kernel (L - 1),
 * per hidden layer cg_adjoint_kernel, cg_wgrad_kernel (v_mfma_f32_32x32x2_f32 both; the rows split over blockIdx.z), cg_wreduce_kernel,
 * cg_colsum_kernel (the column sums, M split over blockIdx.y) and cg_finish_kernel (the injections; db, dgamma, dbeta), cg_head_kernel (1), then the 3 (L - 1) + 1 (2 for L = 1) launches of
 * lipasr_mlp_bounds_grad's sweep, which takes the mixed margins and the gradient on the boxes.  Every sum runs in one order that
 * the shapes fix (no atomics): two calls give the same bits.  Nothing allocates or synchronises. */
int lipasr_mlp_bounds_crown_grad_workspace(lipasr_mlp_t m, int batch, size_t* floats);
int lipasr_mlp_bounds_crown_grad(lipasr_mlp_t m, const float* params, const float* bnstate, const float* margin_ibp /* [batch][classes] */,
                                 const float* margin_crown /* [batch][classes] */, const float* layer_lo, const float* layer_hi,
                                 const int* y /* [batch] */, int batch, float beta, float* workspace, size_t workspace_floats,
                                 float scale_old, float scale_new, float* grads, float* loss_rows /* [batch] */, lipasr_stream_t stream);
/* Host-only twins, as lipasr_mlp_bounds_grad_host: the same values as the device entry point (a zero may differ in sign). */
int lipasr_mlp_bounds_crown_grad_workspace_host(int n_layers, const int* widths, int batch, size_t* floats);
int lipasr_mlp_bounds_crown_grad_host(int n_layers, const int* widths, const int* bn, const float* params, const float* bnstate,
                                      const float* margin_ibp, const float* margin_crown, const float* layer_lo, const float* layer_hi,
                                      const int* y, int batch, float beta, float* workspace, size_t workspace_floats, float scale_old,
                                      float scale_new, float* grads, float* loss_rows);
/* Test hook: launches since the library was loaded of 0 cg_soft_kernel, 1 cg_relax_kernel, 2 bounds_back_kernel (as this call
 * launches it), 3 cg_adjoint_kernel, 4 cg_wgrad_kernel, 5 cg_wreduce_kernel, 6 cg_colsum_kernel, 7 cg_finish_kernel, 8 cg_head_kernel;
 * the sweep of lipasr_mlp_bounds_grad counts under lipasr_debug_bounds_grad_launches; -1 for an unknown id. */
long lipasr_debug_bounds_crown_grad_launches(int kernel);

/* The time-warp operator (lipasr/warp.py, attacks.TimeWarp; ours -- ART's SpatialTransformation is the image form): every clip
 * resampled under K triples (shift in samples, rate, linear gain) by band-limited interpolation, in one launch.  x is [clips][n];
 * params is float32 [clips * K][3], one triple per OUTPUT row, so every clip may carry its own candidates; out and g are
 * [clips * K][n], row b * K + j being clip b under its candidate j.  n_valid [clips] (or NULL: n for every clip) holds POSITIONS IN
 * THE ROW, clamped to [0, n]; nv below is the clamped value.
 * The interpolation kernel is a Kaiser-windowed sinc, tabulated as resampy tabulates its own: Z = 16 zero crossings per wing, P = 512
 * table steps per crossing, win[i] = sinc(i / P) kaiser(beta = 8.6) for i = 0 .. Z P, computed in float64 and rounded once to fp32,
 * with win[0] = 1 and win[k P] = 0 EXACTLY for k = 1 .. Z; delta[i] = fp32(win[i + 1] - win[i]), delta[Z P] = 0
 * (lipasr_warp_table_host writes both, Z P + 1 floats each).  `table` is the two interleaved, float32 [Z P + 1][2] = (win, delta).
 * The cutoff is Nyquist and there is no roll-off, so that integer positions reproduce samples exactly; the price is paid near
 * Nyquist, where 16 crossings are too few: a sine at 0.8 of Nyquist is interpolated to 4e-5 of its amplitude, one at 0.9 to 7e-2,
 * one at 0.95 to 0.36 ("Time warp").  The 22 050 Hz rows of 16 kHz files hold nothing above 0.73 of Nyquist.  The cutoff
 * does not follow the rate either: a rate above 1 aliases whatever the clip holds above 1 / rate of Nyquist.
 *   For t < nv, in fp64:  c = (nv - 1) / 2,  u = c + rate (t - c) - shift,  n0 = floor(u),  f = u - n0   (rate warps about the
 *   clip's centre; a positive shift delays);  idx = f P, j0 = (int)idx, eta = (float)(idx - j0).
 *   acc, an fp32 fmaf chain from 0 with every tap weight w = fmaf(eta, delta[j], win[j]): first the left wing i = 0 .. Z - 1, sample
 *   n0 - i at table index j0 + i P; then the right wing from idx' = (1 - f) P in the same way, k = 0 .. Z - 1, sample n0 + 1 + k.
 *   A source position outside [0, nv) is absent, as is a table index beyond Z P.
 *   out[row][t] = gain * acc (one fp32 rounding) for t < nv, 0 for nv <= t < n.
 * lipasr_warp_param_vjp writes gp, float64 [clips * K][3] (any 4-byte boundary).  With dxu[t] the same chain over the slopes
 * (delta[j] * P on the left wing, -delta[j] * P on the right; the exact derivative of the table's piecewise-linear form):
 *   gp[row][0] = sum_t g gain (-dxu),   gp[row][1] = sum_t (g gain dxu) (t - c),   gp[row][2] = sum_t g acc,   all over t < nv,
 * the products and sums in fp64: thread t mod 512 adds its terms in ascending t, then row.h's block_sum_d (a butterfly per
 * wavefront, then the 8 wavefronts in index order).
 * Both: one launch, no workspace, nothing allocated or synchronised, no atomics: two runs give the same bits, and a clip's rows
 * have the bits they would have if the clip were launched alone.  Any n up to 2^24, any K >= 1, any 4-byte alignment of every
 * pointer.  LIPASR_OK without a launch when clips, K or n is 0; LIPASR_EINVAL, before the device is touched, for a null pointer
 * (n_valid excepted), n above 2^24, or an output that overlaps an input.  Signals are taken as finite.  A row whose triple is not
 * finite, or whose rate lies outside [0.5, 2], is written as NaN over [0, nv) (gp: three NaN) and touches no other row. */
int lipasr_warp_apply(const float* x /* [clips][n] */, const int* n_valid, const float* params /* [clips * K][3] */,
                      const float* table /* [Z P + 1][2] */, int clips, int K, int n, float* out /* [clips * K][n] */,
                      lipasr_stream_t stream);
int lipasr_warp_param_vjp(const float* x, const float* g /* [clips * K][n] */, const int* n_valid, const float* params,
                          const float* table, int clips, int K, int n, double* gp /* [clips * K][3] */, lipasr_stream_t stream);
/* Host-only (no GPU needed): the table, and the same chains in the same order on host arrays (general path only, absent taps left
 * out where the device multiplies a staged zero): the same bits as the device entry points on finite signals.  Same checks. */
int lipasr_warp_table_host(float* win /* [Z P + 1] */, float* delta /* [Z P + 1] */);
int lipasr_warp_apply_host(const float* x, const int* n_valid, const float* params, const float* table, int clips, int K, int n,
                           float* out);
int lipasr_warp_param_vjp_host(const float* x, const float* g, const int* n_valid, const float* params, const float* table, int clips,
                               int K, int n, double* gp);
/* Test hook: launches since the library was loaded of 0 warp_kernel<false> (apply), 1 warp_kernel<true> (param_vjp), counted on the
 * host where the launch happens; -1 for an unknown id. */
long lipasr_debug_warp_launches(int kernel);

/* Input-transformation defences over audio (lipasr/defences.py, estimators.DefendedClassifier; ours -- ART's SpatialSmoothing,
 * FeatureSqueezing and Resample preprocessors are the NumPy forms): a chain of 1 to LIPASR_DEFENCE_MAX_STAGES stages over rows
 * x [clips][n], in one launch, and the chain's vector-Jacobian product in one launch.  The chain is three HOST arrays of `stages`
 * entries: kinds (LIPASR_DEFENCE_*), args (the width, the tap count or the bits) and taps (for a FIR stage the DEVICE pointer of
 * its float32 taps, any 4-byte boundary; ignored for the other kinds, and the array may be NULL when no stage is a FIR).  They
 * are read before the call returns.  n_valid [clips] (or NULL: n for every clip) holds POSITIONS IN THE ROW, clamped to [0, n];
 * nv below is the clamped value.  Every stage reads its input as 0 outside [0, nv) and writes exactly 0 there, so the chain is the
 * composition of its stages, each as if launched alone.
 *   MEDIAN, odd width k in 3 .. 15, h = (k - 1) / 2:  out[t] = the element of rank h of x[t - h .. t + h].  Elements are ordered by
 *       (value, position) with values compared as floats: -0 and +0 tie and the position decides; the padding zeros take part as
 *       elements at their positions.  The output carries the bits of the selected element.
 *       vjp: gx[s] = sum of g[t] over the t whose selected element is position s, from 0 in ascending t in fp32; the gradient of
 *       an output that selected a padding zero is dropped.
 *   FIR, odd tap count <= 255, c = (taps - 1) / 2:  out[t] = sum_k h[k] x[t + c - k] (centred: zero phase for symmetric taps), one
 *       fmaf chain from 0 in ascending k over every k (an absent sample is a 0 operand).
 *       vjp, the exact adjoint: gx[s] = sum_k h[k] g[s - c + k], g read as 0 outside [0, nv), the same chain.
 *   QUANTIZE, bits in 2 .. 16, q = 2^(bits - 1):  out[t] = clamp(rintf(x[t] q), -q, q - 1) / q: exact in fp32 (ties to even).
 *       vjp: straight-through where the clamp was idle (gx[s] = g[s], its bits), 0 where it acted.
 * The half-widths of a chain (h, c, 0) may sum to at most LIPASR_DEFENCE_MAX_HALO.  A workgroup owns 1 024 positions of one clip
 * and keeps every intermediate in LDS; the vjp launch recomputes the forward pass over the halo it needs and reads no saved state.
 * No element's arithmetic depends on the tiling, the batch or the alignment: two runs give the same bits, a clip's row has the
 * bits it would have if launched alone, and a chain gives the bits of its stages launched one after the other.
 * Both: one launch, no workspace, nothing allocated or synchronised, no atomics.  Any n up to 2^30, any clips, any 4-byte
 * alignment of every pointer.  Signals and taps are taken as finite.  LIPASR_EINVAL, before the device is touched and whatever the
 * sizes: stages outside 1 .. 4, kinds or args NULL, an unknown kind, an even or out-of-range width, tap count or bits, a FIR stage
 * without taps, a halo above the limit, a negative size.  Then LIPASR_OK without a launch when clips or n is 0; else LIPASR_EINVAL
 * for a null x, g, out or gx and for an output that overlaps an input or the taps. */
#define LIPASR_DEFENCE_MEDIAN 0
#define LIPASR_DEFENCE_FIR 1
#define LIPASR_DEFENCE_QUANTIZE 2
#define LIPASR_DEFENCE_MAX_STAGES 4
#define LIPASR_DEFENCE_MAX_HALO 256
int lipasr_defence_apply(const float* x /* [clips][n] */, const int* n_valid, const int* kinds /* host [stages] */,
                         const int* args /* host [stages] */, const float* const* taps /* host [stages] of device pointers */,
                         int stages, int clips, int n, float* out /* [clips][n] */, lipasr_stream_t stream);
int lipasr_defence_vjp(const float* x, const float* g /* [clips][n] */, const int* n_valid, const int* kinds, const int* args,
                       const float* const* taps, int stages, int clips, int n, float* gx /* [clips][n] */, lipasr_stream_t stream);
/* Host-only (no GPU needed): the same inline functions over whole rows in plain loops, on host arrays (taps: host pointers).  The
 * same bits as the device entry points on finite signals.  Same checks. */
int lipasr_defence_apply_host(const float* x, const int* n_valid, const int* kinds, const int* args, const float* const* taps,
                              int stages, int clips, int n, float* out);
int lipasr_defence_vjp_host(const float* x, const float* g, const int* n_valid, const int* kinds, const int* args,
                            const float* const* taps, int stages, int clips, int n, float* gx);
/* Test hook: launches since the library was loaded of 0 defence_apply_kernel, 1 defence_vjp_kernel, counted on the host where the
 * launch happens; -1 for an unknown id. */
long lipasr_debug_defence_launches(int kernel);

/* One fused FGSM/PGD iteration (attacks.py:506-510, 657-661): inference forward at x_adv, CE
 * gradient, backward to the input, and the K4 sign step applied in place on x_adv inside the last
 * backward GEMM's epilogue (dx never reaches memory). */
int lipasr_mlp_attack_step(lipasr_mlp_t m, const float* params, const float* bnstate, float* x_adv,
                           const float* x0, const float* y_onehot, int batch, float alpha, float eps,
                           lipasr_stream_t stream);

/* One FGM / PGD iteration in any norm (1.0f, 2.0f or +INFINITY; else LIPASR_EINVAL): norm inf IS lipasr_mlp_attack_step
 * (same launches, same bits).  Norm 1, 2: inference forward at x_adv, CE gradient, backward to the input with dx stored in a
 * plan workspace buffer, then the lipasr_lp_step kernel -- one launch more than the fused inf path, because the step needs
 * a norm over the whole row of dx and the row spans several column tiles of the dX GEMM.  alpha < 0 is the targeted attack
 * (ART multiplies the gradient by 1 - 2 targeted; y_onehot then holds the targets). */
int lipasr_mlp_attack_step_lp(lipasr_mlp_t m, const float* params, const float* bnstate, float* x_adv, const float* x0,
                              const float* y_onehot, int batch, float norm, float alpha, float eps, lipasr_stream_t stream);

/* ART y=None: labels := one-hot argmax of the estimator's own prediction. */
int lipasr_mlp_own_labels(lipasr_mlp_t m, const float* params, const float* bnstate, const float* x,
                          int batch, float* y_onehot_out, lipasr_stream_t stream);

/* ------------------------------------------------------------------ K1: MFCC
 * extract_features / compute_mfcc_all_files (extract_features_construct_dataset.py:24-39,144-150):
 * librosa.load(mono=True) resampling sr_in -> 22050 Hz (resampy kaiser_best), then
 * librosa.feature.mfcc defaults (reflect-padded STFT 2048/512 periodic Hann, power, 128 Slaney
 * mels, 10 log10 with amin 1e-10 and top_db 80 per clip, DCT-II ortho, 20 coefficients), frame
 * axis truncated / zero-padded to utterance_length, flattened coefficient-major
 * (index = coeff*utterance_length + frame).
 *
 * lipasr_mfcc_plan builds the tables for (sr_in, n_samp) and allocates intermediates for
 * batch_max clips; it must precede the launch functions (not capturable itself). */
int lipasr_mfcc_plan(lipasr_handle_t h, int sr_in, int n_samp, int batch_max);
/* Same with an explicit window: librosa.feature.mfcc(y, sr, n_fft=n_fft, win_length=n_fft,
 * hop_length=hop).  (2048, 512) is the plan above (LDS Stockham FFT).  Any 32 <= n_fft <= 510 with
 * 1 <= hop <= n_fft selects the short-window path, where the windowed real DFT is an fp32 MFMA
 * contraction -- the Speaker-recognition features (Speaker recognition/
 * extract_features_construct_dataset.py:224-226: win_length=441, n_fft=441, hop_length=220 on
 * 1-s windows at 22 050 Hz -> 20 x 101 = 2020).  Other values: LIPASR_EUNSUPPORTED.  The short-window path reflects once: a clip
 * with n_y <= n_fft / 2 is LIPASR_EINVAL ("clip shorter than the reflect padding"). */
int lipasr_mfcc_plan_ex(lipasr_handle_t h, int sr_in, int n_samp, int batch_max, int n_fft, int hop);
/* resampled length int(ceil(n_samp*22050/sr_in)) and frame count 1 + n_y/hop for a plan */
int lipasr_mfcc_dims(lipasr_handle_t h, int* n_y, int* n_frames);

/* wav: [batch][n_samp] float32 mono in [-1,1).  out: [batch][20*utterance_length].
 * affine_mean / affine_scale: optional device double [20*utterance_length]; when given the output
 * is (mfcc - mean)/scale (the precomputed StandardScaler of A2 fused into the last kernel). */
int lipasr_mfcc_f32(lipasr_handle_t h, const float* wav, int batch, int utterance_length,
                    const double* affine_mean, const double* affine_scale, float* out,
                    lipasr_stream_t stream);
/* stage 1 only: y [batch][n_y] (librosa.load output) */
int lipasr_resample_f32(lipasr_handle_t h, const float* wav, int batch, float* y, lipasr_stream_t stream);
/* stages 2..: from an already-resampled 22050 Hz signal y [batch][n_y] (the audio-noise attacks add
 * noise here, attacks.py:108-114, 264-267). */
int lipasr_mfcc_from_22k(lipasr_handle_t h, const float* y, int batch, int n_y, int utterance_length,
                         const double* affine_mean, const double* affine_scale, float* out,
                         lipasr_stream_t stream);

/* 16-bit PCM input (the corpus is 16-bit PCM wav, extract_features_construct_dataset.py:27: librosa.load
 * decodes to float32 by a 2^-15 scale) and clips of DIFFERENT lengths in one launch
 * (compute_mfcc_all_files, :144-150, loops files of any length): pcm is [batch][n_samp] int16 where
 * n_samp is the plan's sample count; n_valid (device int [batch], may be NULL = n_samp everywhere) gives
 * the samples of each row that belong to the clip.  Clip u is processed exactly as a plan of
 * n_valid[u] samples would process it alone (resampled length, frame count, reflect padding and the
 * top_db maximum follow its own length; frames past its end are the zero columns of :33-37).  Same
 * bits as lipasr_mfcc_f32 on pcm * 2^-15.  Needs the 2048/512 path with the 441/320 or 441/160 resampler
 * (16 kHz / 8 kHz input); otherwise LIPASR_EUNSUPPORTED.  Rows whose length is a multiple of 4 samples go
 * through the same three kernels as float32 batches (the resampler reads int16 and cuts each row at its
 * clip's end); other row lengths through the fused resample -> STFT kernel. */
int lipasr_mfcc_i16(lipasr_handle_t h, const int16_t* pcm, const int* n_valid, int batch,
                    int utterance_length, const double* affine_mean, const double* affine_scale,
                    float* out, lipasr_stream_t stream);

/* MFCC plans as objects: each owns its tables and intermediates, so several extractors (a training
 * pipeline's and a validation pass's, or two streams) coexist on one handle without re-planning.
 * The handle-level entry points above operate on the handle's default plan.
 * sample_format: 0 = float32 in [-1, 1), 1 = int16 PCM.  n_valid as in lipasr_mfcc_i16. */
int lipasr_mfcc_create(lipasr_handle_t h, int sr_in, int n_samp_max, int batch_max, int n_fft, int hop,
                       lipasr_mfcc_t* out);
int lipasr_mfcc_destroy(lipasr_mfcc_t p);
/* fused (may be NULL): 1 when the plan runs resampling and STFT as ONE kernel (the resampled signal stays in LDS) */
int lipasr_mfcc_plan_dims(lipasr_mfcc_t p, int* n_y, int* n_frames, int* fused);
int lipasr_mfcc_extract(lipasr_mfcc_t p, const void* wav, int sample_format, const int* n_valid, int batch,
                        int utterance_length, const double* affine_mean, const double* affine_scale,
                        float* out, lipasr_stream_t stream);
int lipasr_mfcc_plan_resample(lipasr_mfcc_t p, const float* wav, int batch, float* y, lipasr_stream_t stream);
int lipasr_mfcc_plan_from_22k(lipasr_mfcc_t p, const float* y, int batch, int n_y, int utterance_length,
                              const double* affine_mean, const double* affine_scale, float* out,
                              lipasr_stream_t stream);

/* Backward pass of K1 (2048/512 plans): the vector-Jacobian product g_sig = J^T g_feat of the feature map
 *   out[k L + t] = (c[k][t] - mean) / scale,  c = D max(dB, clipmax - 80),  dB = 10 log10 max(1e-10, W |STFT(R x)|^2)
 * for a cotangent g_feat [batch][20 L] (what lipasr_mlp_input_grad writes).  In order: Gc = g / scale (frames >= L and the
 * zero columns of fix_frames receive nothing), Gdbc = D^T Gc, Gdb = Gdbc where dB > clipmax - 80 and 0 elsewhere, the position of
 * the clip maximum (which may lie in a frame >= L) also receives the sum of Gdbc over the floored elements, Gmel = Gdb (10/ln 10)
 * / mel where mel > 1e-10, GP = W^T Gmel, Z = 2 GP X on the 1025 one-sided bins (no Hermitian doubling), frame gradient =
 * hann * Re(sum_k Z[k] e^{+2 pi i k n / 2048}), overlap-add, adjoint of the reflect padding (the flanks fold back onto
 * y[1 .. 1024] and y[n_y - 1025 .. n_y - 2]), and for domain 0 the adjoint of the resampler (the appended zero sample gets
 * nothing).  With several equal maxima the FIRST in (frame, mel) order takes the floored sum -- autograd's even split between
 * them is not reproduced; max(dB, floor) passes the gradient to dB only where dB > floor.  An all-zero clip gives an all-zero
 * gradient.
 *   domain 0: sig [batch][n_samp] at the plan's sr_in, g_sig [batch][n_samp];
 *   domain 1: sig [batch][n_y] at 22 050 Hz (lipasr_mfcc_plan_from_22k's input), g_sig [batch][n_y].
 *   affine_scale: the StandardScaler scale the forward applied (device double [20 L]) or NULL (= 1).
 *   flags bit 0: the caller ran THIS plan's forward (lipasr_mfcc_extract for domain 0, lipasr_mfcc_plan_from_22k for domain 1) on
 *     exactly this signal and batch as the plan's last call, on this stream: the plan's intermediates are read instead of
 *     re-running the forward kernels: the resampled signal always, the dB tile and frame maxima where that forward ran the kernel
 *     the backward pass runs for itself -- stft_mel2_kernel (stage-mask bit 256) or, on short-window plans, dft_mel_kernel.  The
 *     default block-DFT kernel windows in the frequency domain and loses, on a frame with a loud burst under the tail of its
 *     window, digits that 1 / mel magnifies here, and stft_mel_kernel (bit 64) sends two frames of any loudness through one
 *     transform: their tiles are never read, and stft_mel2_kernel runs again inside the call.  Same bits either way.  bit 1: the rows are int16 PCM, bit 2: the rows have per-clip
 *     lengths -- neither has a backward pass: LIPASR_EUNSUPPORTED, as for short-window plans and clips of n_y <= 2048.
 * Every sum runs in a fixed order (no floating-point atomics): two calls give the same bits.  No host synchronisation; the
 * plan's backward workspaces are allocated by the first call (make it outside a graph capture). */
int lipasr_mfcc_plan_vjp(lipasr_mfcc_t p, const float* sig, int domain, int batch, int utterance_length,
                         const double* affine_scale, const float* g_feat, float* g_sig, int flags,
                         lipasr_stream_t stream);
/* The same backward pass for clips of different lengths in ONE launch, as lipasr_mfcc_extract's n_valid gives the forward.
 *   n_valid: device int [batch], required: the samples of each row that belong to its clip, ALWAYS counted at the plan's input
 *     rate, also for domain 1 (clamped to [0, n_samp]).  Clip u has n_vy = int(n r) resampled samples, n_y = ceil(n r) after
 *     fix_length and 1 + n_y / 512 frames (none for n_y < 2), r = 22050 / sr_in; a domain-1 row holds its clip in its first
 *     ceil(n r) positions.  Whatever else a row holds is ignored.
 *   sample_format: 0 float32, 1 int16 PCM (domain 0 only; it matters where the forward is re-run: g_sig is float32, the gradient
 *     with respect to pcm * 2^-15).
 *   g_sig: [batch][n_samp] (domain 0) or [batch][n_y] (domain 1), rows as long as the plan's; the gradient is exactly 0 from the
 *     clip's end (n_valid[u], or ceil(n r)) to the end of the row, and a clip of n_valid <= 0 (or of fewer than 2 resampled samples)
 *     gets an all-zero row.
 *   flags bit 0: the plan's last call on this stream was the forward with per-clip lengths on exactly these rows and this
 *     n_valid (lipasr_mfcc_extract with n_valid for domain 0, lipasr_mfcc_plan_from_22k_ragged for domain 1).  Same bits.
 * Clips may be as short as 2 resampled samples: the adjoint of the reflect padding sums every padded position that reflects
 * onto a sample, in ascending order (np.pad reflects repeatedly once n_y <= 1024); a clip of n_y > 2048 keeps the three-term
 * form and the bits lipasr_mfcc_plan_vjp gives for it alone.  Runs on the plans whose three-kernel forward takes per-clip
 * lengths: 2048/512 at 16 kHz or 8 kHz, rows a multiple of 4 samples, 16-byte (float32) / 8-byte (int16) aligned row pointers.
 * LIPASR_EUNSUPPORTED with a message otherwise: short-window plans, other rates, a plan that runs the fused resample -> STFT
 * kernel for this input (it leaves no resampled signal behind), int16 with domain 1.  Fixed summation order, no host
 * synchronisation, workspaces allocated by the first call, as above. */
int lipasr_mfcc_plan_vjp_ragged(lipasr_mfcc_t p, const void* sig, int sample_format, const int* n_valid, int domain,
                                int batch, int utterance_length, const double* affine_scale, const float* g_feat,
                                float* g_sig, int flags /* bit 0: reuse the forward */, lipasr_stream_t stream);
/* The backward pass for the SHORT-WINDOW plans (lipasr_mfcc_plan_ex / lipasr_mfcc_create with n_fft, hop other than 2048, 512: the
 * Speaker-recognition features, n_fft = win_length = 441, hop 220).  Arguments, domains, affine_scale and flags bit 0 mean what
 * they mean for lipasr_mfcc_plan_vjp; rows are float32 and of one length (no other flag bit).  The chain: Gc = g / scale, Gdbc =
 * D^T Gc, the top_db floor with the floored sum handed to the first clip maximum, Gmel = Gdb (10/ln 10) / mel where mel > 1e-10
 * (the many empty mel bands of a small n_fft sit at -100 dB and receive nothing) -- the kernel of the 2048/512 chain as it is --
 * then, per 32 consecutive frame rows of the forward's padded layout: X = frames T recomputed on the fp32 matrix instruction
 * against the forward's folded table, GP = W^T Gmel from the CSR mel bank by bin, Z = 2 GP X, a second contraction over the bins
 * against the same table (S[n] = sum_b Zre[b] Tre[n][b], A[n] = sum_b Zim[b] Tim[n][b]), frame sample n <- S[n] + A[n] and
 * N - n <- S[n] - A[n] (2 S[n] where n pairs with itself; the window is inside the table), overlap-add in ascending frame order
 * (frames with an all-zero cotangent row are left out: their samples receive exactly 0), the sum of the two workgroup images that
 * cover a padded position, the adjoint of the single reflection (g_y[i] = gyp[i + pad] + gyp[pad - i] for 1 <= i <= pad, +
 * gyp[pad + 2 (n_y - 1) - i] for n_y - 1 - pad <= i <= n_y - 2, pad = n_fft / 2), and for domain 0 the adjoint of the resampler.
 * LIPASR_EUNSUPPORTED with a message: a 2048/512 plan (lipasr_mfcc_plan_vjp is for those, and keeps refusing short-window plans),
 * n_fft > 33 hop (more than two images of 32 frames would overlap), more than 512 of min(frames, utterance_length).  Fixed
 * summation order and no floating-point atomics (two calls give the same bits), an all-zero clip gives an all-zero gradient, no
 * host synchronisation, workspaces allocated by the first call (make it outside a graph capture). */
int lipasr_mfcc_plan_vjp_short(lipasr_mfcc_t p, const float* sig, int domain, int batch, int utterance_length,
                               const double* affine_scale, const float* g_feat, float* g_sig, int flags,
                               lipasr_stream_t stream);
/* The two halves of lipasr_mfcc_extract with n_valid (same semantics as above; composed they give its bits).  _resample_ragged
 * leaves zeros from int(n r) to the end of every row of y [batch][n_y]; _from_22k_ragged reads a row's first ceil(n r)
 * positions, position int(n r) as the zero fix_length appends. */
int lipasr_mfcc_plan_resample_ragged(lipasr_mfcc_t p, const void* wav, int sample_format, const int* n_valid, int batch,
                                     float* y, lipasr_stream_t stream);
int lipasr_mfcc_plan_from_22k_ragged(lipasr_mfcc_t p, const float* y, const int* n_valid, int batch, int utterance_length,
                                     const double* affine_mean, const double* affine_scale, float* out,
                                     lipasr_stream_t stream);
/* g_wav [batch][n_samp] = R^T g_y [batch][n_y]: the adjoint of lipasr_mfcc_plan_resample (any plan whose ratio keeps one
 * q-block's window of g_y in LDS; its tap table is built by the first call) */
int lipasr_mfcc_plan_resample_vjp(lipasr_mfcc_t p, const float* g_y, int batch, float* g_wav, lipasr_stream_t stream);

/* Per-kernel HIP-event timing of the next `max_calls` extractions -- lipasr_mfcc_f32 calls, or
 * lipasr_resample_f32 + lipasr_mfcc_from_22k pairs -- recorded on the stream the kernels run on.
 * _end synchronises and returns the average milliseconds of {resample, stft_mel, dct}
 * (host float[3]) and the number of extractions measured (host int).  On the fused path there is no
 * resampling kernel: slot 0 is 0 and slot 1 is the fused resample + STFT + mel kernel. */
int lipasr_mfcc_profile_begin(lipasr_handle_t h, int max_calls);
int lipasr_mfcc_profile_end(lipasr_handle_t h, float* avg_ms3, int* n_calls);
int lipasr_mfcc_plan_profile_begin(lipasr_mfcc_t p, int max_calls);
int lipasr_mfcc_plan_profile_end(lipasr_mfcc_t p, float* avg_ms3, int* n_calls);
/* Knobs of one plan.
 * key 0: the stage mask, for profiling and A/B runs (0 = the default path everywhere).  Every bit:
 *       1  stft_mel_kernel skips its FFT passes          (wrong results: times the remaining stages)
 *       2  stft_mel_kernel skips the mel reduction       (wrong results)
 *       4  the VALU resamplers (resample_reg128_kernel / resample_generic_kernel) instead of any MFMA resampler
 *       8  resample_mfma_kernel skips its MFMA chain     (wrong results)
 *      16  the fp32 resamplers instead of the fp16-plane one: its parity reference.  Rows that cannot be read as float4 go to
 *          resample_mfma_kernel, where the same bit skips the LDS fill (wrong results); aligned rows never reach that kernel
 *      64  the round-2 STFT kernel (stft_mel_kernel, two frames per workgroup); no per-clip lengths then
 *     128  never the fused resample -> STFT kernel: always resample, STFT, DCT with the resampled signal in HBM
 *     256  on the three-kernel path: the Stockham FFT kernel (stft_mel2_kernel) instead of the block-DFT kernel on the
 *          matrix pipe (stft_bdft_kernel, the default): its parity reference.  Inside the fused kernel: stop before the
 *          frames (wrong results).  An extraction runs one of the two paths, so the two meanings never meet.
 *     512  the fused kernel skips the resampling          (wrong results)
 *   65536, 131072, 262144 (bits 16-18)  resample_persist_h2_kernel skips its MFMA chain / its stores / the prefetch of the
 *          next window                                    (wrong results)
 *   Bits 1, 2 and 64 also select stft_mel_kernel; the other bits are unused.
 * key 1: number of workgroups the persistent resampler aims for = the CUs its stream may use (default 256; a pipeline
 *   that runs the MFCC on a CU-masked stream sets it to the size of the mask).
 * key 2: value != 0 makes the plan run the fused resample -> STFT kernel for every batch (1.7x the algorithmic HBM bytes
 *   instead of 4.6x, but about 1.7x the time of the three-kernel path on a whole MI355X: DESIGN.md section 3); by default
 *   the fused kernel runs only where the three-kernel path cannot read the input (int16 or per-clip lengths in rows that
 *   are not a multiple of 4 samples long).
 * key 3: frames per workgroup of the block-DFT kernel (a multiple of 4 in [4, 4096]; default 44 = one workgroup per 1-s clip).
 * key 4: value != 0 lets that kernel apply the top_db floor and the DCT itself when one workgroup covers a whole clip
 *   (<= 64 frames, utterance_length <= 64): no dct_kernel launch, bit-identical features; off by default (slower on batches
 *   that are not cache-warm: DESIGN.md section 3).
 * Replaces the arithmetic of librosa.feature.mfcc's STFT, extract_features_construct_dataset.py:30. */
int lipasr_mfcc_plan_set(lipasr_mfcc_t p, int key, int value);

/* ------------------------------------------------------------------ DolphinAttack: inaudible voice commands
 * "Voice digit recogniton/dolphin_attack.m": a 16 kHz voice command as amplitude-modulated ultrasound at 192 kHz, and -- what the
 * script stops short of -- the signal a microphone with a quadratic non-linearity records from it.  One clip of n valid samples x:
 *   band-pass  v = SOS(x): Butterworth order 10, 100 Hz - 7 kHz, as ten biquads (zero initial state, causal).  The script's
 *              filter(b, a, x) on the 20th-order transfer function is unstable in double precision (roots of a at radius 1.0036);
 *              this is the filter that butter() call designs.
 *   up         u[k] = sum_j h_up[k + 120 - 12 j] v[j], k < 12 n (MATLAB resample(v, 12, 1): firls x Kaiser(5), 241 taps, sum 12)
 *   peak 1     m1 = max|u|,  uh = u / m1 (0 when m1 = 0)
 *   modulate   s'[k] = (uh[k] + carrier_level) cos(2 pi carrier_hz k / 192000), the phase (k carrier_hz) mod 192000 in integers
 *   peak 2     m2 = max|s'|,  s = s' / m2 (a silent clip gives the carrier at amplitude 1; 0 when m2 = 0)
 *   microphone w = a1 s + a2 s^2
 *   record     r[i] = sum_k h_dn[12 i + 120 - k] w[k], i < n (resample(w, 1, 12): the same filter with sum 1)
 * The script's carrier_level is 0.001, which makes the recorded signal essentially v^2; 1 is the DolphinAttack paper's form.
 * Arrays: wav, voice, rec [batch][n_samp_max] float32; ultrasound [batch][12 n_samp_max]; peaks [batch][2] = {m1, m2}; n_valid
 * device int [batch] or NULL (= n_samp_max): samples at or past n_valid[u] are never read, outputs at or past n_valid[u]
 * (12 n_valid[u]) are written as 0, the peaks are taken over the valid part, and a clip's result is bit-identical to launching
 * it alone.  The band-pass runs in fp64 (one workgroup per clip, a chunked scan per section), everything else in fp32; sums run
 * in a fixed order.  No launch function synchronises or allocates.  lipasr_dolphin_generate_recorded gives the bits of
 * _generate followed by _record without the [batch][12 n_samp_max] array ever existing (the 192 kHz signal stays in LDS).
 * Errors: sr_in other than 16000: LIPASR_EUNSUPPORTED; carrier_hz not an integer in (7000, 89000), carrier_level < 0, batch >
 * batch_max, a null or destroyed plan: LIPASR_EINVAL.  Plans still alive are freed by lipasr_destroy, next to the MFCC plans. */
int lipasr_dolphin_create(lipasr_handle_t h, int sr_in, int n_samp_max, int batch_max, double carrier_hz, double carrier_level,
                          lipasr_dolphin_t* out);
int lipasr_dolphin_destroy(lipasr_dolphin_t p);
int lipasr_dolphin_bandpass(lipasr_dolphin_t p, const float* wav, const int* n_valid, int batch, float* voice, lipasr_stream_t stream);
int lipasr_dolphin_generate(lipasr_dolphin_t p, const float* wav, const int* n_valid, int batch, float* ultrasound, float* peaks_or_null,
                            lipasr_stream_t stream);
int lipasr_dolphin_record(lipasr_dolphin_t p, const float* ultrasound, const int* n_valid, int batch, float a1, float a2, float* rec,
                          lipasr_stream_t stream);
int lipasr_dolphin_generate_recorded(lipasr_dolphin_t p, const float* wav, const int* n_valid, int batch, float a1, float a2,
                                     float* rec, lipasr_stream_t stream);
/* Host-only (no GPU needed), fp64 as built: which 0 the band-pass as SOS[10][6] (b0 b1 b2 a0 a1 a2 per section), 1 h_up[241],
 * 2 h_dn[241], 3 each section's state-transition matrix to the power 64 [10][4] (the carry of the chunked scan).  Returns the
 * element count (negative = error); out may be NULL to query the size. */
int lipasr_dolphin_table(int which, int sr_in, double* out, int cap);

/* ------------------------------------------------------------------ psychoacoustic masking threshold, imperceptible attack
 * What ART's PsychoacousticMasker and the second stage of its ImperceptibleASR compute ("Speaker recognition/attacks.py":17
 * imports both and uses neither on a waveform).  Window N = 2048, hop 512, periodic Hann w, no padding: frame t is
 * x[512 t .. 512 t + 2048), T = 1 + (n - 2048) / 512 frames, K = 1025 bins, X[k,t] the DFT of w . frame t.
 * Tables (host, fp64; sr = the plan's sample_rate):
 *   f_k = k sr / 2048,  bark_k = 13 atan(0.00076 f) + 3.5 atan((f / 7500)^2),  shift_k = -6.025 - 0.275 bark_k,
 *   ATH_k = 3.64 q^-0.8 - 6.5 exp(-0.6 (q - 3.3)^2) + 0.001 q^4 - 12, q = f / 1000, for 20 <= f <= 20000, -inf outside.
 * PSD:  p[k,t] = max(-200, 20 log10 |sqrt(8/3) X[k,t] / N|),  psd_max = max over the clip,  psd = 96 - psd_max + p.
 * Maskers of a frame v = psd[:, t]:
 *   1. candidates: strict local maxima v[k] > v[k-1], v[k] > v[k+1], 1 <= k <= 1023 (at most 512)
 *   2. level = 10 log10(10^(v[k-1]/10) + 10^(v[k]/10) + 10^(v[k+1]/10));  3. kept when level > ATH_k
 *   4. greedy merge, ascending, i_prev = 0: for i = 1 ...: if bark(i) - bark(i_prev) < 0.5 the smaller of the two is dropped --
 *      level[i_prev] < level[i]: i_prev is dropped and i_prev <- i_prev + 1 (ART's step, kept literally), otherwise (ties too) i
 *      is dropped -- else i_prev <- i.  bark(i) is the Bark value of masker i's bin; with flag bit 0 it is the Bark table at the
 *      LIST POSITION i, ART's code as written.  The comparison runs on the fp64 table.
 *   5. theta[k,t] = 10^(ATH_k/10) + sum_j 10^((level_j + shift_{bin_j} + SF_j(k)) / 10), LINEAR (ART's dB threshold is
 *      10 log10 theta, possibly -inf), 10^(-inf) = 0, dz = bark_k - bark_{bin_j}, SF = 27 dz for dz <= 0 and
 *      (-27 + 0.37 max(level_j - 40, 0)) dz above.
 * Loss of a perturbation delta (same framing):  c = 10^9.6 / 10^(psd_max/10) (8/3) / N^2,  P = c |STFT_delta|^2,
 *   L = (1 / (K T)) sum_{k,t} max(P - theta, 0) per clip, and its gradient
 *   g[n] = sum_t shift_{512 t}(w . g_t),  g_t[n] = sum_{k=0}^{1024} 2 G_k Re(X_k e^{2 pi i k n / N}),  G = c [P > theta] / (K T);
 *   samples past the last frame get exactly 0, and a frame with no bin over theta contributes exactly 0.
 * Step:  delta <- clamp(delta - lr s(g_net + alpha_u g_theta), +-eps_u), s = sign (use_sign) or the identity; then
 *   x_adv <- clamp(x0 + delta, clip_lo, clip_hi) and delta <- x_adv - x0.  alpha, eps: device [batch]; g_theta (with alpha) may be NULL.
 * Arrays: x, delta, g_delta, x_adv, x0, g_net, g_theta [batch][n] float32 (every row of one call has the same n);
 * psd, theta [batch][T][1025], bins contiguous; psd_max, loss [batch]; n_maskers int [batch][T] or NULL.  lipasr_psy_threshold
 * takes ANY PSD as input; lipasr_psy_prepare is _psd followed by _threshold with the PSD kept in the plan's workspace.
 * lipasr_psy_loss_grad with g_delta = NULL computes the loss alone (the same bits).  Everything runs in fp32 (the Bark differences
 * and c are formed in fp64 and rounded once); every sum runs in a fixed order, without atomics: two runs give the same bits.  No launch
 * function synchronises or allocates.  Errors: n < 2048 or > n_max, batch > batch_max, n_frames > the plan's, unknown flag bits, a
 * null array or plan: LIPASR_EINVAL; a plan whose [batch_max][T][1025] tensors pass 2^31 elements: LIPASR_EUNSUPPORTED.  Plans still
 * alive are freed by lipasr_destroy. */
int lipasr_psy_create(lipasr_handle_t h, int sample_rate, int n_max, int batch_max, int flags /* bit 0: bark by position */,
                      lipasr_psy_t* out);
int lipasr_psy_destroy(lipasr_psy_t p);
int lipasr_psy_psd(lipasr_psy_t p, const float* x, int n, int batch, float* psd, float* psd_max, lipasr_stream_t stream);
int lipasr_psy_threshold(lipasr_psy_t p, const float* psd, int n_frames, int batch, float* theta, int* n_maskers_or_null,
                         lipasr_stream_t stream);
int lipasr_psy_prepare(lipasr_psy_t p, const float* x, int n, int batch, float* theta, float* psd_max, lipasr_stream_t stream);
int lipasr_psy_loss_grad(lipasr_psy_t p, const float* delta, int n, int batch, const float* theta, const float* psd_max, float* loss,
                         float* g_delta_or_null, lipasr_stream_t stream);
int lipasr_psy_step(lipasr_psy_t p, float* delta, float* x_adv, const float* x0, const float* g_net, const float* g_theta_or_null,
                    const float* alpha_or_null, const float* eps, int n, int batch, float lr, int use_sign, float clip_lo, float clip_hi,
                    lipasr_stream_t stream);
/* Host-only (no GPU needed), fp64 [1025]: which 0 f, 1 bark, 2 ATH in dB (-inf outside its domain), 3 shift.  Returns the element
 * count (negative = error); out may be NULL to query the size. */
int lipasr_psy_table(int which, int sample_rate, double* out, int cap);

/* A12 audio-domain noise on device, Philox RNG (attacks.py:73-86, 145-183, 222-245), in place on
 * y [batch][n]:  mode 0: y + N(0, p0)               (add_white_noise, sigma = p0)
 *                mode 1: impulse mixture, p = p0, alpha = p1 (add_noise / mixtgauss)
 *                mode 2: white noise at target SNR p0 dB per clip (add_white_noise_with_snr) */
int lipasr_add_noise_f32(lipasr_handle_t h, float* y, int batch, int n, int mode, float p0, float p1,
                         uint64_t seed, lipasr_stream_t stream);

/* Knobs of the handle's default MFCC plan: keys 0 (the stage mask; its bits are listed at lipasr_mfcc_plan_set), 1 and 2 of
 * lipasr_mfcc_plan_set.  The value of key 1 is kept in the handle: a later lipasr_mfcc_plan inherits it. */
int lipasr_debug_set(lipasr_handle_t h, int key, int value);

/* Profiling knob: GEMM kernel choice. bits 0-1: 0 = automatic, 1 = split-K register kernel only, 2 = LDS-tiled kernel
 * wherever it is legal.  bit 2 (4): lipasr_mlp_train_fwd_bwd launches the first layer's weight gradient on its own
 * (as the data-parallel head / dw0 pair does) instead of inside the grouped launch.  bit 3 (8): the grouped weight-gradient
 * launch on 32x32 register-fragment tiles (round 2) instead of 64x64 LDS tiles.  Round 5 (arithmetic mode 2 only): bit 4 (16) the
 * XCD-aware tile order, bit 5 (32) no LDS-DMA ring kernels, bit 6 (64) the weight gradients on 64x64 ring tiles, bit 7 (128) on
 * 128x128 tiles that split per fragment (no split pass), bit 8 (256) no 128x64 exchange tiles, bit 9 (512) no loader-wavefront instance of the 64x64 exchange tile.  Same results in
 * every setting (to the rounding of a different summation order where the tile changes). */
int lipasr_debug_gemm_mode(int mode);

/* Test hook: how many launches since the library was loaded took kernel family `kind` -- 0: forward / input-gradient GEMMs on
 * 128x64 exchange tiles, 1: grouped weight-gradient launches with 128x128 split-pass tiles; -1 for an unknown kind.  (The choice
 * depends on the plan's CU budget; tests that mean to cover those kernels check that they really ran.) */
long lipasr_debug_launch_count(int kind);

/* Test hook: launches since the library was loaded that took exactly one GEMM kernel instance, counted where the launch happens.
 * kind: 0 32x32 fragment tiles with 4 wavefronts, 1 the same with 16 wavefronts splitting K, 2 64x64 LDS tiles, 3 the 64x64
 * LDS-DMA ring tile, 4 its loader-wavefront instance for one workgroup per CU, 5 the 128x64 exchange tile.  exchange: 1 = the
 * instance with the BatchNorm exchange epilogue.  amode / bmode: 1 = the operand is k-major in memory (lipasr_gemm_f32:
 * amode = transA, bmode = !transB).  arith: 0 exact fp32, 1 bf16 operands, 2 fp16 two-plane split.  epi: the epilogue (0 plain
 * store, 1 bias, 2 bias + ReLU, 3 inference BatchNorm, 4 inference dz, 5 sign step, 6 training forward with column sums, 7 training
 * backward with column sums, 8 backward without BatchNorm, 9 softmax + CE, 10 / 11 the forward / backward exchange epilogue), or
 * -1 for any.  Returns -1 for a key the library has no kernel for, so a test can enumerate the instances from the library. */
long lipasr_debug_gemm_launches(int kind, int exchange, int amode, int bmode, int arith, int epi);

/* Test hook, grouped weight-gradient launches.  family 0: 32x32 fragment tiles, 1: 64x64 LDS tiles (variant -1: launches in
 * arithmetic `arith`); family 2: the ring kernel (arith 2 only) -- variant -1: launches; variant 1, 2, 3: problems carried on
 * 64x64 ring tiles, 128x128 split-pass tiles, 128x128 tiles that split per fragment; variant 0: problems the ring layout cannot take,
 * carried by a ring launch on plain tiles.  -1 for an unknown key. */
long lipasr_debug_group_launches(int family, int arith, int variant);

/* Test hook: lipasr_gemm_f32 (arith 0) / lipasr_gemm_f16x2 (arith 2) with the arithmetic mode as an argument, which also reaches
 * the plain product with bf16 operands (arith 1).  The scales are read in mode 2 only (powers of two). */
int lipasr_debug_gemm(lipasr_handle_t h, int arith, int transA, int transB, int M, int N, int K, const float* A, int lda,
                      const float* B, int ldb, float* C, int ldc, float scale_a, float scale_b, lipasr_stream_t stream);

/* Test hook: launches since the library was loaded of one K3 kernel (csrc/spectral_*.hip), counted on the host where the launch
 * happens.  kernel: 0 / 1 / 2 chain_step_kernel<12> / <20> / <32> (at most 12 / 20 / 32 classes), 3 chain_head_kernel, 4 product_sigma_kernel,
 * 5 scale_layers_kernel, 6 sigma_scale_layers_kernel, 7 pi_u_kernel, 8 pi_v_kernel, 9 pi_finish_kernel, 10 sv_clip_kernel,
 * 11 the Frobenius pair (sumsq_clamped_kernel + frob_scale_kernel: one count per pair), 12 bn_correction_kernel.  Returns -1 for an
 * unknown id, so a test can enumerate the kernels from the library. */
long lipasr_debug_k3_launches(int kernel);

/* Test hook: launches since the library was loaded of one kernel instance of the MFCC forward pass (K1), counted on the host where
 * the launch happens.  kernel: 0 / 1 / 2 / 3 resample_persist_h2_kernel for float32 rows / int16 rows / float32 rows with per-clip
 * lengths / int16 rows with per-clip lengths, 4 resample_persist_kernel, 5 resample_mfma_kernel, 6 resample_reg128_kernel,
 * 7 resample_generic_kernel, 8 copy_pad_kernel, 9 clear_tail_kernel, 10 stft_bdft_kernel without its DCT epilogue, 11 stft_bdft_kernel
 * with it (plan key 4), 12 stft_mel2_kernel, 13 stft_mel_kernel, 14 dft_mel_kernel, 15 dct_kernel, 16 mfcc_fused_kernel for float32
 * rows, 17 mfcc_fused_kernel for int16 rows.  The backward pass re-running the forward counts too.  Returns -1 for an unknown id,
 * so a test can enumerate the instances from the library. */
long lipasr_debug_k1_launches(int kernel);

/* Test hook: ONE asynchronous device-to-device copy, on `stream`, of an intermediate that the plan's last forward call left in the
 * plan, into out (device).  which 0: the dB tile [batch][n_frames][128], 10 log10 max(1e-10, mel) BEFORE the top_db floor; which 1:
 * the frame maxima [batch][n_frames] (the maximum over the 128 mels of each row of the tile); which 2: the resampled signal
 * [batch][n_y] that lipasr_mfcc_extract left behind on the three-kernel path (the fused kernel writes none).  Rows and frames are
 * laid out for the plan's n_frames / n_y; with per-clip lengths the frames past a clip's own count hold whatever an earlier call
 * left.  LIPASR_EINVAL for a null argument, a batch outside [1, batch_max] or another `which`.  No synchronisation, no allocation. */
int lipasr_debug_mfcc_stage(lipasr_mfcc_t p, int which, int batch, float* out, lipasr_stream_t stream);

/* Test hook: launches since the library was loaded of one kernel instance of the MFCC backward pass, counted on the host where the
 * launch happens.  kernel: 0 / 1 mfcc_vjp_db_kernel for one length / with per-clip lengths, 2 / 3 stft_vjp_kernel likewise, 4 / 5
 * stft_vjp_fold_kernel likewise, 6 resample_vjp_kernel with 8 outputs per thread, 7 with one output per thread (the 8-output window
 * of g_y exceeds 60 KiB of LDS), 8 / 9 the same two forms with per-clip lengths, 10 copy_cut_kernel (22 050 Hz plans), 11
 * dft_vjp_kernel, 12 dft_vjp_fold_kernel (short-window plans).  The forward kernels a backward call re-runs count in
 * lipasr_debug_k1_launches.  Returns -1 for an unknown id, so a test can enumerate the instances from the library. */
long lipasr_debug_k1_vjp_launches(int kernel);

/* Test hook: ONE asynchronous device-to-device copy, on `stream`, of an intermediate that the plan's last backward call
 * (lipasr_mfcc_plan_vjp, _vjp_ragged, _vjp_short) left in the plan, into out (device).  which 0: Gmel [batch][n_frames][128], d loss /
 * d mel power; which 1: g_y [batch][n_y], the gradient at 22 050 Hz of a domain-0 call (a domain-1 call writes g_sig instead and
 * leaves this array alone).  Rows are laid out for the plan's n_frames / n_y; with per-clip lengths the frames of Gmel past a clip's
 * own count hold whatever an earlier call left.  LIPASR_EINVAL in the cases of lipasr_debug_mfcc_stage, and while the plan has no
 * backward workspaces (they are allocated by its first backward call).  No synchronisation, no allocation. */
int lipasr_debug_mfcc_vjp_stage(lipasr_mfcc_t p, int which, int batch, float* out, lipasr_stream_t stream);

/* Test hook, the opposite direction of lipasr_debug_mfcc_stage: ONE asynchronous device-to-device copy, on `stream`, FROM in (device)
 * INTO the plan.  which 0: the dB tile [batch][n_frames][128]; which 1: the frame maxima [batch][n_frames] (no other `which`).  A
 * backward call with flags bit 0 reads these two arrays instead of re-running the forward (2048/512 plans: with stage-mask bit 256
 * set, see lipasr_mfcc_plan_vjp), so a test can hand step 1 of the chain
 * (DCT^T, top_db floor, dB -> mel) a tile with exact ties or elements exactly on the floor; the later steps recompute X from the
 * signal and do not read the tile.  The next forward call overwrites them.  LIPASR_EINVAL as for lipasr_debug_mfcc_stage. */
int lipasr_debug_mfcc_stage_put(lipasr_mfcc_t p, int which, int batch, const float* in, lipasr_stream_t stream);

/* Test hook: launches since the library was loaded of one of the training step's own kernels (K2 without the GEMMs, K5), counted on
 * the host where the launch happens.  kernel: 0 bn_apply_fwd_kernel with BatchNorm, 1 bn_apply_fwd_kernel as dropout only (a layer
 * with dropout and no BatchNorm), 2 bn_apply_bwd_kernel, 3 part_reduce_kernel (synchronized BatchNorm: lipasr_mlp_train_segment),
 * 4 softmax_ce_kernel, 5 softmax_vjp_kernel, 6 softmax_vjp_onehot_kernel, 7 adam_nonneg_kernel, 8 step_inc_kernel.  The BatchNorm
 * and softmax arithmetic that runs inside a GEMM's epilogue (the exchange epilogue, softmax + CE of at most 32 classes) counts in
 * lipasr_debug_gemm_launches.  Returns -1 for an unknown id, so a test can enumerate the kernels from the library. */
long lipasr_debug_k2_launches(int kernel);

/* Test hook: ONE asynchronous device-to-device copy, on `stream`, of an intermediate that the plan's last call left in the plan's
 * workspace, into out (device), rows packed at the layer's width n_out.  which 0: A_l, the post-ReLU output [batch][n_out]; 1: H_l,
 * after BatchNorm and dropout (A_l itself on a layer with neither); 2: the saved [mean | rstd], [2][n_out], of a training-mode
 * forward; 3: dz_l, the gradient at the pre-activation (for the last layer: at the logits, whichever call wrote it last); 4: the g
 * buffer bn_apply_bwd_kernel read for layer l, dh times dropout [batch][n_out], as the last launch-chain backward of that layer
 * left it; 5: the logits [batch][classes]; 6: the probabilities [batch][classes] the plan kept (a call that was given a `probs` or
 * `logits` destination of the caller's writes there instead).  0, 1, 2 and 4 exist on hidden layers only, 2 and 4 only with
 * BatchNorm, 5 and 6 on the last layer only.  g is ONE buffer for all layers: a whole step overwrites it layer by layer (what is
 * left belongs to the first BatchNorm layer), and the exchange epilogue never writes it -- read it after running only that layer's
 * segment through lipasr_mlp_train_segment, or on a plan with one BatchNorm layer and lipasr_mlp_set_fuse_bn(plan, 0).
 * LIPASR_EINVAL for a null argument, a layer out of range, a batch outside [1, max_batch] or a `which` the layer does not have.  No
 * synchronisation, no allocation. */
int lipasr_debug_mlp_stage(lipasr_mlp_t m, int layer, int which, int batch, float* out, lipasr_stream_t stream);

/* Profiling knob: how many of the leading (small) steps of the product chain W_m^T ... W_1^T run as ONE launch
 * (chain_head_kernel, fp32 matrix instructions): -1 = automatic (the first two steps, when their panels have <= 256 columns
 * in multiples of 16 and there are at most 16 classes; never the last step), 0 = none (one launch per step, rounds 1-3),
 * n = 2 or 3 = at most n.
 * The fused steps associate their sums differently: the product agrees with the per-step launches to ~1e-7. */
int lipasr_debug_chain_head(int n);

/* Host-only (no GPU needed): copies one constant table, exactly as the kernels read it, into `out`
 * and returns its element count (negative = error); out may be NULL to query the size.
 * which: 0 Hann[2048]; 1 DCT[20*128]; 2 dense mel filter bank[128*1025]; 3 polyphase resampling taps
 * [up*taps] for sr_in -> 22050; 4 {up, down, taps, left}; 5 per-phase input offsets [up]. */
int lipasr_debug_table(int which, int sr_in, float* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* LIPASR_H */
