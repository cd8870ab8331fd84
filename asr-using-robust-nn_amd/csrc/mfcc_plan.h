// K1 host side: the MFCC plan (mfcc.hip), the stage-mask bits, the ONE path selector (pick_mfcc_path, mfcc.hip) and the per-stage
// launchers it feeds (resample.hip, stft_mel.hip, mfcc_fused.hip; the default STFT kernel of stft_bdft.hip is declared in stft.h).
#pragma once
#include "common.h"
#include "mfcc_tables.h"
#include "stft.h"

namespace lipasr {

// Stage-mask bits (lipasr_mfcc_plan_set / lipasr_debug_set key 0).  The table for callers is in include/lipasr.h at
// lipasr_mfcc_plan_set; this enum is the only place that holds the values.  Two values carry two names each: the two readers
// of such a bit never run in the same extraction, so they cannot collide --
//   256: SM_STOCKHAM is read by the selector on the three-kernel path, SM_FUSED_STOP inside mfcc_fused_kernel;
//    16: SM_NO_H2 is read by the selector (the persistent fp32 resampler then takes the aligned rows), SM_MFMA_SKIP_FILL inside
//        resample_mfma_kernel, which only gets the rows the persistent kernels cannot read.
enum StageMask : int {
  SM_SKIP_FFT = 1,          // profiling, wrong results: stft_mel_kernel skips its FFT passes
  SM_SKIP_MEL = 2,          // profiling, wrong results: stft_mel_kernel skips the mel reduction
  SM_VALU_RESAMPLER = 4,    // no MFMA resampler of any kind: resample_reg128_kernel / resample_generic_kernel
  SM_MFMA_SKIP_CHAIN = 8,   // profiling, wrong results: resample_mfma_kernel skips its MFMA chain
  SM_NO_H2 = 16,            // the fp32 resamplers instead of the fp16-plane one (its parity reference)
  SM_MFMA_SKIP_FILL = 16,   // profiling, wrong results: resample_mfma_kernel skips its LDS fill
  SM_ROUND2_STFT = 64,      // stft_mel_kernel (two frames per workgroup) instead of stft_mel2_kernel / stft_bdft_kernel
  SM_NO_FUSED = 128,        // never the fused resample -> STFT kernel
  SM_STOCKHAM = 256,        // stft_mel2_kernel instead of the block-DFT kernel (its parity reference)
  SM_FUSED_STOP = 256,      // profiling, wrong results: mfcc_fused_kernel stops before the frames
  SM_FUSED_SKIP_RESAMPLE = 512,  // profiling, wrong results: mfcc_fused_kernel skips the resampling
  // bits 16-18 travel to resample_persist_h2_kernel as dbg = (mask >> SM_H2_SHIFT) & SM_H2_BITS (profiling, wrong results)
  SM_H2_SHIFT = 16, SM_H2_BITS = 7,
  H2_SKIP_MFMA = 1, H2_SKIP_STORE = 2, H2_NO_PREFETCH = 4,
};

// geometry of the MFMA resamplers that the plan, the selector and more than one unit need (described in resample.hip)
constexpr int kRsBand = 152, kRsStride = 481;
constexpr int kRpMaxWaves = 16;
constexpr int kRhK = 160, kRhChunks = kRhK / 16, kRhRowHalfs = 480, kRhRowBytes = 2 * kRhRowHalfs * 2 + 16;
constexpr float kRhTapScale = 64.0f, kRhSigScale = 2048.0f;
constexpr int kFuQ = 16;                                    // q-blocks per workgroup = rows of the 16x16x4 MFMA
constexpr int kFuUp = 441;
constexpr int kDftRows = 64, kDftGroup = 8, kDftMaxTiles = 8;
constexpr int kSvRows = 32;                                 // frame rows per workgroup of dft_vjp_kernel (one MFMA row block)
typedef float rs_f32x16 __attribute__((ext_vector_type(16)));

struct MfccPlan {
  lipasr_ctx* ctx = nullptr;  // owning handle
  int sr_in = 0, n_samp = 0, batch_max = 0;
  int up = 1, down = 1, taps = 0, left = 0;
  int n_valid = 0, n_y = 0, n_frames = 0;
  int n_fft = tables::kNFft, hop = tables::kHop;
  bool dft = false;          // short-window variant: STFT as an MFMA contraction (dft_mel_kernel)
  int dft_krows = 0, dft_tiles = 0, dft_rpc = 0;
  float* d_dft = nullptr;    // [dft_krows][dft_tiles*64] windowed DFT matrix
  bool identity = false;  // sr_in == 22050
  float* d_h = nullptr;   // [up][taps]
  int* d_noff = nullptr;  // [up]
  float* d_hband = nullptr;  // [n_ptiles][kRsBand][32]: banded taps of 32-phase tiles (MFMA resampler)
  unsigned int* d_hbandh = nullptr;  // [n_ptiles][2 planes][kRhChunks][64 lanes][8 fp16]: the same taps x 8 as fp16 hi / lo fragments
  int* d_lo = nullptr;       // [n_ptiles]: n_off of each tile's first phase
  int n_ptiles = 0;
  int stage_mask = 0;        // StageMask bits (debug / profiling / A-B runs)
  int rs_target_wgs = 256;   // persistent resampler: workgroups to aim for (one per CU; fewer leaves CUs to the other stream)
  // fused resample -> STFT kernel (mfcc_fused_kernel): frame groups of a clip of n_samp samples, {q0, f_begin, f_end, 0}
  int* d_groups = nullptr;
  int n_groups = 0;
  bool fused = false;         // the plan CAN run the fused kernel
  bool prefer_fused = false;  // ... and uses it for plain float32 batches too (lipasr_mfcc_plan_set key 2)
  float* d_hann = nullptr;
  float* d_tw = nullptr;  // float2 [2048]
  int* d_mel_start = nullptr;
  int* d_mel_len = nullptr;
  int* d_mel_off = nullptr;
  float* d_mel_w = nullptr;
  float* d_mel_wlo = nullptr;  // [1025] two-filters-per-bin form (mel_pairs)
  float* d_mel_whi = nullptr;
  int* d_mel_pstart = nullptr;  // [128]
  int* d_mel_plen = nullptr;
  float* d_dct = nullptr;  // DCT-II rows in MFMA fragment order: [32 rows (20 real)][k parity][64]
  float* d_y = nullptr;    // [batch_max][n_y]
  float* d_db = nullptr;   // [batch_max][n_frames][128]
  float* d_fmax = nullptr; // [batch_max][n_frames]
  // optional per-kernel HIP-event timing of lipasr_mfcc_f32 (bench.py's live roofline measurement): kProfEvents per
  // extraction.  The fused entry records all five; the split entries (lipasr_resample_f32 then lipasr_mfcc_from_22k, as the
  // phase-locked pipeline issues them) fill the same slot.
  std::vector<hipEvent_t> prof_events;
  int prof_cap = 0, prof_n = 0;
  bool prof_half = false;  // slot prof_n already holds a resample timing
  // block-DFT STFT on the matrix pipe (stft_bdft.hip): the default 2048/512 path; SM_STOCKHAM selects the Stockham
  // kernel stft_mel2_kernel instead (the parity reference)
  BdftTables bd;
  int bd_seg = 44;  // frames per workgroup (a multiple of 4; 44 = a whole 1-s clip)
  // the kernel's fused top_db + DCT epilogue (lipasr_mfcc_plan_set key 4): off by default -- measured on batches that are not
  // cache-warm it loses to the separate dct_kernel (STFT 139 + 5 us against 120 + 19 us per 1024 clips, round 4)
  bool bd_fuse_dct = false;
  // backward pass (plan_vjp in mfcc.hip, kernels in mfcc_vjp.hip): allocated at the first call, which sets vj_ready last
  bool vj_ready = false;
  float* d_gmel = nullptr;      // [batch_max][n_frames][128]
  float* d_part = nullptr;      // [batch_max][vj_groups][kVjSeg]
  float* d_gy = nullptr;        // [batch_max][n_y]
  float* d_dct_rows = nullptr;  // [20][128] plain DCT rows
  int* d_bin_run = nullptr;     // [1025]
  int vj_groups = 0;
  // the resampler's adjoint as a polyphase filter (lipasr_mfcc_plan_resample_vjp): allocated at the first call
  float* d_rt_taps = nullptr;   // [rt_nt][down]
  int* d_rt_t0 = nullptr;       // [down]
  int rt_nt = 0, rt_t0min = 0, rt_t0max = 0;
  // backward pass of the short-window path (lipasr_mfcc_plan_vjp_short, kernels in mfcc_vjp_short.hip): allocated at the same
  // first call, next to d_gmel / d_gy / d_dct_rows above; d_part then holds the workgroup images [workgroups][sv_seg]
  float* d_dft_t = nullptr;     // [dft_tiles*32 bins][dft_tiles*64]: d_dft with bins and samples exchanged
  int* d_melt_off = nullptr;    // [dft_tiles*32]: the mel bank by bin (the CSR bank transposed), filters in ascending order
  int* d_melt_len = nullptr;
  int* d_melt_m = nullptr;
  float* d_melt_w = nullptr;
};

// What one extraction runs.  pick_mfcc_path (mfcc.hip) is the ONE place that decides it; the launchers below take the kind and
// launch.  Precedence of the resamplers: fp16-plane -> persistent fp32 -> MFMA -> reg128 -> generic.
struct MfccPath {
  enum Resampler { RS_NONE, RS_H2, RS_PERSIST_F32, RS_MFMA, RS_REG128, RS_GENERIC, RS_COPY };
  enum Stft { ST_BDFT, ST_STOCKHAM4, ST_STOCKHAM2, ST_DFT };
  Resampler resampler = RS_NONE;  // of the three-kernel form (RS_NONE: it cannot read this input, or there is no input to resample)
  Stft stft = ST_BDFT;            // of the three-kernel form
  bool fused = false;             // mfcc_fused_kernel instead of both
  int rc = LIPASR_OK;             // LIPASR_EUNSUPPORTED (message set) when neither form can take the input
};
// wav: the rows at the plan's input rate (fmt 0 float32, 1 int16 PCM; ragged: with per-clip lengths), or null for a signal
// that is already at 22 050 Hz
MfccPath pick_mfcc_path(const MfccPlan* p, const void* wav, int fmt, bool ragged);

// Test hook (lipasr_debug_k1_launches): launches since load per K1 forward kernel instance, counted on the host where the launch
// happens.  The ids are part of the ABI (include/lipasr.h); K1_RESAMPLE_H2 + i is entry i of launch_resample's kerns[] table.
enum K1Kernel { K1_RESAMPLE_H2 = 0, K1_RESAMPLE_PERSIST = 4, K1_RESAMPLE_MFMA, K1_RESAMPLE_REG128, K1_RESAMPLE_GENERIC, K1_COPY_PAD,
                K1_CLEAR_TAIL, K1_STFT_BDFT, K1_STFT_BDFT_DCT, K1_STFT_MEL2, K1_STFT_MEL, K1_DFT_MEL, K1_DCT, K1_FUSED_F32, K1_FUSED_I16,
                K1_KERNELS };
extern long g_k1_launches[K1_KERNELS];  // mfcc.hip
// The same for the backward pass (lipasr_debug_k1_vjp_launches): one id per kernel instance of mfcc_vjp.h, mfcc_vjp.hip and
// mfcc_vjp_short.hip, in the order include/lipasr.h lists them.
enum K1VjpKernel { K1V_DB = 0, K1V_DB_RAGGED, K1V_STFT, K1V_STFT_RAGGED, K1V_FOLD, K1V_FOLD_RAGGED, K1V_RESAMPLE_Q8, K1V_RESAMPLE_Q1,
                   K1V_RESAMPLE_Q8_RAGGED, K1V_RESAMPLE_Q1_RAGGED, K1V_COPY_CUT, K1V_DFT, K1V_DFT_FOLD, K1V_KERNELS };
extern long g_k1_vjp_launches[K1V_KERNELS];  // mfcc.hip

// rows of n_samp samples can be read four at a time: float4 (fmt 0) / short4 (fmt 1) aligned, a multiple of 4 samples long
inline bool rows_vec4(const MfccPlan* p, const void* wav, int fmt) {
  return (reinterpret_cast<uintptr_t>(wav) & (fmt ? 7 : 15)) == 0 && (p->n_samp & 3) == 0;
}

// resample.hip
bool build_band_tables(const tables::Polyphase& pp, std::vector<float>* hb_out, std::vector<int>* lo_out);
std::vector<unsigned int> build_band_h2(const std::vector<float>& hb, const std::vector<int>& lo);
int launch_resample(const MfccPlan* p, MfccPath::Resampler kind, const void* wav, int fmt, const int* n_valid, int batch, float* y,
                    hipStream_t st);
// zeros from each clip's int(n ratio) to the end of its row of y (what the resamplers leave there with per-clip lengths is ringing)
int launch_clear_tail(const MfccPlan* p, const int* n_valid, int batch, float* y, hipStream_t st);
// stft_mel.hip.  launch_from_22k: STFT + mel + dB by `kind`, then the DCT; mid is recorded between the two; stft_only stops
// after the dB tile and the frame maxima (the backward pass re-running the forward; nothing is written to out)
std::vector<float> dct_fragments();
void fill_stft_args(const MfccPlan* p, const float* y, StftArgs* a);
int launch_dct(const MfccPlan* p, int batch, int L, const double* am, const double* as, float* out, const int* n_valid, hipStream_t st);
int launch_from_22k(const MfccPlan* p, MfccPath::Stft kind, const float* y, const int* n_valid, int batch, int L, const double* am,
                    const double* as, float* out, hipStream_t st, hipEvent_t mid = nullptr, bool stft_only = false);
// mfcc_vjp.hip: step 1 of the backward pass alone (DCT^T, top_db floor, dB -> mel into a.gmel), shared with the short-window chain
int launch_mfcc_vjp_db(const MfccVjpArgs& a, hipStream_t st);
// mfcc_vjp_short.hip: mel^T, |X|^2, STFT^T and overlap-add of the short-window path, then the adjoint of the reflect padding
struct ShortVjpArgs {
  const float* y;        // [batch][n_y] the 22 050 Hz signal the forward read
  const float* table;    // [k_rows][n_tiles*64] the forward's folded table
  const float* table_t;  // [n_tiles*32][n_tiles*64] the same weights, [bin][sample]
  const float* gmel;     // [batch][n_frames][128] d loss / d mel
  const int* melt_off;   // [n_tiles*32] the mel bank by bin
  const int* melt_len;
  const int* melt_m;
  const float* melt_w;
  int n_y, batch, hop, n_fft, k_rows, n_tiles, rpc, n_frames, total_rows, seg;
  float* part;           // [workgroups][seg] scratch: the overlap-added frame gradients of each workgroup's rows
  float* gy;             // [batch][n_y] out
};
// workgroups and image length for `batch` clips; the limits of the kernel (0 = fits, else the message is set)
int short_vjp_geometry(int n_fft, int hop, int rpc, int n_tiles, int batch, int* n_wgs, int* seg);
int launch_short_vjp(const ShortVjpArgs& a, hipStream_t st);
// mfcc_fused.hip
std::vector<int> build_groups(int n_y, int n_frames, int up);
int launch_fused(const MfccPlan* p, const void* wav, int fmt, const int* n_valid, int batch, hipStream_t st);

}  // namespace lipasr
