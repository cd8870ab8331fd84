// K1 stages 1 + 2 in one kernel (mfcc_fused_kernel), its frame-group table (build_groups) and its launcher.  Not the default:
// pick_mfcc_path (mfcc.hip) takes it where the three-kernel path cannot read the input (int16 PCM or per-clip lengths in rows
// that are not a multiple of 4 samples long) or where the plan asks for it (lipasr_mfcc_plan_set key 2); dct_kernel follows.
#include "mfcc_plan.h"

namespace lipasr {

using namespace tables;

// ---------------------------------------------------------------------------------------------
// stages 1 + 2 fused: the resampled signal never leaves the CU.
//
//   One workgroup = (clip, frame group).  A frame group is a run of STFT frames whose reflect-padded windows lie
//   inside 16 consecutive q-blocks of the resampled clip (16 x 441 = 7056 samples; a 1-s clip has the four groups
//   12 | 10 | 10 | 12 frames, built on the host by build_groups()).  The workgroup
//     1. stages the input samples of its 16 q-blocks in LDS (float4 / short4 loads; int16 PCM is scaled by 2^-15 here,
//        which is librosa.load's decode; samples outside [0, n_valid) are zero = resampy's tap-count clamps),
//     2. resamples them with the polyphase contraction of resample_mfma_kernel on v_mfma_f32_16x16x4_f32 -- rows are
//        the 16 q-blocks of ONE clip (A operand from LDS: row stride down + 2 floats, so the 16 rows x 2 k-columns of a
//        half-wave hit 32 different banks), columns 2 x 16 phases sharing one A read, K = the 152-sample band -- and
//        writes the 7056 resampled samples to a second LDS region (fix_length zeros past int(n * ratio)),
//     3. runs the frame pairs of its group as complex 2048-point FFTs straight from that region (the code of
//        stft_mel_kernel; the x staging area becomes the FFT buffer), with the Hann weights, all radix-8 / radix-4
//        twiddles and the mel-stage constants of each thread loaded ONCE per workgroup instead of once per frame pair.
//   HBM traffic of the stage drops from 4.5x to about 1.4x the algorithmic bytes (the resampled signal's 88 kB per clip
//   written and 89 kB read back are gone; the 16-q windows of neighbouring groups overlap by ~30 %, served from L2).
//   The MFMA pipe (resampling) and the VALU (FFT butterflies) belong to different phases of a workgroup; with three
//   workgroups per CU in different phases the two pipes overlap.
//   Clips of different lengths in one launch: n_valid[u] samples of clip u are real, the rest of its row is ignored;
//   lengths, frame count and the reflect padding follow the clip's own length (the group table is the one of the
//   longest clip: frames a shorter clip does not have are skipped).
// ---------------------------------------------------------------------------------------------
constexpr int kFuYLds = kFuQ * kFuUp + 8;                   // resampled span (floats)
constexpr int kFuXMax = kFuQ * 320 + 160;                   // staged input samples at down = 320 (last row's band end)
constexpr int kFuXLds = kFuXMax + 2 * (kFuXMax / 160) + 6;  // + 2 pad floats per q-block (down >= 160)
constexpr int kFuULds = (kFuXLds > 2 * kFftLds ? kFuXLds : 2 * kFftLds);  // union: x staging | FFT buffer
constexpr int kFuLdsFloats = kFuYLds + kFuULds + 2 * 2 * 128 + 8;
typedef float fu_f32x4 __attribute__((ext_vector_type(4)));

struct FusedArgs {
  const void* wav;     // [batch][row_stride] float32 or int16
  long row_stride;     // samples between clips
  int n_samp_max;      // samples per row that may be valid
  const int* n_valid;  // [batch] or null (= n_samp_max everywhere)
  int sr_in, down;
  int vec;             // rows are 16-byte (f32) / 8-byte (i16) aligned: vector loads
  const float* Hband;  // [n_ptiles][kRsBand][32]
  const int* lo;       // [n_ptiles]
  int n_ptiles;
  const int4* groups;
  int n_groups;
  StftArgs st;         // n_y / n_frames of the LONGEST clip: strides of db / fmax
};

template <bool I16>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void mfcc_fused_kernel(FusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fl[];
  float* ys = fl;                     // resampled span
  float* xs = fl + kFuYLds;           // input staging, later the FFT buffer
  float2* buf = reinterpret_cast<float2*>(xs);
  float2* rsum = reinterpret_cast<float2*>(fl + kFuYLds + kFuULds);  // [2][128]
  float* wmax = fl + kFuYLds + kFuULds + 2 * 2 * 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware block -> (clip, group) map (speed only): the groups of one clip go to one XCD, whose L2 then serves
  // the ~30 % of input samples neighbouring groups share
  int u, g;
  {
    const int ng = gridDim.x, L = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.y;
    const int full = (nb / 8) * 8 * ng;
    if (L < full) {
      const int chunk = L >> 3;
      u = (chunk / ng) * 8 + (L & 7);
      g = chunk % ng;
    } else {
      u = blockIdx.y;
      g = blockIdx.x;
    }
  }
  int n = a.n_samp_max;
  if (a.n_valid) n = min(max(a.n_valid[u], 0), a.n_samp_max);
  int n_vy, n_y, n_frames;
  clip_lengths(n, a.sr_in, &n_vy, &n_y, &n_frames);
  const int4 G = a.groups[g];
  const int q0 = G.x, fb = G.y, fe = min(G.z, n_frames);
  if (fb >= fe) return;  // this clip has no frame in the group (workgroup-uniform)
  const int down = a.down;
  // ---- 1. stage the input: element i of the staging area = sample xbase + i, stored at i + 2 (i / down)
  {
    const int xbase = down * q0 - 64;
    const int x_count = kFuQ * down + 160;
    const size_t row = (size_t)u * a.row_stride;
    for (int v = tid; v < x_count / 4; v += 256) {
      const int i4 = 4 * v, sidx = xbase + i4;
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
      if (a.vec && sidx >= 0 && sidx + 3 < n) {
        if (I16) {
          const short4 t = *reinterpret_cast<const short4*>(static_cast<const short*>(a.wav) + row + sidx);
          e0 = (float)t.x * (1.0f / 32768.0f); e1 = (float)t.y * (1.0f / 32768.0f);
          e2 = (float)t.z * (1.0f / 32768.0f); e3 = (float)t.w * (1.0f / 32768.0f);
        } else {
          const float4 t = *reinterpret_cast<const float4*>(static_cast<const float*>(a.wav) + row + sidx);
          e0 = t.x; e1 = t.y; e2 = t.z; e3 = t.w;
        }
      } else if (sidx + 3 >= 0 && sidx < n) {
        float e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int sc = sidx + c;
          e[c] = 0.f;
          if (sc >= 0 && sc < n)
            e[c] = I16 ? (float)static_cast<const short*>(a.wav)[row + sc] * (1.0f / 32768.0f) : static_cast<const float*>(a.wav)[row + sc];
        }
        e0 = e[0]; e1 = e[1]; e2 = e[2]; e3 = e[3];
      }
      float* d = xs + i4 + 2 * (i4 / down);  // 8-byte aligned: two ds_write_b64
      *reinterpret_cast<float2*>(d) = make_float2(e0, e1);
      *reinterpret_cast<float2*>(d + 2) = make_float2(e2, e3);
    }
  }
  __syncthreads();
  // ---- 2. polyphase resampling on the matrix cores: Y[q-block i][phase] = X_i[band] . Hband
  {
    const int ir = lane & 15, kk = lane >> 4;
    const float* xrow = xs + (down + 2) * ir;
    for (int r = wave; r < ((a.st.stage_mask & SM_FUSED_SKIP_RESAMPLE) ? 0 : a.n_ptiles); r += 4) {  // (profiling, skips the resampling)
      const int lo_r = a.lo[r];
      const float* hb = a.Hband + (size_t)r * kRsBand * 32 + kk * 32 + ir;
      float b0[kRsBand / 4], b1[kRsBand / 4];
#pragma unroll
      for (int s2 = 0; s2 < kRsBand / 4; ++s2) {
        b0[s2] = hb[s2 * 128];
        b1[s2] = hb[s2 * 128 + 16];
      }
      const int t0 = lo_r + 1 + kk;
      const float* pa = xrow + t0;
      const int cross = down - t0;  // band position t0 + 4 s lies in the next q-block's 320 samples once 4 s >= cross
      fu_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s2 = 0; s2 < kRsBand / 4; ++s2) {
        const float av = pa[4 * s2 + ((4 * s2 >= cross) ? 2 : 0)];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0[s2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1[s2], acc1, 0, 0, 0);
      }
      // C layout: column (phase) = lane & 15, row (q-block) = 4 (lane >> 4) + e
#pragma unroll
      for (int jh = 0; jh < 2; ++jh) {
        const int ph = 32 * r + 16 * jh + ir;
        if (ph < kFuUp) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int rw = 4 * kk + e;
            const int t = kFuUp * (q0 + rw) + ph;
            const float val = jh ? acc1[e] : acc0[e];
            ys[kFuUp * rw + ph] = (t < n_vy) ? val : 0.0f;
          }
        }
      }
    }
  }
  __syncthreads();
  if (a.st.stage_mask & SM_FUSED_STOP) return;  // (profiling, stops before the frames)
  // ---- 3. the frame pairs of the group, from LDS
  const StftArgs& st = a.st;
  const int ybase = kFuUp * q0;
  // per-thread constants, once per workgroup: Hann weights, twiddles of passes 2-4, mel weights and runs
  float hw[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) hw[e] = st.hann[tid + 256 * e];
  cpx w3[7];
  load_tw<8>(st.tw, tid, 64, w3);
  const int mel_part = (tid >> 6) & 1, mel_run = ((tid >> 7) << 6) + (tid & 63);
  const int mst = st.mel_start[mel_run], mln = st.mel_len[mel_run];
  float mwl[5], mwh[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int k = tid + 256 * i;
    mwl[i] = (k <= 1024) ? st.mel_wlo[k] : 0.0f;
    mwh[i] = (k <= 1024) ? st.mel_whi[k] : 0.0f;
  }
  for (int f0 = fb; f0 < fe; f0 += 2) {
    const int f1 = f0 + 1;
    const bool has1 = f1 < fe;  // fe <= n_frames; a pair never straddles two groups (groups hold whole pairs)
    // The thread index is made opaque inside the loop: every LDS address of the five passes depends on it alone, and
    // hoisted out of the loop as invariants those ~90 addresses would push the per-thread tables into scratch.
    int tq = tid;
    asm volatile("" : "+v"(tq));
    // (the twiddles of passes 2 and 4 are fetched per pair, from the L2-resident table, at the top of the iteration: keeping them
    // resident as well pushed 15 registers per lane into scratch -- 63 MB of scratch traffic per 1024 clips)
    cpx w2[7], w4a[3], w4b[3];
    load_tw<8>(st.tw, tq, 8, w2);
    load_tw<4>(st.tw, tq, 512, w4a);
    load_tw<4>(st.tw, tq + 256, 512, w4b);
    cpx x0[8];
    if (has1 && f0 >= 2 && f1 * 512 + 1024 <= n_y) {
      const float* p = ys + (f0 * 512 - 1024 - ybase) + tq;
      float sm[10];
#pragma unroll
      for (int e = 0; e < 10; ++e) sm[e] = p[256 * e];
#pragma unroll
      for (int e = 0; e < 8; ++e) x0[e] = {hw[e] * sm[e], hw[e] * sm[e + 2]};
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j0 = f0 * 512 + tq + 256 * e - 1024;
        const float s0 = ys[reflect_index(j0, n_y) - ybase];
        const float s1 = has1 ? ys[reflect_index(j0 + 512, n_y) - ybase] : 0.0f;
        x0[e] = {hw[e] * s0, hw[e] * s1};
      }
    }
    {
      const cpx none7[7] = {};
      fft_pass_regs<8>(buf, 1, tq, none7, x0);
      lds_barrier();
      fft_pass_regs<8>(buf, 8, tq, w2, nullptr);
      lds_barrier();
      fft_pass_regs<8>(buf, 64, tq, w3, nullptr);
      lds_barrier();
      // radix 4, two butterflies per thread: both read, the workgroup meets, both write
      cpx va[4], vb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float2 ta = buf[padi(tq + r * 512)], tb = buf[padi(tq + 256 + r * 512)];
        va[r] = {ta.x, ta.y};
        vb[r] = {tb.x, tb.y};
      }
      lds_barrier();
#pragma unroll
      for (int r = 1; r < 4; ++r) { va[r] = cmul(va[r], w4a[r - 1]); vb[r] = cmul(vb[r], w4b[r - 1]); }
      dft4(va);
      dft4(vb);
      // Ns = 512: k = j, output index j + r 512
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        buf[padi(tq + r * 512)] = make_float2(va[r].re, va[r].im);
        buf[padi(tq + 256 + r * 512)] = make_float2(vb[r].re, vb[r].im);
      }
      lds_barrier();
    }
    float2 zz[5], zc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tq + 256 * i;
      if (k <= 1024) {
        zz[i] = buf[padi(k)];
        zc[i] = buf[padi((2048 - k) & 2047)];
      }
    }
    lds_barrier();
    float2* T = buf;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int k = tq + 256 * i;
      if (k <= 1024) {
        const float zr = zz[i].x, zi = zz[i].y, wr = zc[i].x, wi = -zc[i].y;
        const float x0r = 0.5f * (zr + wr), x0i = 0.5f * (zi + wi);
        const float x1r = 0.5f * (zi - wi), x1i = -0.5f * (zr - wr);
        const float p0 = x0r * x0r + x0i * x0i, p1 = x1r * x1r + x1i * x1i;
        T[k] = make_float2(mwl[i] * p0, mwl[i] * p1);
        T[kTPair + k] = make_float2(mwh[i] * p0, mwh[i] * p1);
      }
    }
    lds_barrier();
    const int sel = tq >> 7, m = tq & 127;
    {
      const float2* Tp = T + mel_part * kTPair + mst;
      float2 a0 = make_float2(0.0f, 0.0f), a1 = a0, a2 = a0, a3 = a0;
      int i = 0;
      for (; i + 4 <= mln; i += 4) {
        const float2 v0 = Tp[i], v1 = Tp[i + 1], v2 = Tp[i + 2], v3 = Tp[i + 3];
        a0.x += v0.x; a0.y += v0.y; a1.x += v1.x; a1.y += v1.y;
        a2.x += v2.x; a2.y += v2.y; a3.x += v3.x; a3.y += v3.y;
      }
      for (; i < mln; ++i) { const float2 v = Tp[i]; a0.x += v.x; a0.y += v.y; }
      rsum[mel_part * 128 + mel_run] = make_float2((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y));
    }
    lds_barrier();
    const float* rs = reinterpret_cast<const float*>(rsum);
    const float sacc = rs[2 * m + sel] + ((m > 0) ? rs[2 * (128 + m - 1) + sel] : 0.0f);
    const float dbv = power_to_db(sacc);  // librosa.power_to_db(ref=1, amin=1e-10)
    const int f = sel ? f1 : f0;
    if (f < fe) st.db[((size_t)u * st.n_frames + f) * 128 + m] = dbv;
    const float wm = wave_max(dbv);
    if (lane == 0) wmax[tq >> 6] = wm;
    lds_barrier();
    if (tq == 0) st.fmax[(size_t)u * st.n_frames + f0] = fmaxf(wmax[0], wmax[1]);
    if (tq == 128 && has1) st.fmax[(size_t)u * st.n_frames + f1] = fmaxf(wmax[2], wmax[3]);
  }
}

// Frame groups of a clip with n_y resampled samples and n_frames frames for mfcc_fused_kernel: runs of whole frame
// pairs whose reflect-padded windows (plus one sample of slack below: a SHORTER clip in the same launch reflects around
// its own end and may touch one sample before the window) lie inside kFuQ q-blocks starting at q0.
std::vector<int> build_groups(int n_y, int n_frames, int up) {
  std::vector<int> g;
  int f = 0;
  while (f < n_frames) {
    const int lo = std::max(0, kHop * f - kNFft / 2 - 1);
    const int q0 = lo / up;
    int fe = f;
    while (fe < n_frames) {
      const int cand = std::min(fe + 2, n_frames);
      const int hi = std::min(n_y, kHop * (cand - 1) + kNFft / 2);  // one past the last sample the frames need
      if ((hi + up - 1) / up - q0 > kFuQ) break;
      fe = cand;
    }
    if (fe == f) return std::vector<int>();  // a single pair does not fit: never with 2048/512 and up = 441
    g.push_back(q0); g.push_back(f); g.push_back(fe); g.push_back(0);
    f = fe;
  }
  return g;
}

// stages 1 + 2 in one kernel (mfcc_fused_kernel); wav: float32 (fmt 0) or int16 PCM (fmt 1)
int launch_fused(const MfccPlan* p, const void* wav, int fmt, const int* n_valid, int batch, hipStream_t st) {
  FusedArgs a;
  a.wav = wav; a.row_stride = p->n_samp; a.n_samp_max = p->n_samp; a.n_valid = n_valid;
  a.sr_in = p->sr_in; a.down = p->down;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(wav);
  a.vec = (addr & (fmt ? 7 : 15)) == 0 && (p->n_samp & 3) == 0;  // (speed only: the kernel reads any rows)
  a.Hband = p->d_hband; a.lo = p->d_lo; a.n_ptiles = p->n_ptiles;
  a.groups = reinterpret_cast<const int4*>(p->d_groups); a.n_groups = p->n_groups;
  fill_stft_args(p, nullptr, &a.st);
  const size_t lds = (size_t)kFuLdsFloats * sizeof(float);
  if (fmt) {
    LP_DYN_LDS(mfcc_fused_kernel<true>, lds);
    hipLaunchKernelGGL(mfcc_fused_kernel<true>, dim3(p->n_groups, batch), dim3(256), lds, st, a);
    ++g_k1_launches[K1_FUSED_I16];
  } else {
    LP_DYN_LDS(mfcc_fused_kernel<false>, lds);
    hipLaunchKernelGGL(mfcc_fused_kernel<false>, dim3(p->n_groups, batch), dim3(256), lds, st, a);
    ++g_k1_launches[K1_FUSED_F32];
  }
  LP_LAUNCH_CHECK();
  return LIPASR_OK;
}

}  // namespace lipasr
