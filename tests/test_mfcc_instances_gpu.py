"""Every kernel instance of the MFCC forward pass (K1) stage by stage against float64, and proof of which kernels ran.

Every case goes through the raw C entry points with ctypes, so that pointers, alignment and batch sizes are the test's:

  * memory: every user-visible device array (the wav rows, y, out, the destinations of lipasr_debug_mfcc_stage) lives in a buffer of
    its own between at least 8 sentinel floats (16 sentinel samples for int16 rows); an "off" array starts one float off a 16-byte
    boundary (int16 rows: one sample off 8 bytes).  Plans are made with batch_max larger than the batch of the call, so rows >= batch
    of y, out and the hook's destinations hold sentinels too.  All sentinels must survive.
  * kernels: every case names the counters of lipasr_debug_k1_launches it must move and by how much, written out by hand from
    pick_mfcc_path and the launchers; exactly those counters must move by exactly those amounts.  The last test fails when the library
    knows an id that no case claims, and prints (-s) per kernel the first case that showed it running and its worst error.
  * determinism: each case runs twice from the same inputs into fresh buffers; the outputs are bit-identical.
  * header promises, as bits: int16 rows = float32 rows of pcm 2^-15; a clip in a ragged launch = a plan of its own length running it
    alone (where the same kernel serves both); stft_bdft_kernel's DCT epilogue = dct_kernel; lipasr_mfcc_plan_resample_ragged followed
    by _from_22k_ragged = lipasr_mfcc_extract with n_valid.

Stage A (resamplers): oracle.mfcc_ref.librosa_load_resample in float64, bound 2e-6 max|x| of the clip per sample (the 2e-6 of the
existing resampler tests at full scale, their relative form for quiet clips).  Stage B (STFT + mel + dB, read with
lipasr_debug_mfcc_stage) and stage C (dct_kernel): metric, yardstick and bounds of tests/mfcc_stage_ref.py; the CPU companion
test_mfcc_instances_cpu.py shows that those bounds tell wrong kernels from right ones.  Every case also keeps the end-to-end statement
of test_mfcc_gpu.py: features within ATOL = 2e-2 of the oracle.

Where the case tables differ from a naive reading of the kernels' names: int16 rows of one length reach the resampler through
lipasr_mfcc_extract only (lipasr_mfcc_plan_resample takes float32), so that case reads y with the hook; the 45-frame cases of the DCT
epilogue set plan key 3 to 48 (the epilogue needs one workgroup per clip, and 44 frames per workgroup leave a 45th to a second one); a
clip of one input sample has no plan of its own (plans need 2), so the one-frame ragged clip has 2 samples; batches hold the five
stage-B clips, 5 of a batch_max of 6.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mfcc_stage_ref as S
from oracle import mfcc_ref as M

pytestmark = pytest.mark.gpu
ATOL = 2e-2
GUARD = 8
SENTINEL = -12345.0

# kernel ids of lipasr_debug_k1_launches (include/lipasr.h)
(H2_F32, H2_I16, H2_F32_RAGGED, H2_I16_RAGGED, PERSIST, MFMA, REG128, GENERIC, COPY, CLEAR_TAIL, BDFT, BDFT_DCT, MEL2, MEL, DFT, DCT, FUSED_F32,
 FUSED_I16) = range(18)
K1_NAMES = ("resample_persist_h2_kernel<float32>", "resample_persist_h2_kernel<int16>", "resample_persist_h2_kernel<float32, ragged>",
            "resample_persist_h2_kernel<int16, ragged>", "resample_persist_kernel", "resample_mfma_kernel", "resample_reg128_kernel",
            "resample_generic_kernel", "copy_pad_kernel", "clear_tail_kernel", "stft_bdft_kernel", "stft_bdft_kernel + DCT epilogue",
            "stft_mel2_kernel", "stft_mel_kernel", "dft_mel_kernel", "dct_kernel", "mfcc_fused_kernel<float32>", "mfcc_fused_kernel<int16>")

_ran = {}    # kernel id -> the first case whose counter assertion showed it running
_worst = {}  # kernel id -> (worst error of a case that ran it, as a fraction of its bound, that case, device-to-yardstick ratio or None)
_bits = {}   # outputs that a later case compares with (reports only)


def _native():
    from lipasr import _native as N

    return N


def _snapshot():
    lib = _native().lib
    return [lib.lipasr_debug_k1_launches(k) for k in range(len(K1_NAMES))]


def _assert_moved(before, expect, what):
    moved = {k: a - b for k, (b, a) in enumerate(zip(before, _snapshot())) if a != b}
    names = lambda d: {K1_NAMES[k]: v for k, v in d.items()}
    assert moved == expect, f"{what}: launched {names(moved)}, the case is meant to launch {names(expect)}"


def _record(case_id, kernels, frac, ratio=None):
    for k in kernels:
        _ran.setdefault(k, case_id)
        if k not in _worst or frac > _worst[k][0]:
            _worst[k] = (frac, case_id, ratio)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Buf:
    """One array between sentinels in a device buffer of its own: [>= 8 sentinel floats] array [>= 8 sentinel floats].  dtype float32 or
    int16 (16 sentinel samples); off: the array starts one element past a 16-byte (int16: 8-byte) boundary."""

    def __init__(self, shape, data=None, off=False, dtype=np.float32):
        self.shape, self.n, self.dtype = tuple(shape), int(np.prod(shape)), dtype
        guard = GUARD * (4 // np.dtype(dtype).itemsize)
        self.start = guard + (1 if off else 0)
        host = np.full(self.start + self.n + guard, SENTINEL, dtype)
        if data is not None:
            host[self.start:self.start + self.n] = np.asarray(data, dtype).ravel()
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        align = 16 if dtype == np.float32 else 8
        assert (self.ptr().value % align == 0) != off

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.start * np.dtype(self.dtype).itemsize)

    def read(self, rows=None):
        """The array back on the host; asserts that no sentinel was touched, and (rows given) that rows >= rows still hold sentinels."""
        host = self.t.cpu().numpy()
        s = host.dtype.type(SENTINEL)
        assert (host[:self.start] == s).all(), "sentinels before the array were written"
        assert (host[self.start + self.n:] == s).all(), "sentinels after the array were written"
        a = host[self.start:self.start + self.n].reshape(self.shape).copy()
        if rows is not None:
            assert (a[rows:] == s).all(), f"rows >= batch ({rows}) were written"
            a = a[:rows]
        return a


class Plan:
    def __init__(self, sr, n, batch_max, n_fft=2048, hop=512, keys=()):
        N = _native()
        self.h = N.c_h()
        N.check(N.lib.lipasr_mfcc_create(N.get_handle(0).h, sr, n, batch_max, n_fft, hop, C.byref(self.h)))
        ny, nf, fu = C.c_int(), C.c_int(), C.c_int()
        N.check(N.lib.lipasr_mfcc_plan_dims(self.h, C.byref(ny), C.byref(nf), C.byref(fu)))
        self.sr, self.n, self.batch_max, self.n_y, self.n_frames, self.fused = sr, n, batch_max, ny.value, nf.value, fu.value
        self.n_fft, self.mask = n_fft, 0
        for k, v in keys:
            self.set(k, v)
        self.scrub()

    def scrub(self):
        """One forward call on other rows, so that the plan's dB tile and frame maxima hold WRONG values before a case runs: device
        memory that a destroyed plan of the same shape left behind may hold the right ones, and a kernel that skipped a frame would
        then pass.  On a 2048/512 plan ANOTHER STFT kernel than the case's writes them (stft_mel2_kernel, or stft_bdft_kernel for the
        cases of stft_mel2_kernel): a kernel that skips a frame skips it in its own scrub too.  (Not part of any case's counter
        window.)"""
        N = _native()
        mask = self.mask
        if self.n_fft == 2048:
            self.set(0, 0 if mask & 256 else 256)
        rng = np.random.default_rng(9)
        y = Buf((self.batch_max, self.n_y), 0.37 * rng.uniform(-1.0, 1.0, (self.batch_max, self.n_y)))
        out = Buf((self.batch_max, 20))
        N.check(N.lib.lipasr_mfcc_plan_from_22k(self.h, y.ptr(), self.batch_max, self.n_y, 1, None, None, out.ptr(), N.stream_ptr()))
        torch.cuda.synchronize()
        if self.n_fft == 2048:
            self.set(0, mask)

    def set(self, k, v):
        N = _native()
        if k == 0:
            self.mask = v
        N.check(N.lib.lipasr_mfcc_plan_set(self.h, k, v))

    def close(self):
        if self.h:
            N = _native()
            torch.cuda.synchronize()
            N.check(N.lib.lipasr_mfcc_destroy(self.h))
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stage(self, which, batch):
        """lipasr_debug_mfcc_stage into a guarded destination laid out for batch_max rows"""
        N = _native()
        shape = {0: (self.batch_max, self.n_frames, 128), 1: (self.batch_max, self.n_frames), 2: (self.batch_max, self.n_y)}[which]
        dst = Buf(shape)
        N.check(N.lib.lipasr_debug_mfcc_stage(self.h, which, batch, dst.ptr(), N.stream_ptr()))
        torch.cuda.synchronize()
        return dst.read(batch)


def _nv(values):
    return None if values is None else torch.as_tensor(np.asarray(values, np.int32)).cuda()


def _affine(L, seed=0):
    rng = np.random.default_rng(300 + seed)
    return rng.standard_normal(20 * L), rng.uniform(0.5, 2.0, 20 * L) * np.where(rng.random(20 * L) < 0.25, -1.0, 1.0)


def _dev64(a):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float64)).cuda()


def _clip_lengths(n, sr):
    """resampled samples, samples after fix_length and frames of a clip of n samples at sr (include/lipasr.h, lipasr_mfcc_plan_vjp_ragged)"""
    v = n * (float(M.SR_TARGET) / float(sr))
    n_y = int(np.ceil(v))
    return int(v), n_y, (1 + n_y // M.HOP if n_y >= 2 else 0)


# ====================================================================================================== stage A: the resamplers
RAGGED_NV = (1600, 1599, 803, 4, 1, 0, 1600)
# id: (sr, rows, batch, batch_max, sample format, n_valid, stage mask, plan key 1, wav off, y off, entry, counters)
A_CASES = {
    "h2-f32": (16000, 1600, 33, 40, 0, None, 0, None, False, False, "resample", {H2_F32: 1}),
    "h2-f32-short-last-qblock": (16000, 1604, 33, 40, 0, None, 0, None, False, False, "resample", {H2_F32: 1}),
    "h2-f32-8k": (8000, 800, 33, 40, 0, None, 0, None, False, False, "resample", {H2_F32: 1}),
    "h2-f32-3-workgroups": (16000, 1600, 33, 40, 0, None, 0, 3, False, False, "resample", {H2_F32: 1}),
    "h2-i16": (16000, 1600, 33, 40, 1, None, 0, None, False, False, "extract", {H2_I16: 1, BDFT: 1, DCT: 1}),
    "h2-f32-ragged": (16000, 1600, 7, 8, 0, RAGGED_NV, 0, None, False, False, "resample_ragged", {H2_F32_RAGGED: 1, CLEAR_TAIL: 1}),
    "h2-i16-ragged": (16000, 1600, 7, 8, 1, RAGGED_NV, 0, None, False, False, "resample_ragged", {H2_I16_RAGGED: 1, CLEAR_TAIL: 1}),
    "persist-1600": (16000, 1600, 33, 40, 0, None, 16, None, False, False, "resample", {PERSIST: 1}),
    "persist-1604": (16000, 1604, 33, 40, 0, None, 16, None, False, False, "resample", {PERSIST: 1}),
    "mfma-1602": (16000, 1602, 33, 40, 0, None, 0, None, False, False, "resample", {MFMA: 1}),
    "mfma-1600-wav-off": (16000, 1600, 33, 40, 0, None, 0, None, True, False, "resample", {MFMA: 1}),
    "mfma-12k": (12000, 1200, 33, 40, 0, None, 0, None, False, False, "resample", {MFMA: 1}),
    "reg128-1600": (16000, 1600, 33, 40, 0, None, 4, None, False, False, "resample", {REG128: 1}),
    "reg128-13-qblocks": (16000, 4000, 3, 4, 0, None, 4, None, False, False, "resample", {REG128: 1}),  # 13 q-blocks: a workgroup of 10, one of 3
    "generic-44100": (44100, 4410, 3, 4, 0, None, 0, None, False, False, "resample", {GENERIC: 1}),     # down-sampling, 256 taps
    "generic-22005": (22005, 2200, 3, 4, 0, None, 0, None, False, False, "resample", {GENERIC: 1}),     # 490 phases of 128 taps
    "copy": (22050, 2205, 3, 4, 0, None, 0, None, False, False, "resample", {COPY: 1}),
    "copy-off": (22050, 2205, 3, 4, 0, None, 0, None, True, True, "resample", {COPY: 1}),
}


@functools.lru_cache(maxsize=None)
def _a_rows(sr, n, batch, fmt, nv):
    """Rows and their float64 reference: full-scale uniform noise, row 1 scaled by 1e-3, row 2 all zero; with n_valid, garbage past each
    clip's end.  Returns (what the device reads, the float32 clips, ref [batch][n_y] float64 with zeros from int(n r) on)."""
    rng = np.random.default_rng(sr + 7 * n + batch)
    x = rng.uniform(-1.0, 1.0, (batch, n))
    x[1] *= 1e-3
    x[2] = 0.0
    if fmt:
        dev = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
        x = (dev.astype(np.float32) / 32768.0).astype(np.float32)
    else:
        x = x.astype(np.float32)
        dev = x.copy()
    n_y = _clip_lengths(n, sr)[1]
    ref = np.zeros((batch, n_y))
    for u in range(batch):
        nu = n if nv is None else nv[u]
        if nu > 0:
            r = M.librosa_load_resample(x[u, :nu], sr, dtype=np.float64)
            ref[u, :len(r)] = r
        if nu < n:
            dev[u, nu:] = (rng.integers(-30000, 30000, n - nu) if fmt else rng.standard_normal(n - nu)).astype(dev.dtype)
    return dev, x, ref


@pytest.mark.parametrize("case", list(A_CASES))
def test_stage_a_resamplers(cuda, case):
    N = _native()
    sr, n, batch, bmax, fmt, nv, mask, key1, wav_off, y_off, entry, expect = A_CASES[case]
    dev_rows, x, ref = _a_rows(sr, n, batch, fmt, nv)
    keys = [(0, mask)] + ([(1, key1)] if key1 else [])
    L = 6
    with Plan(sr, n, bmax, keys=keys) as plan:
        assert ref.shape[1] == plan.n_y
        runs = []
        for rep in range(2):
            wav = Buf(dev_rows.shape, dev_rows, wav_off, np.int16 if fmt else np.float32)
            y = Buf((bmax, plan.n_y), None, y_off)
            out = Buf((bmax, 20 * L))
            nvt = _nv(nv)
            before = _snapshot()
            if entry == "resample":
                N.check(N.lib.lipasr_mfcc_plan_resample(plan.h, wav.ptr(), batch, y.ptr(), N.stream_ptr()))
            elif entry == "resample_ragged":
                N.check(N.lib.lipasr_mfcc_plan_resample_ragged(plan.h, wav.ptr(), fmt, N.ptr(nvt), batch, y.ptr(), N.stream_ptr()))
            else:  # int16 rows of one length reach the resampler through the whole extraction only: y is read with the hook
                N.check(N.lib.lipasr_mfcc_extract(plan.h, wav.ptr(), fmt, None, batch, L, None, None, out.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            _assert_moved(before, expect, case)
            wav.read()
            runs.append(plan.stage(2, batch) if entry == "extract" else y.read(batch))
        assert _same_bits(runs[0], runs[1]), "two runs from the same inputs differ"
        got = runs[0]
        # the end-to-end statement, on the same plan: the features of these rows against the oracle
        wav = Buf(dev_rows.shape, dev_rows, wav_off, np.int16 if fmt else np.float32)
        out = Buf((bmax, 20 * L))
        nvt = _nv(nv)
        N.check(N.lib.lipasr_mfcc_extract(plan.h, wav.ptr(), fmt, N.ptr(nvt), batch, L, None, None, out.ptr(), N.stream_ptr()))
        torch.cuda.synchronize()
        feats = out.read(batch)
        if entry == "extract":  # int16 rows equal float32 rows of pcm 2^-15, bit for bit (same kernel family: id 0 instead of id 1)
            wf = Buf(x.shape, x)
            of = Buf((bmax, 20 * L))
            before = _snapshot()
            N.check(N.lib.lipasr_mfcc_extract(plan.h, wf.ptr(), 0, None, batch, L, None, None, of.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            _assert_moved(before, {H2_F32: 1, BDFT: 1, DCT: 1}, case + " (float32 twin)")
            assert _same_bits(plan.stage(2, batch), got) and _same_bits(of.read(batch), feats)
        if entry == "resample_ragged":  # resample_ragged then from_22k_ragged = extract with n_valid, bit for bit
            yb = Buf((bmax, plan.n_y), np.concatenate([got, np.full((bmax - batch, plan.n_y), SENTINEL, np.float32)]))
            o2 = Buf((bmax, 20 * L))
            N.check(N.lib.lipasr_mfcc_plan_from_22k_ragged(plan.h, yb.ptr(), N.ptr(nvt), batch, L, None, None, o2.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            assert _same_bits(o2.read(batch), feats)
            if fmt:  # int16 rows equal float32 rows of pcm 2^-15 on the ragged instances too (id 3 against id 2)
                fdev = dev_rows.astype(np.float32) / 32768.0
                wf = Buf(fdev.shape, fdev)
                yf = Buf((bmax, plan.n_y))
                before = _snapshot()
                N.check(N.lib.lipasr_mfcc_plan_resample_ragged(plan.h, wf.ptr(), 0, N.ptr(nvt), batch, yf.ptr(), N.stream_ptr()))
                torch.cuda.synchronize()
                _assert_moved(before, {H2_F32_RAGGED: 1, CLEAR_TAIL: 1}, case + " (float32 twin)")
                assert _same_bits(yf.read(batch), got)
    worst = 0.0
    for u in range(batch):
        nu = n if nv is None else nv[u]
        n_vy = _clip_lengths(nu, sr)[0]
        peak = float(np.abs(x[u, :nu]).max()) if nu else 0.0
        err = float(np.abs(got[u] - ref[u]).max())
        assert err <= 2e-6 * peak, f"{case}: clip {u} ({nu} samples, peak {peak:.1e}) is {err:.2e} from the float64 oracle, bound {2e-6 * peak:.2e}"
        if peak == 0.0:
            assert not got[u].any()  # the all-zero clip gives exactly 0
        else:
            worst = max(worst, err / (2e-6 * peak))
        assert not got[u, n_vy:].any(), f"{case}: clip {u} is not exactly 0 from int(n r) = {n_vy} on (the appended zero, the rest of a ragged row)"
        if nu >= 1:  # (one sample resamples to ceil(r) = 2 samples: one frame)
            e2e = float(np.abs(feats[u] - M.compute_mfcc_batch(x[u:u + 1, :nu], sr, L)[0]).max())
            assert e2e < ATOL, (case, u, e2e)
        else:
            assert not feats[u].any()
    print(f"\n{case}: worst error {worst:.3f} of the bound 2e-6 max|x|")
    _record(case, [k for k in expect if k not in (BDFT, DCT)], worst)
    if case == "h2-f32":
        _bits["h2-f32"] = got
    if case == "h2-f32-3-workgroups" and "h2-f32" in _bits:
        print(f"{case}: 3 workgroups looping over 10 work items give {'the same bits as' if _same_bits(got, _bits['h2-f32']) else 'other bits than'} "
              "one workgroup per work item")
    elif case == "h2-f32-3-workgroups":
        print(f"{case}: not compared with the default distribution (the case h2-f32 did not run before this one)")
    if nv is not None:  # a clip in a ragged launch = a plan of its own length running it alone (rows of 4 k samples stay on this kernel)
        for u, nu in enumerate(nv):
            if nu >= 4 and nu % 4 == 0 and (u == 0 or nu != nv[0]):
                with Plan(sr, nu, 1) as one:
                    w1 = Buf((1, nu), dev_rows[u:u + 1, :nu], False, np.int16 if fmt else np.float32)
                    o1 = Buf((1, 20 * L))
                    before = _snapshot()
                    N.check(N.lib.lipasr_mfcc_extract(one.h, w1.ptr(), fmt, None, 1, L, None, None, o1.ptr(), N.stream_ptr()))
                    torch.cuda.synchronize()
                    _assert_moved(before, {H2_I16 if fmt else H2_F32: 1, BDFT: 1, DCT: 1}, f"{case}: clip {u} alone")
                    assert _same_bits(one.stage(2, 1)[0], got[u, :one.n_y]), (case, u, nu)
                    assert _same_bits(o1.read(1)[0], feats[u]), (case, u, nu)


# ====================================================================================================== stages B and C
# The factor of the stage-B bound per STFT kernel instance: STAGE_B_FACTOR = 8 (tests/mfcc_stage_ref.py) unless listed here.  An entry
# is the smallest power of two that held on the MI355X, with the measured device / yardstick ratio and the reason (DESIGN.md, K1
# coverage, holds the whole table).
# Every entry has the same reason.  The device's power is read from d_db, a float32 dB value: its spacing at magnitudes 32 .. 128 is 0.9e-6
# to 1.8e-6 of the power, several times the float32 oracle's whole error (0.5e-7 .. 5e-7), and the kernels' log10f adds to it.  Kernels
# with different arithmetic land on the SAME figure (stft_bdft_kernel = stft_mel2_kernel = 1.671e-06 on the 1e-4 noise clip of 700
# samples), and against a yardstick that is itself taken through a float32 dB value every kernel is within 3.2 x.
STAGE_B_FACTORS = {
    BDFT: 16.0,       # measured 10.87 (bdft-2, full-scale noise; 9.71 and 9.21 on the 1e-4 noise clip of 700 and 2205 samples)
    BDFT_DCT: 16.0,   # measured 9.21 (the same dB tile as BDFT at 2205 samples)
    MEL2: 16.0,       # measured 9.71 (mel2-700, the 1e-4 noise clip)
    MEL: 32.0,        # measured 18.24 (mel-2, the impulse clip; 10.40 at 700 samples)
    DFT: 16.0,        # measured 11.70 (dft-32-32-200, the 1e-4 noise clip)
    FUSED_F32: 32.0,  # measured 21.89 (fused-f32-1600, the impulse clip)
    FUSED_I16: 32.0,  # measured 16.03 (fused-i16-1600 and -1601, the impulse clip): 16 does not hold
}


def _check_stage_b(case, db, fmax, refs, kernels):
    """db [batch][>= frames][128], fmax [batch][>= frames] of the device; refs: per clip (P64 [frames][128], yardstick [frames],
    yardstick through a float32 dB value [frames]).  Every figure is printed before anything about it is asserted."""
    factor = max(STAGE_B_FACTORS.get(k, S.STAGE_B_FACTOR) for k in kernels)
    assert factor <= S.STAGE_B_MAX_FACTOR  # what the CPU companion shows to be decisive
    loud = [r for r in refs if not S.silent_frames(r[0]).all()]
    yard = max((float(r[1][~S.silent_frames(r[0])].max()) for r in loud), default=0.0)
    yard_db = max((float(r[2][~S.silent_frames(r[0])].max()) for r in loud), default=0.0)
    bound = factor * yard
    worst, where = 0.0, None
    for u, (P64, _, _) in enumerate(refs):
        nf = P64.shape[0]
        silent = S.silent_frames(P64)
        if nf and (~silent).any():
            m = S.frame_metric(S.db_to_power(db[u, :nf]), P64)[~silent]
            if m.max() > worst:
                worst, where = float(m.max()), (u, int(np.flatnonzero(~silent)[m.argmax()]))
    ratio = worst / yard if yard else 0.0
    print(f"\n{case}: stage B worst {worst:.3e} (clip, frame {where}), float32 yardstick {yard:.3e}, device / yardstick {ratio:.2f} (bound {factor:g}); "
          f"yardstick through a float32 dB value {yard_db:.3e}, device / that {worst / yard_db if yard_db else 0.0:.2f}")
    for u, (P64, _, _) in enumerate(refs):
        nf = P64.shape[0]
        if nf == 0:
            continue
        assert _same_bits(fmax[u, :nf], db[u, :nf].max(axis=1)), f"{case}: clip {u}: the frame maxima are not the maxima of the dB rows"
        silent = S.silent_frames(P64)
        assert (db[u, :nf][silent] == np.float32(-100.0)).all(), f"{case}: clip {u}: a frame that is all at amin in float64 is not exactly -100 dB"
    assert worst <= bound, (f"{case}: clip, frame {where}: mel power {worst:.3e} of the frame's peak from float64, "
                            f"bound {bound:.3e} = {factor:g} x the float32 oracle's {yard:.3e}")
    _record(case, kernels, worst / bound if bound else 0.0, ratio)


def _check_stage_c(case, out, db, fmax, frames, L, mean, scale, kernels):
    """out [batch][20 L] against float64 on the device's own dB tile and frame maxima; frames: per clip frame count"""
    worst = 0.0
    for u, nf in enumerate(frames):
        val, bound = S.dct_reference(db[u], fmax[u], nf, L, mean, scale)
        err = np.abs(out[u].reshape(20, L) - val)
        at = np.unravel_index((err - bound).argmax(), err.shape)
        assert (err <= bound).all(), f"{case}: clip {u}: coefficient, frame {at} is {err[at]:.3e} from float64, bound {bound[at]:.3e}"
        pad = out[u].reshape(20, L)[:, min(nf, L):]
        want = np.zeros((20, L)) if mean is None else (0.0 - np.asarray(mean).reshape(20, L)) / np.asarray(scale).reshape(20, L)
        assert _same_bits(pad, want[:, min(nf, L):].astype(np.float32)), f"{case}: clip {u}: columns from frame {nf} on are not the zero columns of fix_frames"
        if nf and L:
            worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
    print(f"{case}: stage C worst {worst:.3f} of the derived bound")
    _record(case, kernels, worst)


def _run_22k(plan, y_rows, batch, L, expect, case, y_off=False, out_off=False, affine=None, nv=None):
    """lipasr_mfcc_plan_from_22k (or _ragged) twice from the same rows; returns out, db, fmax of the first run after comparing the bits"""
    N = _native()
    runs = []
    mean, scale = (_dev64(affine[0]), _dev64(affine[1])) if affine else (None, None)
    for rep in range(2):
        y = Buf((plan.batch_max, plan.n_y), np.concatenate([y_rows, np.full((plan.batch_max - batch, plan.n_y), SENTINEL, np.float32)]), y_off)
        out = Buf((plan.batch_max, 20 * L), None, out_off)
        nvt = _nv(nv)
        before = _snapshot()
        if nv is None:
            N.check(N.lib.lipasr_mfcc_plan_from_22k(plan.h, y.ptr(), batch, plan.n_y, L, N.ptr(mean), N.ptr(scale), out.ptr(), N.stream_ptr()))
        else:
            N.check(N.lib.lipasr_mfcc_plan_from_22k_ragged(plan.h, y.ptr(), N.ptr(nvt), batch, L, N.ptr(mean), N.ptr(scale), out.ptr(), N.stream_ptr()))
        torch.cuda.synchronize()
        _assert_moved(before, expect, case)
        y.read()
        runs.append((out.read(batch), plan.stage(0, batch), plan.stage(1, batch)))
    for a, b in zip(runs[0][:1] if nv is not None else runs[0], runs[1]):  # (ragged: frames past a clip's end hold what an earlier call left)
        assert _same_bits(a, b), f"{case}: two runs from the same inputs differ"
    return runs[0]


N_Y = (2, 700, 2205, 22528)  # 1 frame (repeated reflection), 2 frames (n_y <= 1024), 5 frames (a lone fifth), 45 frames (44 + 1)
# id: (n_fft, hop, n_y, plan keys, y off, L or None = all frames, counters, the STFT kernel judged)
B_CASES = {}
for _n in N_Y:
    for _off in (False, True):
        B_CASES[f"bdft-{_n}{'-off' if _off else ''}"] = (2048, 512, _n, (), _off, None, {BDFT: 1, DCT: 1}, BDFT)
    B_CASES[f"mel2-{_n}"] = (2048, 512, _n, ((0, 256),), False, None, {MEL2: 1, DCT: 1}, MEL2)
    B_CASES[f"mel-{_n}"] = (2048, 512, _n, ((0, 64),), False, None, {MEL: 1, DCT: 1}, MEL)
for _n in (2205, 22528):
    B_CASES[f"bdft-seg4-{_n}"] = (2048, 512, _n, ((3, 4),), False, None, {BDFT: 1, DCT: 1}, BDFT)
for _f, _h, _n in ((32, 32, 200), (33, 16, 200), (64, 1, 100), (441, 220, 2205), (510, 510, 2205)):
    B_CASES[f"dft-{_f}-{_h}-{_n}"] = (_f, _h, _n, (), False, None, {DFT: 1, DCT: 1}, DFT)


@functools.lru_cache(maxsize=None)
def _b_inputs(n_fft, hop, n_y, six):
    clips = S.stage_b_clips(n_y)
    if six:  # 441/220: 6 clips x 13 rows = 78 virtual rows, so that a 64-row workgroup spans two clips
        clips = np.concatenate([clips, S.stage_b_clips(n_y, seed=1)[:1]])
    refs = [S.stage_b_reference(y, n_fft, hop) for y in clips]
    return clips, refs


@pytest.mark.parametrize("case", list(B_CASES))
def test_stage_b_stft_mel_db(cuda, case):
    n_fft, hop, n_y, keys, y_off, L, expect, kid = B_CASES[case]
    clips, refs = _b_inputs(n_fft, hop, n_y, (n_fft, hop) == (441, 220))
    batch = len(clips)
    with Plan(22050, n_y, batch + 1, n_fft, hop, keys) as plan:
        assert plan.n_y == n_y and plan.n_frames == 1 + n_y // hop == refs[0][0].shape[0]
        L = L or plan.n_frames
        out, db, fmax = _run_22k(plan, clips, batch, L, expect, case, y_off)
    _check_stage_b(case, db, fmax, refs, [kid])
    _check_stage_c(case, out, db, fmax, [plan.n_frames] * batch, L, None, None, [DCT])
    for u in range(batch):
        e2e = float(np.abs(out[u] - S.features_reference(clips[u], L, n_fft, hop)).max())
        assert e2e < ATOL, (case, u, e2e)
    if case in ("bdft-2205", "bdft-22528"):
        _bits[case] = db
    if case.startswith("bdft-seg4") and f"bdft-{n_y}" in _bits:
        print(f"{case}: 4 frames per workgroup give {'the same bits as' if _same_bits(db, _bits[f'bdft-{n_y}']) else 'other bits than'} 44")
    elif case.startswith("bdft-seg4"):
        print(f"{case}: not compared with 44 frames per workgroup (the case bdft-{n_y} did not run before this one)")


def test_short_window_plan_refuses_a_clip_inside_the_padding(cuda):
    """lipasr_mfcc_plan_ex (include/lipasr.h): the short-window path reflects once, so n_y <= n_fft / 2 is LIPASR_EINVAL"""
    N = _native()
    h = N.c_h()
    assert N.lib.lipasr_mfcc_create(N.get_handle(0).h, 22050, 16, 1, 32, 32, C.byref(h)) == N.EINVAL
    assert "clip shorter than the reflect padding" in N.last_error()
    assert N.lib.lipasr_mfcc_create(N.get_handle(0).h, 22050, 220, 1, 441, 220, C.byref(h)) == N.EINVAL
    with Plan(22050, 17, 1, 32, 32) as plan:
        assert plan.n_frames == 1


@pytest.mark.parametrize("n_y,L", [(n, L) for n in (2205, 22528) for L in ("frames", "frames-1", 64, 65)])
def test_bdft_dct_epilogue_equals_dct_kernel(cuda, n_y, L):
    """Plan key 4: with one workgroup per clip (<= 64 frames) and L <= 64 stft_bdft_kernel finishes with the floor and the DCT itself --
    id 11 moves, dct_kernel's id 15 does not -- and the features are the bits of the key-4-off path.  L = 65: the plain kernel and
    dct_kernel.  45 frames need plan key 3 = 48 for one workgroup per clip."""
    clips, refs = _b_inputs(2048, 512, n_y, False)
    keys = ((3, 48),) if n_y == 22528 else ()
    case = f"bdft-dct-{n_y}-L{L}"
    with Plan(22050, n_y, 6, keys=keys) as plan:
        Lv = {"frames": plan.n_frames, "frames-1": plan.n_frames - 1}.get(L, L)
        aff = _affine(Lv)
        plain = _run_22k(plan, clips, 5, Lv, {BDFT: 1, DCT: 1}, case + " (key 4 off)", affine=aff)
        plan.set(4, 1)
        fused = Lv <= 64
        out, db, fmax = _run_22k(plan, clips, 5, Lv, {BDFT_DCT: 1} if fused else {BDFT: 1, DCT: 1}, case, affine=aff)
    for a, b in zip(plain, (out, db, fmax)):
        assert _same_bits(a, b), f"{case}: the DCT epilogue and dct_kernel give different bits"
    if fused:
        _check_stage_b(case, db, fmax, refs, [BDFT_DCT])
        _check_stage_c(case, out, db, fmax, [plan.n_frames] * 5, Lv, aff[0], aff[1], [BDFT_DCT])


@pytest.mark.parametrize("mask", [0, 256])
@pytest.mark.parametrize("affine", [False, True])
def test_ragged_stft_equals_each_clip_alone(cuda, mask, affine):
    """lipasr_mfcc_plan_from_22k_ragged on stft_bdft_kernel (mask 0) and stft_mel2_kernel (mask 256): clips of 0, 1, 2 and 5 frames in
    rows of 2205 with garbage from int(n r) on, which is never read into the result: each clip's dB rows, frame maxima and features
    are the bits of a plan of its own length running it alone.  L = 6: zero columns past every clip (stage C with per-clip lengths)."""
    nv = (0, 2, 372, 1600)
    kid = MEL2 if mask else BDFT
    case = f"ragged-{'mel2' if mask else 'bdft'}{'-affine' if affine else ''}"
    L = 6
    aff = _affine(L, 1) if affine else None
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((4, 2205)).astype(np.float32)  # garbage everywhere ...
    clips, refs, frames = [], [], []
    for u, n in enumerate(nv):
        n_vy, c_y, nf = _clip_lengths(n, 16000)
        y = np.zeros(c_y, np.float32)
        y[:n_vy] = rng.uniform(-1.0, 1.0, n_vy)
        rows[u, :n_vy] = y[:n_vy]  # ... but the clip's int(n r) samples
        clips.append(y)
        frames.append(nf)
        refs.append(S.stage_b_reference(y) if nf else (np.zeros((0, 128)), np.zeros(0), np.zeros(0)))
    assert frames == [0, 1, 2, 5]
    with Plan(16000, 1600, 5, keys=((0, mask),)) as plan:
        assert plan.n_y == 2205
        out, db, fmax = _run_22k(plan, rows, 4, L, {kid: 1, DCT: 1}, case, affine=aff, nv=nv)
    _check_stage_b(case, db, fmax, refs, [kid])
    _check_stage_c(case, out, db, fmax, frames, L, aff and aff[0], aff and aff[1], [DCT])
    for u, n in enumerate(nv):
        if frames[u] == 0:
            continue
        with Plan(22050, len(clips[u]), 1, keys=((0, mask),)) as one:
            assert one.n_frames == frames[u]
            o1, d1, f1 = _run_22k(one, clips[u][None], 1, L, {kid: 1, DCT: 1}, f"{case}: clip {u} alone", affine=aff)
        assert _same_bits(d1[0], db[u, :frames[u]]) and _same_bits(f1[0], fmax[u, :frames[u]]) and _same_bits(o1[0], out[u]), (case, u)
        if not affine:
            assert float(np.abs(out[u] - S.features_reference(clips[u], L)).max()) < ATOL


# id: (sr, rows, sample format, plan key 2, n_valid, kernel)
F_CASES = {
    "fused-f32-1600": (16000, 1600, 0, 1, None, FUSED_F32),
    "fused-f32-5003": (16000, 5003, 0, 1, None, FUSED_F32),  # several frame groups
    "fused-f32-8k-800": (8000, 800, 0, 1, None, FUSED_F32),
    "fused-f32-1600-ragged": (16000, 1600, 0, 1, (1600, 1599, 372, 2, 0), FUSED_F32),
    "fused-f32-5003-ragged": (16000, 5003, 0, 1, (5003, 5000, 1601, 372, 0), FUSED_F32),
    "fused-i16-1601": (16000, 1601, 1, 0, None, FUSED_I16),  # rows that are no multiple of 4: the plan takes the fused kernel by itself
    "fused-i16-1600": (16000, 1600, 1, 1, None, FUSED_I16),
    "fused-i16-1601-ragged": (16000, 1601, 1, 0, (1601, 1600, 372, 2, 0), FUSED_I16),
    "fused-i16-1600-ragged": (16000, 1600, 1, 1, (1600, 1599, 372, 2, 0), FUSED_I16),
}


@pytest.mark.parametrize("case", list(F_CASES))
def test_stage_b_fused_kernel(cuda, case):
    """mfcc_fused_kernel through lipasr_mfcc_extract.  The oracle chain starts at wav: float64 resampling, then the float64 spectrogram;
    the yardstick is the float32 spectrogram of the float32-rounded float64 resampling."""
    N = _native()
    sr, n, fmt, key2, nv, kid = F_CASES[case]
    x = S.stage_b_clips(n, sr=sr)
    rng = np.random.default_rng(n)
    if fmt:
        dev = np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)
        x = (dev.astype(np.float32) / 32768.0).astype(np.float32)
    else:
        dev = x.copy()
    refs, frames, ys = [], [], []
    for u in range(5):
        nu = n if nv is None else nv[u]
        frames.append(_clip_lengths(nu, sr)[2])
        if nu < n:
            dev[u, nu:] = (rng.integers(-30000, 30000, n - nu) if fmt else rng.standard_normal(n - nu)).astype(dev.dtype)
        if frames[-1] == 0:
            refs.append((np.zeros((0, 128)), np.zeros(0), np.zeros(0)))
            continue
        y64 = M.librosa_load_resample(x[u, :nu], sr, dtype=np.float64)
        refs.append(S.stage_b_reference(y64.astype(np.float32), y64=y64))
    L = max(frames) + 1
    with Plan(sr, n, 6, keys=((2, key2),)) as plan:
        assert plan.fused and plan.n_frames == max(frames)
        runs = []
        for rep in range(2):
            wav = Buf(dev.shape, dev, False, np.int16 if fmt else np.float32)
            out = Buf((6, 20 * L))
            nvt = _nv(nv)
            before = _snapshot()
            N.check(N.lib.lipasr_mfcc_extract(plan.h, wav.ptr(), fmt, N.ptr(nvt), 5, L, None, None, out.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            _assert_moved(before, {kid: 1, DCT: 1}, case)
            wav.read()
            runs.append((out.read(5), plan.stage(0, 5), plan.stage(1, 5)))
        for a, b in zip(runs[0][:1] if nv is not None else runs[0], runs[1]):  # (ragged: frames past a clip's end hold what an earlier call left)
            assert _same_bits(a, b), f"{case}: two runs from the same inputs differ"
        out, db, fmax = runs[0]
        if fmt:  # int16 rows equal float32 rows of pcm 2^-15, bit for bit
            plan.set(2, 1)
            fdev = dev.astype(np.float32) / 32768.0
            wf = Buf(fdev.shape, fdev)
            of = Buf((6, 20 * L))
            before = _snapshot()
            N.check(N.lib.lipasr_mfcc_extract(plan.h, wf.ptr(), 0, N.ptr(_nv(nv)), 5, L, None, None, of.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            _assert_moved(before, {FUSED_F32: 1, DCT: 1}, case + " (float32 twin)")
            assert _same_bits(of.read(5), out)
    _check_stage_b(case, db, fmax, refs, [kid])
    _check_stage_c(case, out, db, fmax, frames, L, None, None, [DCT])
    for u in range(5):
        nu = n if nv is None else nv[u]
        if nu >= 2:
            e2e = float(np.abs(out[u] - M.compute_mfcc_batch(x[u:u + 1, :nu], sr, L)[0]).max())
            assert e2e < ATOL, (case, u, e2e)
    if nv is not None:  # a clip in a ragged launch = a plan of its own length running it alone: the fused kernel serves both
        for u in (1, 2):
            nu = nv[u]
            with Plan(sr, nu, 1, keys=((2, 1),)) as one:
                w1 = Buf((1, nu), dev[u:u + 1, :nu], False, np.int16 if fmt else np.float32)
                o1 = Buf((1, 20 * L))
                before = _snapshot()
                N.check(N.lib.lipasr_mfcc_extract(one.h, w1.ptr(), fmt, None, 1, L, None, None, o1.ptr(), N.stream_ptr()))
                torch.cuda.synchronize()
                _assert_moved(before, {kid: 1, DCT: 1}, f"{case}: clip {u} alone")
                assert _same_bits(o1.read(1)[0], out[u]), (case, u, nu)
                assert _same_bits(one.stage(0, 1)[0], db[u, :frames[u]]), (case, u, nu)


C_LENGTHS = (1, 3, 4, 5, 6, 44, 45, 64, 65, 129)


@pytest.mark.parametrize("n_y", [2205, 22528])
@pytest.mark.parametrize("L", C_LENGTHS)
def test_stage_c_dct_kernel(cuda, n_y, L):
    """dct_kernel against float64 on the device's own dB tile and frame maxima: zero columns past the clip, one to three chunks of 64
    frames, the last of one frame (65, 129), with and without the affine (negative scales too), out one float off.  The sixth clip's
    loudest frame is its last one, >= 60 dB above the frames that are output when L is small: the floor comes from a frame that is
    not output."""
    clips = np.concatenate([S.stage_b_clips(n_y), S.loud_last_clip(n_y)[None]])
    for variant, aff, off in (("", None, False), ("-affine-off", _affine(L, L), True)):
        case = f"dct-{n_y}-L{L}{variant}"
        with Plan(22050, n_y, 7) as plan:
            out, db, fmax = _run_22k(plan, clips, 6, L, {BDFT: 1, DCT: 1}, case, out_off=off, affine=aff)
        assert fmax[5].argmax() == plan.n_frames - 1 and fmax[5].max() - fmax[5, :min(L, 3)].max() > 60.0
        _check_stage_c(case, out, db, fmax, [plan.n_frames] * 6, L, aff and aff[0], aff and aff[1], [DCT])
        if aff is None:
            for u in range(6):
                e2e = float(np.abs(out[u] - S.features_reference(clips[u], L)).max())
                assert e2e < ATOL, (case, u, e2e)


@pytest.mark.parametrize("L", [3, 66])
def test_stage_c_floor_maximum_spans_both_wavefronts(cuda, L):
    """66 frames: dct_kernel's second wavefront alone sees the maxima of frames 64 and 65, the loud ones of the loud-last clip.  A
    threshold taken from the first wavefront's partial maximum would leave the quiet frames unfloored."""
    n_y = 33280
    clips = np.stack([S.stage_b_clips(n_y)[0], S.loud_last_clip(n_y)])
    case = f"dct-{n_y}-L{L}"
    with Plan(22050, n_y, 3) as plan:
        assert plan.n_frames == 66
        out, db, fmax = _run_22k(plan, clips, 2, L, {BDFT: 1, DCT: 1}, case)
    assert fmax[1].argmax() == 65 and fmax[1, 64:].min() - fmax[1, :63].max() > 60.0
    _check_stage_c(case, out, db, fmax, [66, 66], L, None, None, [DCT])
    for u in range(2):
        assert float(np.abs(out[u] - S.features_reference(clips[u], L)).max()) < ATOL


def test_stage_hook_validates(cuda):
    N = _native()
    with Plan(22050, 2205, 2) as plan:
        dst = Buf((2, 5))
        for args in ((None, 1, 1, dst.ptr()), (plan.h, 1, 1, None), (plan.h, 3, 1, dst.ptr()), (plan.h, -1, 1, dst.ptr()), (plan.h, 1, 0, dst.ptr()),
                     (plan.h, 1, 3, dst.ptr())):
            assert N.lib.lipasr_debug_mfcc_stage(*args, N.stream_ptr()) == N.EINVAL, args
        torch.cuda.synchronize()
        dst.read(0)


def test_every_k1_kernel_is_claimed_and_ran():
    """The ids lipasr_debug_k1_launches knows against the claims of the tables above: a kernel added without a case fails here.  Prints
    (-s) the table that DESIGN.md (K1 section) records.  This test reads what the cases of THIS process recorded (_ran, _worst): it is
    the last test of the module and passes only after the whole module ran in one process, in file order; selected alone, with -k or
    on a worker that did not run every case it fails with the list of kernels that no case of the session ran.  The two bit reports
    (3 workgroups, 4 frames per workgroup) likewise need their partner case to have run first, and say so when it has not."""
    lib = _native().lib
    have = {k for k in range(64) if lib.lipasr_debug_k1_launches(k) >= 0}
    assert lib.lipasr_debug_k1_launches(-1) == -1 and lib.lipasr_debug_k1_launches(len(K1_NAMES)) == -1
    assert have == set(range(len(K1_NAMES)))
    claimed = {BDFT_DCT}  # test_bdft_dct_epilogue_equals_dct_kernel
    for table in (A_CASES, B_CASES):
        for c in table.values():
            claimed |= set(c[-2] if table is B_CASES else c[-1])
    claimed |= {c[-1] for c in F_CASES.values()}
    assert have - claimed == set(), "kernels no case claims: " + ", ".join(K1_NAMES[k] for k in sorted(have - claimed))
    missing = have - set(_ran)
    assert not missing, "no case of this session ran: " + ", ".join(K1_NAMES[k] for k in sorted(missing))
    for k in sorted(have):
        assert lib.lipasr_debug_k1_launches(k) > 0
        frac, case, ratio = _worst[k]
        print(f"{k:2d} {K1_NAMES[k]}: first shown by {_ran[k]}; worst error {frac:.3f} of its bound ({case})" + (f"; device / yardstick {ratio:.2f}" if ratio is not None else ""))
