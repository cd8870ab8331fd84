"""Float64 references per stage of the MFCC backward pass (test_mfcc_vjp_instances_gpu.py, test_mfcc_vjp_instances_cpu.py), with the
wrong restatements the CPU companion holds the bounds against.  The chain is the one include/lipasr.h states at lipasr_mfcc_plan_vjp.

Stage 1 (mfcc_vjp_db_kernel): dB tile, frame maxima, g_feat -> Gmel.  The comparisons the kernel makes in fp32 are made in np.float32
(thr = mx - 80, d > thr, d == mx, d > -100), so that the mask and the arg-max are the kernel's by construction; everything else is
float64.  Next to the value stands its absolute evaluation A (every term replaced by its magnitude, the floored sum that lands on the
maximum included); the device is held to |got - ref| <= F1 2^-24 A per element.

Stages 2+3 (stft_vjp_kernel + stft_vjp_fold_kernel, dft_vjp_kernel + dft_vjp_fold_kernel): a 22 050 Hz clip and a Gmel tile -> g_y:
GP = W^T Gmel, Z = 2 GP X on the one-sided bins, frame gradient = hann Re sum_k Z[k] e^{+2 pi i k n / N}, overlap-add, adjoint of
np.pad's reflection (a scatter through np.pad's own indices: valid for any n_y >= 2).  dtype=torch.float32 evaluates the same steps in
single precision: the yardstick.  The device is held to F2 x the yardstick's error in the metric of mfcc_grad_ref.errs.

Stage 4 (resample_vjp_kernel, copy_cut_kernel): R^T as an explicit float64 sum over the fp32 taps exactly as the kernels read them
(lipasr_debug_table 3 / 4 / 5), so that tap rounding does not enter the error; the bound (nt + 1) 2^-24 sum |h| |g_y| is the a-priori
bound of nt sequential fmas.

The factors start at STAGE_B_FACTOR = 8 and never exceed STAGE_B_MAX_FACTOR = 32 (tests/mfcc_stage_ref.py).
"""
import functools
import math

import numpy as np
import torch

import mfcc_stage_ref as S
from oracle import mfcc_ref as M

U = 2.0 ** -24
F_START = S.STAGE_B_FACTOR
F_MAX = S.STAGE_B_MAX_FACTOR
DB_SLOPE = 10.0 / math.log(10.0)
SR = M.SR_TARGET


def clip_lengths(n, sr):
    """(int(n r), ceil(n r), frames) of a clip of n samples at sr, 2048/512 (include/lipasr.h, lipasr_mfcc_plan_vjp_ragged)"""
    v = n * (float(SR) / float(sr))
    n_y = int(math.ceil(v))
    return int(v), n_y, (1 + n_y // M.HOP if n_y >= 2 else 0)


# ====================================================================================================== stage 1
def stage1(db, fmax, g_feat, L, T, scale=None, wrong=None, cmp=np.float32):
    """db [>= T][128], fmax [>= T] float32 as the plan holds them, g_feat [20 L], T the clip's frames -> (Gmel [T][128], A [T][128]).
    cmp: the type the comparisons are made in (np.float64 only where a float64 tile is composed with the other stages).
    wrong: None, or one of 'last' (the floored sum to the LAST maximum), 'ge' (>= instead of > at the floor), 'drop' (the floored sum
    dropped), 'firstL' (the maximum searched over the first L frames only), 'mul' (multiply instead of divide by the scale)."""
    val, A = np.zeros((T, M.N_MELS)), np.zeros((T, M.N_MELS))
    if T == 0:
        return val, A
    d = np.ascontiguousarray(np.asarray(db, cmp)[:T])
    fm = np.asarray(fmax, cmp)[:T]
    Tc = min(T, L)
    g = np.asarray(g_feat, np.float64).reshape(M.N_MFCC, L)[:, :Tc]
    if scale is not None:
        sc = np.asarray(scale, np.float64).reshape(M.N_MFCC, L)[:, :Tc]
        g = g * sc if wrong == "mul" else g / sc
    D = M.dct_matrix()  # [20][128]
    gd, gd_abs = np.zeros((T, M.N_MELS)), np.zeros((T, M.N_MELS))
    gd[:Tc] = g.T @ D
    gd_abs[:Tc] = np.abs(g).T @ np.abs(D)
    # the kernel's own comparisons, in float32
    T_max = min(T, L) if wrong == "firstL" else T
    mx = cmp(fm[:T_max].max())
    thr = cmp(mx - cmp(80.0))
    keep = (d >= thr) if wrong == "ge" else (d > thr)
    at_max = np.flatnonzero((d[:T_max] == mx).ravel())
    live = d > cmp(-100.0)
    gdb, gdb_abs = np.where(keep, gd, 0.0), np.where(keep, gd_abs, 0.0)
    if at_max.size and wrong != "drop":
        t, m = divmod(int(at_max[-1] if wrong == "last" else at_max[0]), M.N_MELS)
        # (the owner rewrites its slot from the unmasked Gdbc plus the floored sum)
        gdb[t, m] = gd[t, m] + gd[~keep].sum()
        gdb_abs[t, m] = gd_abs[t, m] + gd_abs[~keep].sum()
    slope = DB_SLOPE * 10.0 ** (-0.1 * d.astype(np.float64))
    val[:] = np.where(live, gdb * slope, 0.0)
    A[:] = np.where(live, gdb_abs * slope, 0.0)
    return val, A


def tile_from_clip(y, n_fft=M.N_FFT, hop=M.HOP):
    """(dB tile [T][128] float32, frame maxima [T] float32) as a float32 forward leaves them, from a 22 050 Hz clip"""
    db = (10.0 * np.log10(S.mel_power(np.asarray(y, np.float32), np.float32, n_fft, hop))).astype(np.float32)
    return db, db.max(axis=1)


def tie_tile(T=5, seed=0):
    """A tile with three positions exactly at the maximum, in frames 1, 1 and 3; a few elements below the floor."""
    rng = np.random.default_rng(4000 + seed)
    db = rng.uniform(-70.0, -5.0, (T, M.N_MELS)).astype(np.float32)
    db[0, :9] = rng.uniform(-99.0, -90.0, 9).astype(np.float32)  # floored: the sum is not zero
    for t, m in ((1, 40), (1, 90), (3, 7)):
        db[t, m] = np.float32(-2.5)
    return db, db.max(axis=1)


def floor_tile(T=5, seed=0):
    """A tile whose maximum is 3.25 dB (one element): elements exactly on thr = -76.75, one float32 step above it and below it, plus
    uniform values either side and pinned -100 dB elements."""
    rng = np.random.default_rng(5000 + seed)
    db = rng.uniform(-95.0, -20.0, (T, M.N_MELS)).astype(np.float32)
    db[2, 17] = np.float32(3.25)
    thr = np.float32(np.float32(3.25) - np.float32(80.0))
    for t in range(T):
        db[t, 30], db[t, 31], db[t, 32] = thr, np.nextafter(thr, np.float32(0.0)), np.nextafter(thr, np.float32(-200.0))
        db[t, 100:104] = np.float32(-100.0)
    return db, db.max(axis=1)


def last_element_tile(T=5, seed=0):
    """The maximum is the very last element of the clip (frame T - 1, mel 127); a third of the elements are floored."""
    rng = np.random.default_rng(6000 + seed)
    db = rng.uniform(-110.0, -20.0, (T, M.N_MELS)).astype(np.float32)
    db = np.maximum(db, np.float32(-100.0))
    db[T - 1, 127] = np.float32(-10.0)
    return db, db.max(axis=1)


def dead_tile(T=5):
    db = np.full((T, M.N_MELS), -100.0, np.float32)
    return db, db.max(axis=1)


# ====================================================================================================== stages 2 + 3
@functools.lru_cache(maxsize=None)
def _consts(n_fft, wrong_hann):
    win = np.hanning(n_fft) if wrong_hann else M.hann_periodic(n_fft)
    return win, M.mel_filterbank(n_fft=n_fft).astype(np.float64)


def reflect_indices(n_y, n_fft, wrong=None):
    """np.pad(arange(n_y), n_fft // 2, 'reflect'); wrong 'fold': the right flank folded about n_y instead of n_y - 1"""
    pad = n_fft // 2
    idx = np.pad(np.arange(n_y), pad, mode="reflect")
    if wrong == "fold":
        j = np.arange(n_y, n_y + pad)
        idx[pad + n_y:] = np.clip(2 * n_y - j, 0, n_y - 1)
    return idx


def stage23(y, gmel, n_fft=M.N_FFT, hop=M.HOP, dtype=torch.float64, wrong=None):
    """y [n_y >= 2] at 22 050 Hz, gmel [T][128] with T = 1 + (n_y + 2 (n_fft // 2) - n_fft) // hop -> (g_y [n_y] float64, reached [n_y] bool: samples that a frame
    with a non-zero cotangent row covers).  wrong: None, 'edge2' (bins 0 and N/2 doubled), 'edge1' (bins 1 and N/2 - 1 doubled), 'late' (frame gradients one sample late),
    'hann' (a symmetric Hann window), 'fold' (the right flank folded about n_y instead of n_y - 1)."""
    y = np.asarray(y, np.float64)
    n_y, pad = len(y), n_fft // 2
    T = 1 + (n_y + 2 * pad - n_fft) // hop
    gmel = np.asarray(gmel, np.float64)[:T]
    assert gmel.shape == (T, M.N_MELS)
    win, W = _consts(n_fft, wrong == "hann")
    cdt = torch.complex64 if dtype == torch.float32 else torch.complex128
    idx = torch.as_tensor(reflect_indices(n_y, n_fft))  # the forward's gather is always the right one
    yt, wt, Wt, gt = (torch.as_tensor(a).to(dtype) for a in (y, win, W, gmel))
    frames = yt[idx].unfold(0, n_fft, hop)[:T] * wt        # [T][N]
    X = torch.fft.rfft(frames, dim=1)                       # [T][N/2 + 1]
    GP = gt @ Wt                                            # W^T Gmel, [T][bins]
    Z = (2.0 * GP).to(cdt) * X
    if wrong in ("edge2", "edge1"):  # the two end bins; 'edge1': their inner neighbours
        e = 0 if wrong == "edge2" else 1
        Z[:, e] *= 2.0
        if n_fft % 2 == 0:
            Z[:, Z.shape[1] - 1 - e] *= 2.0
    Zp = torch.zeros((T, n_fft), dtype=cdt)
    Zp[:, :Z.shape[1]] = Z
    gf = (torch.fft.ifft(Zp, dim=1).real * float(n_fft)).to(dtype) * wt  # hann Re sum_k Z[k] e^{+2 pi i k n / N}
    live = (gmel != 0.0).any(axis=1)
    gyp = torch.zeros(n_y + 2 * pad + 1, dtype=dtype)
    cover = np.zeros(n_y + 2 * pad + 1, bool)
    shift = 1 if wrong == "late" else 0
    for t in range(T):  # ascending frames
        if live[t]:
            gyp[hop * t + shift:hop * t + shift + n_fft] += gf[t]
            cover[hop * t:hop * t + n_fft] = True
    fold = torch.as_tensor(reflect_indices(n_y, n_fft, wrong))
    g = torch.zeros(n_y, dtype=dtype).index_add_(0, fold, gyp[:n_y + 2 * pad])
    reached = np.zeros(n_y, bool)
    reached[reflect_indices(n_y, n_fft)[cover[:n_y + 2 * pad]]] = True
    return g.to(torch.float64).numpy(), reached


def errs(g, g64):
    """mfcc_grad_ref.errs: (inf-norm, two-norm) error relative to the float64 result's norms"""
    d = np.asarray(g, np.float64) - g64
    return float(np.abs(d).max() / np.abs(g64).max()), float(np.linalg.norm(d) / np.linalg.norm(g64))


def random_gmel(T, frames=None, seed=0):
    """A Gmel tile of signed values spread over four decades; frames: the frames that are non-zero (default all)"""
    rng = np.random.default_rng(7000 + seed)
    g = rng.standard_normal((T, M.N_MELS)) * 10.0 ** rng.uniform(-2.0, 2.0, (T, M.N_MELS))
    if frames is not None:
        keep = np.zeros(T, bool)
        keep[list(frames)] = True
        g[~keep] = 0.0
    return g.astype(np.float32)


# ====================================================================================================== stage 4
def polyphase_from_tables(h, meta, noff):
    """(H [up][taps] float64 from the fp32 taps, up, down, taps, left, n_off [up]) from lipasr_debug_table 3, 4, 5"""
    up, down, taps, left = (int(v) for v in meta)
    return np.asarray(h, np.float32).reshape(up, taps).astype(np.float64), up, down, taps, left, np.asarray(noff).astype(np.int64)


def oracle_tables(sr, rounded=True):
    """the same tuple from the oracle's float64 table, rounded to float32 as the library uploads it (rounded=False: as it is, for
    the composition with the autograd oracle)"""
    h, n_off, L, Md, wing = M._polyphase_table(sr, SR)
    return (h.astype(np.float32).astype(np.float64) if rounded else h), L, Md, 2 * wing, wing, np.asarray(n_off, np.int64)


def adjoint_taps(tab):
    """nt: the longest run of outputs that reach one input sample (the fmas one g_x sample takes, zero taps included)"""
    H, up, down, taps, left, noff = tab
    t = np.arange(-2 * up, (taps // down + 6) * up + 2 * up)
    pos = down * np.floor_divide(t, up) + noff[np.mod(t, up)]
    j = np.arange(2 * down, 3 * down)
    lo = np.searchsorted(pos, j + left - taps, side="left")
    hi = np.searchsorted(pos, j + left - 1, side="right")
    return int((hi - lo).max())


def resample_vjp(gy, n, sr, tab, wrong=None):
    """g_y [>= int(n r)] -> (g_x [n] float64, sum |h| |g_y| [n]).  Output t = up q + p of the forward reads x[down q + n_off[p] - (left
    - 1) + k], k < taps, for t < int(n r): the appended zero sample and everything after it receive nothing.  wrong: 'first' / 'last'
    (the first / last tap of every phase dropped), 't0' (every output's window one input sample late)."""
    if sr == SR:
        g = np.zeros(n)
        m = min(n, len(gy))
        g[:m] = np.asarray(gy, np.float64)[:m]
        return g, np.abs(g)
    H, up, down, taps, left, noff = tab
    if wrong in ("first", "last"):  # (the first / last NON-ZERO tap: the ends of a phase's row may be zero)
        H = H.copy()
        for p in range(up):
            nzp = np.flatnonzero(H[p])
            H[p, nzp[0 if wrong == "first" else -1]] = 0.0
    n_vy = int(n * (float(SR) / float(sr)))
    gy = np.asarray(gy, np.float64)[:n_vy]
    t = np.flatnonzero(gy)  # (a zero gives nothing)
    gy = gy[t]
    q, p = t // up, t % up
    j0 = down * q + noff[p] - (left - 1) + (1 if wrong == "t0" else 0)
    j = j0[:, None] + np.arange(taps)[None, :]
    ok = (j >= 0) & (j < n)
    contrib = H[p] * gy[:, None]
    g, a = np.zeros(n), np.zeros(n)
    np.add.at(g, j[ok], contrib[ok])
    np.add.at(a, j[ok], np.abs(contrib[ok]))
    return g, a


def comb_rows(n_y, n_vy, spacing):
    """[spacing][n_y] float32: row s carries unit impulses at s, s + spacing, ...; plus an impulse on the appended zero sample
    (position n_vy, when the row has one), which must give exactly nothing"""
    rows = np.zeros((spacing, n_y), np.float32)
    for s in range(spacing):
        rows[s, s:n_vy:spacing] = 1.0
        if n_vy < n_y:
            rows[s, n_vy] = 1.0
    return rows


# ====================================================================================================== what the two test files share
# The factors of the stage-1 and stage-2+3 bounds per kernel family: F_START = 8 unless the MI355X measurement ("Backward
# pass") asks for the next power of two at or above twice the worst measured ratio; never above F_MAX = 32.
# Measured on the MI355X, worst device / yardstick ratio over every case: stage 1 5.98 (one-7000-L44-d0 on a tile of stft_bdft_kernel;
# 5.15 on the tiles the backward pass reads now), so F1 = 16, the next power of two at or above twice that; stages 2+3 3.54
# (stft_vjp_kernel + fold, one-3000-L4-d0) and 2.58 (dft_vjp_kernel + fold, 441/220): both keep 8.
F1 = 16.0                                     # mfcc_vjp_db_kernel
F2 = {"stft": F_START, "dft": F_START}        # stft_vjp_kernel + fold, dft_vjp_kernel + fold
ONE_LENGTH_N = (1487, 3000, 7000)             # 16 kHz: n_y 2050 / 4135 / 9647, 5 / 9 / 19 frames, 1 / 2 / 3 frame groups
RAGGED_NV = {16000: (0, 1, 40, 400, 1486, 1487, 3000, 7000),   # n_y 0, 2, 56, 552, 2048, 2050, 4135, 9647
             8000: (0, 1, 20, 200, 743, 744, 1500, 3500)}      # n_y 0, 3, 56, 552, 2048, 2051, 4135, 9647
SHORT_SHAPES = ((441, 220, 2205), (32, 7, 300), (510, 510, 2040), (64, 32, 1000))


def case_clip(n_y, seed=0):
    """A 22 050 Hz clip for the stage cases: a chirp under a skewed envelope plus noise 40 dB down, and two tones at 11 Hz and 11 014 Hz so
    that the first and the last bins that a mel filter reads (1 and N/2 - 1) carry energy (float32)"""
    rng = np.random.default_rng(8000 + 17 * n_y + seed)
    t = np.arange(n_y) / float(SR)
    u = (np.arange(n_y) + 0.5) / n_y
    env = 0.1 + 0.9 * np.sin(np.pi * u ** 0.7) ** 2
    return (0.5 * env * np.sin(2 * np.pi * (300.0 * t + 0.5 * 4.0e4 * t * t) + rng.uniform(0, 6.28)) + 5e-3 * rng.standard_normal(n_y)
            + 0.1 * np.cos(2 * np.pi * 11.0 * t + 0.3) + 0.1 * np.cos(2 * np.pi * 11014.0 * t + 0.7)).astype(np.float32)


def case_cotangent(L, seed=0):
    """(g_feat [20 L], scale [20 L]): a cotangent of unit-variance entries and a StandardScaler scale in [0.5, 2], a quarter negative"""
    rng = np.random.default_rng(9000 + L + seed)
    return rng.standard_normal(20 * L).astype(np.float32), rng.uniform(0.5, 2.0, 20 * L) * np.where(rng.random(20 * L) < 0.25, -1.0, 1.0)
