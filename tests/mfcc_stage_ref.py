"""Float64 references, clip sets and bounds of the per-stage MFCC tests (test_mfcc_instances_gpu.py, test_mfcc_instances_cpu.py).

Stage B (STFT + mel + dB) is judged on the mel POWER of every frame, P = 10^(dB/10):
    metric(frame) = max_m |P[m] - P64[m]| / max_m P64[m]
where P64 is oracle.mfcc_ref.power_spectrogram in float64 through the float64 mel bank, clamped at amin = 1e-10.  The yardstick is the
same metric for the oracle evaluated in float32 (power_spectrogram(y, np.float32) through the float32 mel bank, the reference's own
clean path), recomputed by every run; a case's bound is the kernel's factor x the yardstick of the case's worst frame.  The factor is
STAGE_B_FACTOR = 8, the project's: 2^-21 per product of the fp16-plane kernels against fp32's 2^-24, as in the VJP tests.  It is a
margin over the reference, not a measured property of the device.

The device's power is read from d_db, a float32 dB value, and the yardstick's is not.  A dB value of magnitude 64 .. 128 has a float32
spacing of 7.6e-6 dB, 1.8e-6 of the power, which is more than the whole error of the float32 oracle on quiet clips.  The kernels
whose arithmetic is otherwise within 8 x therefore get the next power of two where they need it (STAGE_B_FACTORS in
test_mfcc_instances_gpu.py, measured ratios in DESIGN.md); stage_b_reference also returns the yardstick taken through a float32 dB
value (librosa.power_to_db keeps float32), which the tests print next to the issue's, and never assert on.

Stage C (top_db floor + DCT) is judged against float64 arithmetic on the device's OWN dB tile and frame maxima, with the forward
error bound of a 128-term fp32 dot product in any order plus the final rounding.
"""
import numpy as np

from oracle import mfcc_ref as M

AMIN = 1e-10
STAGE_B_FACTOR = 8.0
STAGE_B_MAX_FACTOR = 32.0  # the largest factor a kernel may be given (test_mfcc_instances_gpu.STAGE_B_FACTORS)
SR = M.SR_TARGET


def stage_b_clips(n, seed=0, sr=SR):
    """The five clips of every stage-B batch, [5][n] float32 at `sr` Hz: full-scale uniform noise, 0.5 sin(2 pi 1000.3 t), 1e-4 x
    Gaussian noise, all zeros, a unit impulse at sample 700 (at the last sample of a clip that has no sample 700)."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / float(sr)
    imp = np.zeros(n)
    imp[min(700, n - 1)] = 1.0
    return np.stack([rng.uniform(-1.0, 1.0, n), 0.5 * np.sin(2 * np.pi * 1000.3 * t), 1e-4 * rng.standard_normal(n), np.zeros(n), imp]).astype(np.float32)


def mel_power(y, dtype, n_fft=M.N_FFT, hop=M.HOP):
    """max(amin, mel bank @ |STFT|^2) in `dtype`, [n_frames][128]"""
    S = M.power_spectrogram(y, dtype, n_fft, hop)
    return np.maximum(dtype(AMIN), M.mel_filterbank(n_fft=n_fft).astype(dtype) @ S).T


def mel_power_wrong(y, which, n_fft=M.N_FFT, hop=M.HOP):
    """Three wrong restatements in float64 that the stage-B bound must tell from the right one: 'hann' a symmetric instead of the
    periodic window, 'mel' the mel bank shifted by one bin, 'offset' every frame one sample late."""
    y = np.asarray(y, np.float64)
    yp = M.reflect_pad(y, n_fft // 2 + 1)[1:]  # one more reflected sample at the end, for the late frames
    n_frames = 1 + len(y) // hop
    idx = np.arange(n_fft)[:, None] + hop * np.arange(n_frames)[None, :] + (1 if which == "offset" else 0)
    win = np.hanning(n_fft) if which == "hann" else M.hann_periodic(n_fft)
    S = np.abs(np.fft.rfft(win[:, None] * yp[idx], axis=0)) ** 2
    bank = M.mel_filterbank(n_fft=n_fft).astype(np.float64)
    if which == "mel":
        bank = np.roll(bank, 1, axis=1)
    return np.maximum(AMIN, bank @ S).T


def frame_metric(P, P64):
    """max_m |P - P64| / max_m P64 per frame"""
    P, P64 = np.asarray(P, np.float64), np.asarray(P64, np.float64)
    return np.abs(P - P64).max(axis=1) / P64.max(axis=1)


def silent_frames(P64):
    """frames that are all at amin in float64"""
    return (np.asarray(P64) <= AMIN).all(axis=1)


def stage_b_reference(y, n_fft=M.N_FFT, hop=M.HOP, y64=None):
    """(P64 [T][128], yardstick [T], yardstick through a float32 dB value [T]) of one clip.  y: the float32 signal the float32 oracle
    reads; y64: the float64 signal behind it (the fused kernel's chain starts at the waveform: float64 resampling, whose float32
    rounding is y), default y itself.  The third entry is reported only."""
    P64 = mel_power(y if y64 is None else y64, np.float64, n_fft, hop)
    P32 = mel_power(np.asarray(y, np.float32), np.float32, n_fft, hop)
    db32 = np.float32(10.0) * np.log10(P32)  # power_to_db in float32, no top_db
    assert db32.dtype == np.float32
    return P64, frame_metric(P32, P64), frame_metric(db_to_power(db32), P64)


def db_to_power(db):
    return 10.0 ** (np.asarray(db, np.float64) / 10.0)


def dct_reference(db, fmax, nf, L, mean=None, scale=None, floor_frames=None):
    """Stage 3 in float64 from a dB tile db [n_frames][128] and frame maxima fmax [n_frames] of a clip with nf frames:
    floor at max(fmax[:nf]) - 80, DCT-II ortho, 20 x L coefficient-major with zero columns from frame nf on, optional affine
    (value - mean) / scale with mean, scale [20 L].  floor_frames: take the floor's maximum over that many frames only (a WRONG
    restatement, for the CPU companion).  Returns (value [20][L], bound [20][L]): per element
        bound = 130 * 2^-24 * sum_m |D[k][m]| |db_floored[m]| / |scale| + 2^-24 |value|
    the forward error of a 128-term fp32 dot product in any order (gamma_128 < 130 u) plus the final rounding."""
    D = M.dct_matrix()
    val = np.zeros((M.N_MFCC, L))
    mag = np.zeros((M.N_MFCC, L))
    n = min(nf, L)
    if nf > 0 and n > 0:
        thr = np.float64(np.max(np.asarray(fmax, np.float64)[:nf if floor_frames is None else floor_frames])) - 80.0
        fl = np.maximum(np.asarray(db, np.float64)[:n], thr)  # [n][128]
        val[:, :n] = D @ fl.T
        mag[:, :n] = np.abs(D) @ np.abs(fl).T
    if mean is not None:
        mean, scale = np.asarray(mean, np.float64).reshape(M.N_MFCC, L), np.asarray(scale, np.float64).reshape(M.N_MFCC, L)
        val = (val - mean) / scale
        mag = mag / np.abs(scale)
    return val, 130.0 * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(val)


def loud_last_clip(n=2205, seed=0):
    """A clip whose loudest frame is its last one: 1e-5 x Gaussian noise, full-scale uniform noise over the last 105 samples.  The
    frames whose windows end before them (frames 0 .. 2 of the 5 at n = 2205, 0 .. 41 of the 45 at n = 22528) see the quiet part
    only, about 100 dB below the last frame."""
    rng = np.random.default_rng(2000 + seed)
    y = 1e-5 * rng.standard_normal(n)
    y[n - 105:] = rng.uniform(-1.0, 1.0, 105)
    return y.astype(np.float32)


def features_reference(y, L, n_fft=M.N_FFT, hop=M.HOP):
    """the end-to-end oracle from a 22 050 Hz clip, [20 L] coefficient-major (float32 clean path for 2048/512, float64 for the
    short windows, as the reference runs them)"""
    dt = np.float32 if (n_fft, hop) == (M.N_FFT, M.HOP) else np.float64
    return M.fix_frames(M.mfcc_22k(np.asarray(y, dt), dt, n_fft, hop), L).astype(np.float64).reshape(-1)
