"""Differentiable float64 restatement of the waveform -> MFCC forward (oracle.mfcc_ref, include/lipasr.h K1) in torch, so
that autograd supplies the oracle gradient of the MFCC stage, for the 2048/512 plans and (``n_fft=``, ``hop=``) the short-window
ones.  TEST INFRASTRUCTURE for tests/test_wave_attacks_*, test_wave_ragged_* and test_short_vjp_*: the tables come from
oracle.mfcc_ref (_polyphase_table, hann_periodic, mel_filterbank, dct_matrix); nothing here is used by the library.

    y   = R x                      kaiser_best polyphase taps (unfold + per-phase dot) + librosa's appended zero sample
    X_t = rfft(hann_N * reflect_pad(y, N // 2)[hop t : hop t + N]),  t < 1 + n_y // hop
    db  = 10 log10(max(1e-10, W_N |X|^2)),  thr = max(db) - 80,  c = D max(db, thr)
    out[k L + t] = (c[k, t] - mean) / scale for t < min(T, L), the zero columns of fix_frames standardised like the rest

The reflect padding is an index gather with np.pad's own indices, ``np.pad(np.arange(n_y), N // 2, mode="reflect")``: valid for
any clip of n_y >= 2 samples (np.pad reflects repeatedly; torch's reflect pad refuses a clip that is not longer than the padding)
and differentiable (autograd scatters the gradient back through the gather: the general adjoint of the padding).
``dtype=torch.float32`` evaluates the same graph in single precision: the yardstick the GPU parity bounds are built on
(``parity_rows`` below).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import mfcc_ref as M

SR = M.SR_TARGET


def resample(x, sr_in, dtype=torch.float64):
    """librosa_load_resample as a differentiable map: [n] -> [ceil(n * 22050 / sr_in)]."""
    x = x.to(dtype)
    if sr_in == SR:
        return x
    h, n_off, L, Md, wing = M._polyphase_table(sr_in, SR)
    n = x.shape[0]
    ratio = float(SR) / float(sr_in)
    n_out, n_fixed = int(n * ratio), int(math.ceil(n * ratio))
    nq = (n_out + L - 1) // L
    xp = torch.cat([torch.zeros(wing - 1, dtype=dtype), x, torch.zeros(2 * wing + Md * (nq + 1), dtype=dtype)])
    win = xp.unfold(0, 2 * wing, 1)  # win[i] = x[i - 63 .. i + 64]
    ht = torch.as_tensor(h).to(dtype)
    base = Md * torch.arange(nq)
    cols = [win[base + int(n_off[p])] @ ht[p] for p in range(L)]
    y = torch.stack(cols, dim=1).reshape(-1)[:n_out]
    if n_fixed > n_out:
        y = torch.cat([y, torch.zeros(n_fixed - n_out, dtype=dtype)])
    return y


def db_22k(y, dtype=torch.float64, n_fft=M.N_FFT, hop=M.HOP):
    """[n_y >= 2] -> pre-floor dB [1 + n_y // hop, 128]."""
    y = y.to(dtype)
    idx = torch.as_tensor(np.pad(np.arange(y.shape[0]), n_fft // 2, mode="reflect"))
    frames = y[idx].unfold(0, n_fft, hop)
    hann = torch.as_tensor(M.hann_periodic(n_fft)).to(dtype)
    X = torch.fft.rfft(frames * hann, dim=1)
    P = X.real ** 2 + X.imag ** 2
    W = torch.as_tensor(M.mel_filterbank(n_fft=n_fft).astype(np.float64)).to(dtype)
    mel = P @ W.T
    return 10.0 * torch.log10(torch.clamp(mel, min=1e-10))


def features_22k(y, utterance_length=M.STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, dtype=torch.float64, n_fft=M.N_FFT, hop=M.HOP):
    """[n_y] at 22 050 Hz -> standardised features [20 * L], coefficient-major."""
    db = db_22k(y, dtype, n_fft, hop)
    thr = db.max() - 80.0
    D = torch.as_tensor(M.dct_matrix()).to(dtype)
    c = (torch.maximum(db, thr) @ D.T).T  # [20, T]
    T, L = c.shape[1], utterance_length
    c = c[:, :L] if T >= L else torch.cat([c, torch.zeros(c.shape[0], L - T, dtype=dtype)], dim=1)  # M.fix_frames
    out = c.reshape(-1)
    if mean is not None:
        out = (out - torch.as_tensor(mean).to(dtype)) / torch.as_tensor(scale).to(dtype)
    return out


def features(x, sr_in=16000, utterance_length=M.STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, dtype=torch.float64, domain="input",
             n_fft=M.N_FFT, hop=M.HOP):
    """domain="input": x at sr_in; "22k": x is already the 22 050 Hz signal."""
    y = x.to(dtype) if domain == "22k" else resample(x, sr_in, dtype)
    return features_22k(y, utterance_length, mean, scale, dtype, n_fft, hop)


def vjp(x, g_feat, sr_in=16000, utterance_length=M.STANDARD_UTTERANCE_LENGTH, scale=None, dtype=torch.float64, domain="input",
        n_fft=M.N_FFT, hop=M.HOP):
    """Gradient of <features(x), g_feat> w.r.t. x (NumPy in, NumPy float64 out), the graph evaluated in ``dtype``."""
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype).requires_grad_(True)
    f = features(xt, sr_in, utterance_length, None if scale is None else np.zeros_like(np.asarray(scale)), scale, dtype, domain, n_fft, hop)
    (f * torch.as_tensor(np.asarray(g_feat, dtype=np.float64)).to(dtype)).sum().backward()
    return xt.grad.detach().to(torch.float64).numpy()


def guard_margins(y22, n_fft=M.N_FFT, hop=M.HOP):
    """(distance of the closest pre-floor dB element to the top_db floor -- over ALL elements, the empty mel bands pinned at -100 dB
    included --, gap between the two largest, number of elements below the floor), float64."""
    with torch.no_grad():
        db = db_22k(torch.as_tensor(np.asarray(y22, dtype=np.float64)), n_fft=n_fft, hop=hop).reshape(-1)
    top = torch.topk(db, 2).values
    thr = top[0] - 80.0
    return float((db - thr).abs().min()), float(top[0] - top[1]), int((db < thr).sum())


# ---- what the GPU parity tests share ----
def errs(g, g64):
    """(inf-norm, two-norm) error of g relative to the float64 gradient's norms."""
    d = g - g64
    return float(np.abs(d).max() / np.abs(g64).max()), float(np.linalg.norm(d) / np.linalg.norm(g64))


def onehot(lab, n):
    y = np.zeros((len(lab), n), dtype=np.float32)
    y[np.arange(len(lab)), lab] = 1
    return y


def mean_ce(prob, y):
    return float(-np.log(np.maximum(prob[np.arange(len(y)), y], 1e-30)).mean())


def parity_row(got, sig, g_feat, **vjp_kw):
    """One clip: the device gradient ``got`` against the float64 oracle, and the float32 oracle (the yardstick) against the same ->
    (errs of the device, errs of the float32 oracle, sign-mismatch share of the device, of the float32 oracle, the float64 gradient)."""
    g64 = vjp(sig, g_feat, **vjp_kw)
    g32 = vjp(sig, g_feat, dtype=torch.float32, **vjp_kw)
    return (errs(got, g64), errs(g32, g64), float(np.mean(np.sign(got) != np.sign(g64))), float(np.mean(np.sign(g32) != np.sign(g64))), g64)


# ---- the parity clips: four non-stationary analytic signals at three lengths (33, 44 and 54 frames against L = 44) ----
LENGTHS = (12000, 16000, 20000)
# with per-clip lengths, four clips per length, 16 kHz.  n_y = ceil(n * 1.378125): 1486 -> 2048 (the old limit of the backward pass:
# the two reflected flanks overlap), 1487 -> 2050, 400 and 40 need repeated reflection, 3000 -> 9 frames (a second frame group of
# one unpaired frame), 7000 -> 19 frames, 20000 -> 54 frames > L = 44
RAGGED_LENGTHS = (40, 400, 1000, 1486, 1487, 3000, 7000, 12000, 16000, 20000)
CLIP_NAMES = ("chirp", "noise", "voiced", "chirp_gated_noise")
CLIP_SEED = 20240611  # the noise draws; chosen, like the clips, so that every clip passes guard_margins with room


def parity_clips(n_samples, sr=16000):
    """[4, n_samples] float32: the 200 -> 3500 Hz chirp, 0.1 x white noise, a voiced clip (19 harmonics of a gliding 140 Hz under
    a raised-sine envelope + 1e-3 noise) and the chirp plus gated noise.  Stationary clips (a pure tone, a clipped square) have
    near-ties at the clip maximum (top gaps below 1e-8 dB) and are no parity inputs."""
    t = np.arange(n_samples) / sr
    dur = n_samples / sr
    rngs = [np.random.default_rng(CLIP_SEED + 10 * n_samples + i) for i in range(3)]
    chirp = 0.4 * np.sin(2 * np.pi * (200.0 * t + 0.5 * (3300.0 / dur) * t * t))
    noise = 0.1 * rngs[0].standard_normal(n_samples)
    f0_phase = 2 * np.pi * (140.0 * t + 0.5 * (40.0 / dur) * t * t)  # 140 -> 180 Hz glide
    env = 0.05 + 0.95 * np.sin(np.pi * (t / dur) ** 0.7) ** 2  # skewed: a symmetric envelope puts two near-equal maxima in the clip
    voiced = env * sum(np.sin(h * f0_phase) / h for h in range(1, 20)) * 0.25 + 1e-3 * rngs[1].standard_normal(n_samples)
    gate = ((t / dur > 0.3) & (t / dur < 0.62)).astype(np.float64)
    gated = chirp + 0.05 * gate * rngs[2].standard_normal(n_samples)
    return np.stack([chirp, noise, voiced, gated]).astype(np.float32)


# ---- the short-window parity clips: per shape three non-stationary analytic signals at 22 050 Hz, seeds searched on the CPU so that every
# clip (and every gain it is used at) passes guard_margins with room.  With ~13 k dB elements per 441/220 window a clip whose range
# straddles the 80 dB floor lands within 1e-2 dB of it by chance: about one seed in three passes. ----
SHORT_SHAPES = ((441, 220, 22050), (400, 160, 4000), (510, 510, 2040), (64, 32, 1000), (32, 7, 300))
SHORT_CLIP_NAMES = ("chirp_gated_noise", "voiced", "noise")
# (seed of the chirp + gated noise clip, seed of the voiced clip, seed of the noise clip) per shape
SHORT_CLIP_SEEDS = {
    (441, 220, 22050): (7, 1, 0),  # 7372 floored elements (the pinned bands among them), 5, and none
    (400, 160, 4000): (0, 0, 0),
    (510, 510, 2040): (0, 0, 0),
    (64, 32, 1000): (0, 15, 0),
    (32, 7, 300): (0, 2, 0),
}
# the gains a batch repeats the clips at.  A gain g shifts every dB value by 20 log10 g; the noise clip is quiet on purpose: its
# maximum stays below -20 dB, so that the empty mel bands (pinned at -100 dB) lie ABOVE its floor and it has no floored element.
SHORT_GAINS = (1.0, 0.5, 0.7, 0.35, 0.85)


def make_short_clip(kind, n, seed):
    """One analytic clip of n samples at 22 050 Hz (float64)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    dur = n / SR
    u = t / dur
    env = 0.05 + 0.95 * np.sin(np.pi * u ** 0.7) ** 2  # skewed: a symmetric envelope puts two near-equal maxima in the clip
    if kind == "chirp_gated_noise":  # 300 -> 5000 Hz chirp under the envelope, noise in the middle third
        f0, f1 = 300.0 + 50.0 * rng.uniform(), 5000.0 + 500.0 * rng.uniform()
        chirp = 0.4 * env * np.sin(2 * np.pi * (f0 * t + 0.5 * ((f1 - f0) / dur) * t * t) + rng.uniform(0, 2 * np.pi))
        gate = ((u > 0.3) & (u < 0.62)).astype(np.float64)
        return chirp + 0.02 * gate * rng.standard_normal(n)
    if kind == "voiced":  # 19 harmonics of a gliding 140 Hz + a noise floor 50 dB down
        ph = 2 * np.pi * ((140.0 + 10.0 * rng.uniform()) * t + 0.5 * (40.0 / dur) * t * t)
        return env * sum(np.sin(h * ph + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 20)) * 0.25 + 1e-3 * rng.standard_normal(n)
    if kind == "noise":  # quiet white noise under the envelope
        return 0.004 * (0.3 + 0.7 * env) * rng.standard_normal(n)
    raise ValueError(kind)


def short_parity_clips(n_fft, hop, n_samp):
    """[3, n_samp] float32 in SHORT_CLIP_NAMES order."""
    seeds = SHORT_CLIP_SEEDS[(n_fft, hop, n_samp)]
    return np.stack([make_short_clip(k, n_samp, s) for k, s in zip(SHORT_CLIP_NAMES, seeds)]).astype(np.float32)


def short_parity_batch(n_fft, hop, n_samp, batch):
    """[batch, n_samp] float32: row i is clip i % 3 at gain SHORT_GAINS[i // 3]."""
    c = short_parity_clips(n_fft, hop, n_samp)
    return np.stack([(np.float32(SHORT_GAINS[i // 3]) * c[i % 3]).astype(np.float32) for i in range(batch)])


# the clips of the domain-"input" test: 16 000 samples at 16 kHz (the same generators; their time axis is then 1.378 x slower), seeds
# searched so that the RESAMPLED signal (oracle.mfcc_ref.librosa_load_resample, 22 050 samples) passes guard_margins at 441/220
INPUT_RATE, INPUT_SAMPLES = 16000, 16000
INPUT_SEEDS = (104, 100, 100)


def input_rate_clips():
    """[3, 16000] float32 in SHORT_CLIP_NAMES order."""
    return np.stack([make_short_clip(k, INPUT_SAMPLES, s) for k, s in zip(SHORT_CLIP_NAMES, INPUT_SEEDS)]).astype(np.float32)
