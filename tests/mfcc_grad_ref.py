"""Differentiable float64 restatement of the waveform -> MFCC forward (oracle.mfcc_ref, include/lipasr.h K1) in torch, so
that autograd supplies the oracle gradient of the MFCC stage.  TEST INFRASTRUCTURE for tests/test_wave_attacks_*: the
tables come from oracle.mfcc_ref (_polyphase_table, hann_periodic, mel_filterbank, dct_matrix); nothing here is used by
the library.

    y   = R x                      kaiser_best polyphase taps (unfold + per-phase dot) + librosa's appended zero sample
    X_t = rfft(hann * reflect_pad(y, 1024)[512 t : 512 t + 2048]),  t < 1 + n_y // 512
    db  = 10 log10(max(1e-10, W |X|^2)),  thr = max(db) - 80,  c = D max(db, thr)
    out[k L + t] = (c[k, t] - mean) / scale for t < min(T, L), the zero columns of fix_frames standardised like the rest

``dtype=torch.float32`` evaluates the same graph in single precision: the yardstick the GPU parity bounds are built on.
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


def db_22k(y, dtype=torch.float64):
    """[n_y] -> pre-floor dB [T, 128]."""
    y = y.to(dtype)
    yp = torch.nn.functional.pad(y[None, None, :], (M.N_FFT // 2, M.N_FFT // 2), mode="reflect")[0, 0]
    frames = yp.unfold(0, M.N_FFT, M.HOP)
    hann = torch.as_tensor(M.hann_periodic()).to(dtype)
    X = torch.fft.rfft(frames * hann, dim=1)
    P = X.real ** 2 + X.imag ** 2
    W = torch.as_tensor(M.mel_filterbank().astype(np.float64)).to(dtype)
    mel = P @ W.T
    return 10.0 * torch.log10(torch.clamp(mel, min=1e-10))


def features_22k(y, utterance_length=M.STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, dtype=torch.float64):
    """[n_y] at 22 050 Hz -> standardised features [20 * L], coefficient-major."""
    db = db_22k(y, dtype)
    thr = db.max() - 80.0
    D = torch.as_tensor(M.dct_matrix()).to(dtype)
    c = (torch.maximum(db, thr) @ D.T).T  # [20, T]
    T, L = c.shape[1], utterance_length
    c = c[:, :L] if T >= L else torch.cat([c, torch.zeros(c.shape[0], L - T, dtype=dtype)], dim=1)
    out = c.reshape(-1)
    if mean is not None:
        out = (out - torch.as_tensor(mean).to(dtype)) / torch.as_tensor(scale).to(dtype)
    return out


def features(x, sr_in=16000, utterance_length=M.STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, dtype=torch.float64, domain="input"):
    """domain="input": x at sr_in; "22k": x is already the 22 050 Hz signal."""
    y = x.to(dtype) if domain == "22k" else resample(x, sr_in, dtype)
    return features_22k(y, utterance_length, mean, scale, dtype)


def vjp(x, g_feat, sr_in=16000, utterance_length=M.STANDARD_UTTERANCE_LENGTH, scale=None, dtype=torch.float64, domain="input"):
    """Gradient of <features(x), g_feat> w.r.t. x (NumPy in, NumPy float64 out), the graph evaluated in ``dtype``."""
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype).requires_grad_(True)
    f = features(xt, sr_in, utterance_length, None if scale is None else np.zeros_like(np.asarray(scale)), scale, dtype, domain)
    (f * torch.as_tensor(np.asarray(g_feat, dtype=np.float64)).to(dtype)).sum().backward()
    return xt.grad.detach().to(torch.float64).numpy()


def guard_margins(y22):
    """(distance of the closest pre-floor dB element to the top_db floor, gap between the two largest), in dB, float64."""
    with torch.no_grad():
        db = db_22k(torch.as_tensor(np.asarray(y22, dtype=np.float64))).reshape(-1)
    top = torch.topk(db, 2).values
    return float((db - (top[0] - 80.0)).abs().min()), float(top[0] - top[1])


# ---- the parity clips: four non-stationary analytic signals at three lengths (33, 44 and 54 frames against L = 44) ----
LENGTHS = (12000, 16000, 20000)
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
