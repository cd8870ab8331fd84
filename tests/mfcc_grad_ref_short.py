"""Differentiable float64 restatement of the SHORT-WINDOW MFCC forward (oracle.mfcc_ref.mfcc_22k with n_fft = win_length and hop
as parameters; include/lipasr.h, lipasr_mfcc_plan_ex) in torch, so that autograd supplies the oracle gradient of that stage.
TEST INFRASTRUCTURE for tests/test_short_vjp_*: the tables come from oracle.mfcc_ref (hann_periodic, mel_filterbank(n_fft=),
dct_matrix), the resampler from tests/mfcc_grad_ref.py; nothing here is used by the library.

    X_t = rfft(hann_N * reflect_pad(y, N // 2)[hop t : hop t + N]),  t < 1 + (n_y + 2 (N // 2) - N) // hop
    db  = 10 log10(max(1e-10, W_N |X|^2)),  thr = max(db) - 80,  c = D max(db, thr)
    out[k L + t] = (c[k, t] - mean) / scale for t < min(T, L), the zero columns of fix_frames standardised like the rest

``dtype=torch.float32`` evaluates the same graph in single precision: the yardstick the GPU parity bounds are built on.
"""
from __future__ import annotations

import numpy as np
import torch

import mfcc_grad_ref as G
from oracle import mfcc_ref as M

SR = M.SR_TARGET


def db_22k(y, n_fft, hop, dtype=torch.float64):
    """[n_y] -> pre-floor dB [T, 128]."""
    y = y.to(dtype)
    yp = torch.nn.functional.pad(y[None, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    frames = yp.unfold(0, n_fft, hop)
    hann = torch.as_tensor(M.hann_periodic(n_fft)).to(dtype)
    X = torch.fft.rfft(frames * hann, dim=1)
    P = X.real ** 2 + X.imag ** 2
    W = torch.as_tensor(M.mel_filterbank(n_fft=n_fft).astype(np.float64)).to(dtype)
    mel = P @ W.T
    return 10.0 * torch.log10(torch.clamp(mel, min=1e-10))


def features_22k(y, n_fft, hop, utterance_length, mean=None, scale=None, dtype=torch.float64):
    """[n_y] at 22 050 Hz -> standardised features [20 * L], coefficient-major."""
    db = db_22k(y, n_fft, hop, dtype)
    thr = db.max() - 80.0
    D = torch.as_tensor(M.dct_matrix()).to(dtype)
    c = (torch.maximum(db, thr) @ D.T).T  # [20, T]
    T, L = c.shape[1], utterance_length
    c = c[:, :L] if T >= L else torch.cat([c, torch.zeros(c.shape[0], L - T, dtype=dtype)], dim=1)  # M.fix_frames
    out = c.reshape(-1)
    if mean is not None:
        out = (out - torch.as_tensor(mean).to(dtype)) / torch.as_tensor(scale).to(dtype)
    return out


def features(x, n_fft, hop, utterance_length, sr_in=SR, mean=None, scale=None, dtype=torch.float64, domain="22k"):
    """domain="22k": x is the 22 050 Hz signal; "input": x at sr_in, resampled by tests/mfcc_grad_ref.resample first."""
    y = x.to(dtype) if domain == "22k" else G.resample(x, sr_in, dtype)
    return features_22k(y, n_fft, hop, utterance_length, mean, scale, dtype)


def vjp(x, g_feat, n_fft, hop, utterance_length, sr_in=SR, scale=None, dtype=torch.float64, domain="22k"):
    """Gradient of <features(x), g_feat> w.r.t. x (NumPy in, NumPy float64 out), the graph evaluated in ``dtype``."""
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype).requires_grad_(True)
    f = features(xt, n_fft, hop, utterance_length, sr_in, None if scale is None else np.zeros_like(np.asarray(scale)), scale, dtype, domain)
    (f * torch.as_tensor(np.asarray(g_feat, dtype=np.float64)).to(dtype)).sum().backward()
    return xt.grad.detach().to(torch.float64).numpy()


def guard_margins(y22, n_fft, hop):
    """(distance of the closest pre-floor dB element to the top_db floor -- over ALL elements, the empty mel bands pinned at -100 dB
    included --, gap between the two largest, number of elements below the floor), float64."""
    with torch.no_grad():
        db = db_22k(torch.as_tensor(np.asarray(y22, dtype=np.float64)), n_fft, hop).reshape(-1)
    top = torch.topk(db, 2).values
    thr = top[0] - 80.0
    return float((db - thr).abs().min()), float(top[0] - top[1]), int((db < thr).sum())


# ---- the parity clips: per shape three non-stationary analytic signals at 22 050 Hz, seeds searched on the CPU so that every
# clip (and every gain it is used at) passes guard_margins with room.  With ~13 k dB elements per 441/220 window a clip whose range
# straddles the 80 dB floor lands within 1e-2 dB of it by chance: about one seed in three passes. ----
SHAPES = ((441, 220, 22050), (400, 160, 4000), (510, 510, 2040), (64, 32, 1000), (32, 7, 300))
CLIP_NAMES = ("chirp_gated_noise", "voiced", "noise")
# (seed of the chirp + gated noise clip, seed of the voiced clip, seed of the noise clip) per shape
CLIP_SEEDS = {
    (441, 220, 22050): (7, 1, 0),  # 7372 floored elements (the pinned bands among them), 5, and none
    (400, 160, 4000): (0, 0, 0),
    (510, 510, 2040): (0, 0, 0),
    (64, 32, 1000): (0, 15, 0),
    (32, 7, 300): (0, 2, 0),
}
# the gains a batch repeats the clips at.  A gain g shifts every dB value by 20 log10 g; the noise clip is quiet on purpose: its
# maximum stays below -20 dB, so that the empty mel bands (pinned at -100 dB) lie ABOVE its floor and it has no floored element.
GAINS = (1.0, 0.5, 0.7, 0.35, 0.85)


def make_clip(kind, n, seed):
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


def parity_clips(n_fft, hop, n_samp):
    """[3, n_samp] float32 in CLIP_NAMES order."""
    seeds = CLIP_SEEDS[(n_fft, hop, n_samp)]
    return np.stack([make_clip(k, n_samp, s) for k, s in zip(CLIP_NAMES, seeds)]).astype(np.float32)


def parity_batch(n_fft, hop, n_samp, batch):
    """[batch, n_samp] float32: row i is clip i % 3 at gain GAINS[i // 3]."""
    c = parity_clips(n_fft, hop, n_samp)
    return np.stack([(np.float32(GAINS[i // 3]) * c[i % 3]).astype(np.float32) for i in range(batch)])


# the clips of the domain-"input" test: 16 000 samples at 16 kHz (the same generators; their time axis is then 1.378 x slower), seeds
# searched so that the RESAMPLED signal (oracle.mfcc_ref.librosa_load_resample, 22 050 samples) passes guard_margins at 441/220
INPUT_RATE, INPUT_SAMPLES = 16000, 16000
INPUT_SEEDS = (104, 100, 100)


def input_rate_clips():
    """[3, 16000] float32 in CLIP_NAMES order."""
    return np.stack([make_clip(k, INPUT_SAMPLES, s) for k, s in zip(CLIP_NAMES, INPUT_SEEDS)]).astype(np.float32)
