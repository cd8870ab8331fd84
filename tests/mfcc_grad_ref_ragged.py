"""The oracle graph of tests/mfcc_grad_ref.py for clips of ANY length >= 2 resampled samples.  TEST INFRASTRUCTURE for
tests/test_wave_ragged_*: nothing here is used by the library.

torch's reflect pad refuses a clip that is not longer than the padding (n_y <= 1024); np.pad reflects repeatedly.  Here the
padding is an index gather with np.pad's own indices, ``np.pad(np.arange(n_y), 1024, mode="reflect")``, which is valid for any
n_y >= 2 and differentiable (autograd scatters the gradient back through the gather: the general adjoint of the padding).
Everything else -- the resampler, the tables, the dB, floor, DCT and fix_frames steps -- is mfcc_grad_ref's, unchanged.
``dtype=torch.float32`` evaluates the same graph in single precision: the yardstick of the GPU parity bounds.
"""
from __future__ import annotations

import numpy as np
import torch

import mfcc_grad_ref as G
from oracle import mfcc_ref as M

# four clips (mfcc_grad_ref.parity_clips) per length, 16 kHz.  n_y = ceil(n * 1.378125): 1486 -> 2048 (the old limit of the
# backward pass: the two reflected flanks overlap), 1487 -> 2050, 400 and 40 need repeated reflection, 3000 -> 9 frames (a second
# frame group of one unpaired frame), 7000 -> 19 frames, 20000 -> 54 frames > L = 44
LENGTHS = (40, 400, 1000, 1486, 1487, 3000, 7000, 12000, 16000, 20000)


def db_22k(y, dtype=torch.float64):
    """[n_y >= 2] -> pre-floor dB [1 + n_y // 512, 128]."""
    y = y.to(dtype)
    idx = torch.as_tensor(np.pad(np.arange(y.shape[0]), M.N_FFT // 2, mode="reflect"))
    frames = y[idx].unfold(0, M.N_FFT, M.HOP)
    hann = torch.as_tensor(M.hann_periodic()).to(dtype)
    X = torch.fft.rfft(frames * hann, dim=1)
    P = X.real ** 2 + X.imag ** 2
    W = torch.as_tensor(M.mel_filterbank().astype(np.float64)).to(dtype)
    return 10.0 * torch.log10(torch.clamp(P @ W.T, min=1e-10))


def features_22k(y, utterance_length=M.STANDARD_UTTERANCE_LENGTH, mean=None, scale=None, dtype=torch.float64):
    """[n_y] at 22 050 Hz -> standardised features [20 * L], coefficient-major (mfcc_grad_ref.features_22k over db_22k above)."""
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
    y = x.to(dtype) if domain == "22k" else G.resample(x, sr_in, dtype)
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
