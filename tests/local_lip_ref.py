"""Oracle of the local Lipschitz read-out (lipasr_mlp_jacobian, lipasr_jacobian_sigma, get_local_lipschitz): plumbing over what
the other oracles already state, with no arithmetic of its own beyond an SVD and a faster form of the torch resampler (held to
the existing one by the CPU test).  TEST INFRASTRUCTURE for tests/test_local_lipschitz_*: nothing here is used by the library.

    jacobian        J[b, c, :] = oracle.mlp_ref.output_vjp_infer with the one-hot vector e_c
    audio_jacobian  the same through tests/mfcc_grad_ref.features_22k (behind ``resample`` for rows at the file's rate) and a torch
                    restatement of the classifier's inference forward, one graph and C backward passes over it
                    (``dtype=torch.float32``: the yardstick of the GPU parity bounds)
    sigma_uv        np.linalg.svd in float64 with the sign convention of include/lipasr.h
"""
from __future__ import annotations

import math

import numpy as np
import torch

import mfcc_grad_ref as G
from oracle import mfcc_ref as M, mlp_ref as P


def setup_params(spec, seed):
    """Signed glorot kernels and a non-trivial BatchNorm state: gamma 1 + 0.2 N(0, 1), moving mean 0.2 N(0, 1), moving variance
    U(0.5, 1.5) -- the parameters the attack tests use -> oracle Params (float32)."""
    p = P.init_params(spec, seed=seed, dtype=np.float32, nonneg_init=False)
    rng = np.random.default_rng(seed)
    for l, s in enumerate(spec):
        if s.bn:
            p.gamma[l] = (1 + 0.2 * rng.standard_normal(s.n_out)).astype(np.float32)
            p.mov_mean[l] = (0.2 * rng.standard_normal(s.n_out)).astype(np.float32)
            p.mov_var[l] = rng.uniform(0.5, 1.5, s.n_out).astype(np.float32)
    return p


def jacobian(spec, p64, x, on_logits):
    """[B, n] -> [B, C, n] float64: J[b, c, k] = d out_c(x_b) / d x_b[k] in inference mode."""
    x = np.asarray(x, dtype=np.float64)
    C = spec[-1].n_out
    J = np.zeros((x.shape[0], C, x.shape[1]))
    for c in range(C):
        v = np.zeros((x.shape[0], C))
        v[:, c] = 1.0
        J[:, c] = P.output_vjp_infer(spec, p64, x, v, on_logits=on_logits)[0]
    return J


def outputs(spec, p64, x, on_logits):
    """The function ``jacobian`` differentiates: logits or probabilities [B, C], float64."""
    return P.forward_infer(spec, p64, np.asarray(x, dtype=np.float64), return_logits=bool(on_logits))


def sigma_uv(J):
    """[C, n] -> (sigma, u [C], v [n]) in float64: the largest singular value and its vectors, the component of u of largest
    magnitude positive (lowest index on a tie); a zero matrix gives zeros."""
    J = np.asarray(J, dtype=np.float64)
    if not J.any():
        return 0.0, np.zeros(J.shape[0]), np.zeros(J.shape[1])
    U, S, Vt = np.linalg.svd(J, full_matrices=False)
    u, v = U[:, 0], Vt[0]
    if u[int(np.argmax(np.abs(u)))] < 0:
        u, v = -u, -v
    return float(S[0]), u, v


def sigmas(J):
    """[B, C, n] -> float64 [B]."""
    return np.array([sigma_uv(j)[0] for j in J])


def gram_sigma_f32(J, lanes=256):
    """The device kernel's summation restated on the host: J (float32 [C, n]) scaled by the power of two that brings max |J| into
    [1, 2), the Gram matrix from ``lanes`` lane-serial float32 partial sums (lane l takes columns l, l + lanes, ...) widened to
    float64 and added pairwise (a tree), its largest eigenvalue in float64 -> sigma."""
    J = np.asarray(J, dtype=np.float32)
    mx = float(np.abs(J).max())
    if mx == 0.0:
        return 0.0
    ex = 1 - math.frexp(mx)[1]
    Js = np.ldexp(J, ex).astype(np.float32)
    C, n = Js.shape
    part = np.zeros((lanes, C, C), dtype=np.float32)
    for k0 in range(0, n, lanes):
        blk = Js[:, k0:k0 + lanes]  # column k0 + l belongs to lane l
        w = blk.shape[1]
        b64 = blk.astype(np.float64)
        prod = np.moveaxis(b64[:, None, :] * b64[None, :, :], 2, 0)  # [w, C, C], exact in float64
        part[:w] = (part[:w].astype(np.float64) + prod).astype(np.float32)  # one rounding to float32: a fused multiply-add
    t = part.astype(np.float64)
    while t.shape[0] > 1:
        t = t[0::2] + t[1::2]
    lam = np.linalg.eigvalsh(t[0])[-1]
    return float(np.ldexp(math.sqrt(max(lam, 0.0)), -ex))


def torch_params(p, dtype):
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)
    return dict(W=[t(a) for a in p.W], b=[t(a) for a in p.b], g=[t(a) for a in p.gamma], be=[t(a) for a in p.beta],
                mm=[t(a) for a in p.mov_mean], mv=[t(a) for a in p.mov_var])


def torch_logits(spec, tp, h):
    """oracle.mlp_ref.forward_infer(return_logits=True) written with torch ops, for autograd."""
    for l, s in enumerate(spec):
        z = h @ tp["W"][l] + tp["b"][l]
        if l == len(spec) - 1:
            return z
        h = torch.relu(z)
        if s.bn:
            h = (h - tp["mm"][l]) / torch.sqrt(tp["mv"][l] + P.BN_EPS) * tp["g"][l] + tp["be"][l]
    raise AssertionError


def resample(x, sr_in, dtype=torch.float64):
    """mfcc_grad_ref.resample with ONE gather instead of one indexing per filter phase: the same taps times the same samples
    (tests/test_local_lipschitz_cpu.py holds the two together to rounding), but a backward pass costs 0.05 s instead of 0.7 s --
    audio_jacobian runs one per class and dtype."""
    x = x.to(dtype)
    if sr_in == G.SR:
        return x
    h, n_off, L, Md, wing = M._polyphase_table(sr_in, G.SR)
    n = x.shape[0]
    ratio = float(G.SR) / float(sr_in)
    n_out, n_fixed = int(n * ratio), int(math.ceil(n * ratio))
    nq = (n_out + L - 1) // L
    xp = torch.cat([torch.zeros(wing - 1, dtype=dtype), x, torch.zeros(2 * wing + Md * (nq + 1), dtype=dtype)])
    start = (Md * torch.arange(nq))[:, None] + torch.as_tensor(np.asarray(n_off, dtype=np.int64))[None, :]  # [nq, L]
    taps = start[:, :, None] + torch.arange(2 * wing)[None, None, :]  # xp[start + j] = x[i - 63 + j]
    y = (xp[taps] * torch.as_tensor(h).to(dtype)[None, :, :]).sum(dim=2).reshape(-1)[:n_out]
    if n_fixed > n_out:
        y = torch.cat([y, torch.zeros(n_fixed - n_out, dtype=dtype)])
    return y


def audio_jacobian(spec, p, x, mean, scale, dtype=torch.float64, on_logits=True, n_clip=None, **feat_kw):
    """One row of audio ``x`` [n] -> [C, n] float64: the Jacobian of the classifier's logits (or probabilities) behind the MFCC
    stage, the whole graph evaluated in ``dtype``.  n_clip: the leading positions of the row that belong to its clip (the rest is
    ignored by the extraction: zero columns).  feat_kw: sr_in, domain ("input": x at sr_in, "22k": x at 22 050 Hz) and the
    utterance_length, n_fft, hop of mfcc_grad_ref.features_22k."""
    x = np.asarray(x, dtype=np.float64)
    n_clip = x.shape[0] if n_clip is None else int(n_clip)
    xt = torch.as_tensor(x[:n_clip]).to(dtype).requires_grad_(True)
    feat_kw = dict(feat_kw)
    sr_in, domain = feat_kw.pop("sr_in", 16000), feat_kw.pop("domain", "input")
    y = xt if domain == "22k" else resample(xt, sr_in, dtype)
    f = G.features_22k(y, mean=mean, scale=scale, dtype=dtype, **feat_kw)
    out = torch_logits(spec, torch_params(p, dtype), f[None, :])[0]
    if not on_logits:
        out = torch.softmax(out, dim=0)
    J = np.zeros((out.shape[0], x.shape[0]))
    for c in range(out.shape[0]):
        (g,) = torch.autograd.grad(out[c], xt, retain_graph=True)
        J[c, :n_clip] = g.detach().to(torch.float64).numpy()
    return J
