"""Oracle of randomized smoothing (lipasr_smooth_expand, lipasr_smooth_vote, lipasr_smooth_noise_host, lipasr.smoothing.Smooth): a
float64 restatement.  TEST INFRASTRUCTURE for tests/test_smoothing_*: nothing here is used by the library.

    philox4x32      philox_ref.philox_np: key = seed, counter = (ctr low, ctr high, hi0, hi1)
    normal          the Box-Muller of normal4 on one block per four elements, counter (k >> 2, 0, clip, draw): the uniforms are the
                    kernel's ((x >> 8) + 1) / 2^24, exact in both precisions; log, sqrt, cos and sin are float64 and 2 pi is exact
    expand          clamp(x + sigma z) below n_valid, x behind it                       (include/lipasr.h, lipasr_smooth_expand)
    vote            argmax histogram per clip, lowest index on a tie, NaN rows in the extra bin       (lipasr_smooth_vote)
    cp_lower        scipy.stats.beta.ppf(alpha, k, n - k + 1)
    certify         Cohen, Rosenfeld, Kolter 2019, CERTIFY, over any ``classify`` (float64 rows -> logits) and any ``noise`` source
"""
from __future__ import annotations

import numpy as np

from philox_ref import MASK, philox_np


def philox4x32(seed, ctr, hi0, hi1):
    """ctr: uint64 array [m] -> uint64 array [4, m] of 32-bit words (philox_ref.philox_np with the counter's two halves)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    return philox_np(int(seed), ctr, ctr >> np.uint64(32), int(hi0) & MASK, int(hi1) & MASK)


def normal(seed, clip, draw, n):
    """float64 [n]: z[k] = normal4(seed, k >> 2, clip, draw)[k & 3]."""
    quads = (n + 3) // 4
    o = philox4x32(seed, np.arange(quads, dtype=np.uint64), clip, draw)
    u = ((o >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0  # (0, 1]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    t0, t1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1).reshape(-1)
    return z[:n]


def noise_block(seed, batch, draws, n, clip0=0, draw0=0, noise=normal):
    """float64 [batch * draws, n], row b * draws + j = noise(seed, clip0 + b, draw0 + j, n)."""
    return np.stack([np.asarray(noise(seed, clip0 + b, draw0 + j, n), dtype=np.float64) for b in range(batch) for j in range(draws)]) \
        if batch * draws else np.zeros((0, n))


def expand(x, draws, sigma, seed, clip0=0, draw0=0, n_valid=None, lo=-np.inf, hi=np.inf, noise=normal):
    """x [B, n] -> (out float64 [B * draws, n], valid bool [B * draws, n]).  Padding positions hold x itself."""
    x = np.asarray(x)
    B, n = x.shape
    nv = np.full(B, n) if n_valid is None else np.clip(np.asarray(n_valid, dtype=np.int64), 0, n)
    z = noise_block(seed, B, draws, n, clip0, draw0, noise)
    xr = np.repeat(x.astype(np.float64), draws, axis=0)
    valid = np.arange(n)[None, :] < np.repeat(nv, draws)[:, None]
    return np.where(valid, np.clip(xr + float(sigma) * z, lo, hi), xr), valid


def vote(logits, batch):
    """[batch * draws, C] -> int64 [batch, C + 1]."""
    logits = np.asarray(logits)
    rows, C = logits.shape
    draws = rows // batch if batch else 0
    bins = np.where(np.isnan(logits).any(axis=1), C, np.argmax(np.where(np.isnan(logits), -np.inf, logits), axis=1))
    return np.stack([np.bincount(bins[b * draws:(b + 1) * draws], minlength=C + 1) for b in range(batch)]) if batch \
        else np.zeros((0, C + 1), dtype=np.int64)


def cp_lower(k, n, alpha):
    from scipy import stats

    return 0.0 if k == 0 else float(stats.beta.ppf(alpha, k, n - k + 1))


def certify(classify, x, sigma, n0, n, alpha, seed=0, noise=normal, chunk=512):
    """CERTIFY per row of x (float64 [B, m]) -> dict(cls, p_lower, radius, counts [B, C], counts_select [B, C])."""
    from scipy import stats

    x = np.asarray(x, dtype=np.float64)
    out = dict(cls=[], p_lower=[], radius=[], counts=[], counts_select=[])
    for b in range(x.shape[0]):
        def counts(first, total):
            acc = None
            for j0 in range(first, first + total, chunk):
                d = min(chunk, first + total - j0)
                rows, _ = expand(x[b:b + 1], d, sigma, seed, clip0=b, draw0=j0, noise=noise)
                v = vote(classify(rows), 1)[0]
                acc = v if acc is None else acc + v
            return acc[:-1]
        sel, est = counts(0, n0), counts(n0, n)
        c_a = int(np.argmax(sel))
        p = cp_lower(int(est[c_a]), n, alpha)
        ok = p > 0.5
        out["cls"].append(c_a if ok else -1)
        out["p_lower"].append(p)
        out["radius"].append(float(sigma) * float(stats.norm.ppf(p)) if ok else 0.0)
        out["counts"].append(est)
        out["counts_select"].append(sel)
    return {k: np.asarray(v) for k, v in out.items()}


# ---- the linear two-class case of the tests: rows at known distances from the boundary
LINEAR_SEED = 0  # the first seed tried: the oracle CERTIFY with the host table's draws gives radius / d = 0.90 .. 0.95 on the six rows
LINEAR_SIGMA = 0.25
LINEAR = dict(n0=64, n=4096, alpha=0.001)


def check_linear(cls, radius, d, want_cls, what="oracle"):
    """The inequalities of the linear case: every row gets its clean class, and 0.8 d <= radius <= d.  The smoothed classifier's
    exact radius is d; the upper inequality fails with probability at most alpha per row for an exact sampler, and in 20 000
    simulated binomial trials per distance the smallest radius / d was 0.82."""
    ratio = np.asarray(radius) / d
    print(f"linear classifier ({what}): distance / sigma {(d / LINEAR_SIGMA).round(4).tolist()} class {np.asarray(cls).tolist()} "
          f"radius / d {ratio.round(4).tolist()}")
    np.testing.assert_array_equal(cls, want_cls)
    assert (ratio >= 0.8).all() and (ratio <= 1.0).all()


def linear_case(seed, sigma, n=880, factors=(1.0, 1.0, 1.5, 1.5, 2.0, 2.0)):
    """One dense layer n -> 2 with glorot weights from ``seed`` and rows at distance factors[i] * sigma from its decision boundary,
    alternating sides -> (W float32 [n, 2], bias float32 [2], x float32 [B, n], d float64 [B]: the distances of the float32 rows,
    cls int [B])."""
    rng = np.random.default_rng(seed)
    lim = np.sqrt(6.0 / (n + 2))
    W = rng.uniform(-lim, lim, size=(n, 2)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(2)).astype(np.float32)
    w = W[:, 0].astype(np.float64) - W[:, 1].astype(np.float64)
    c = float(bias[0]) - float(bias[1])
    nw = np.linalg.norm(w)
    rows = []
    for i, f in enumerate(factors):
        x0 = rng.standard_normal(n)
        x0 -= (x0 @ w + c) / nw ** 2 * w  # on the boundary
        rows.append(x0 + (1 if i % 2 == 0 else -1) * f * sigma * w / nw)
    x = np.asarray(rows).astype(np.float32)
    signed = (x.astype(np.float64) @ w + c) / nw
    return W, bias, x, np.abs(signed), np.where(signed > 0, 0, 1)


def linear_classify(W, bias):
    W64, b64 = W.astype(np.float64), bias.astype(np.float64)
    return lambda rows: rows @ W64 + b64
