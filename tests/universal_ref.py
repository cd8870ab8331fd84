"""Oracle of the universal perturbation (lipasr_universal_shifts / _apply / _reduce / _step, their host twins,
lipasr.universal.UniversalPerturbation): a NumPy restatement.  TEST INFRASTRUCTURE for tests/test_universal_*: nothing here is used
by the library.

    shifts        the Philox draw of one shift per row (include/lipasr.h, lipasr_universal_shifts)
    apply         clamp(x + noise[(k + offs) mod P]) inside n_valid, x's bits beyond, in float32
    reduce        the gradient rows summed back onto the period, float64, in the stated order: groups of 64 rows, rows ascending,
                  positions ascending
    total         the group partials added in ascending group order
    step          one lipasr_universal_step: norm inf in float32 (exact); norm 2 in ``dtype`` -- float64 is the reference, float32
                  the yardstick the device's error is measured against
    fit           the driver's loop over any ``grad`` and ``predict``

shifts, apply, reduce and step under norm inf are integer arithmetic, single fp32 additions, clamps and fp64 additions in a fixed
order: the tests compare bits.
"""
from __future__ import annotations

import numpy as np

from philox_ref import nv as _row_nv, philox

GROUP = 64
TAG = 0x554E4956
EVAL_IT = 1 << 23
TOL = 1e-7


def shifts(batch, P, it, seed, clip0=0):
    """int32 [batch]: (o[0] * P) >> 32 of the block with counter words (clip0 + b, 0, it, TAG)."""
    return np.array([(philox(seed, clip0 + b, it, TAG)[0] * P) >> 32 for b in range(batch)], dtype=np.int32)


def _off(offs, b, P):
    return 0 if offs is None else int(offs[b]) % P  # Python's % is already in [0, P)


def clamp(v, lo, hi):
    lo, hi = np.asarray(lo, dtype=v.dtype), np.asarray(hi, dtype=v.dtype)
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(v.dtype)


def apply(x, noise, offs=None, n_valid=None, lo=-np.inf, hi=np.inf):
    x, noise = np.asarray(x, dtype=np.float32), np.asarray(noise, dtype=np.float32)
    B, n = x.shape
    P = noise.shape[0]
    out = x.copy()
    k = np.arange(n)
    for b in range(B):
        nv = _row_nv(n_valid, b, n)
        with np.errstate(invalid="ignore"):
            v = clamp((x[b] + noise[(k + _off(offs, b, P)) % P]).astype(np.float32), lo, hi)
        out[b, :nv] = v[:nv]
    return out


def reduce(g, P, offs=None, n_valid=None):
    """float64 [ceil(B / 64), P]; the accumulator of every period position starts at +0.0 and takes its terms one by one."""
    g = np.asarray(g, dtype=np.float32)
    B, n = g.shape
    sums = np.zeros(((B + GROUP - 1) // GROUP, P), dtype=np.float64)
    p = np.arange(P)
    for b in range(B):
        acc = sums[b // GROUP]
        nv = _row_nv(n_valid, b, n)
        k = (p - _off(offs, b, P)) % P
        while True:
            live = k < nv
            if not live.any():
                break
            v = g[b, np.where(live, k, 0)].astype(np.float64)
            acc += np.where(live & ~np.isnan(v), v, 0.0)  # + 0.0 leaves an accumulator that started at +0.0 as it is
            k = k + P
    return sums


def total(sums):
    G = np.zeros(sums.shape[1], dtype=sums.dtype)
    for grp in range(sums.shape[0]):
        with np.errstate(invalid="ignore"):
            G = G + sums[grp]
    return G


def step(noise, sums, norm, alpha, eps, dtype=np.float64):
    """-> the new noise: float32 under norm inf; under norm 2 an array of ``dtype`` (float64: NOT yet rounded to float32)."""
    noise = np.asarray(noise, dtype=np.float32)
    G = total(np.asarray(sums, dtype=np.float64))
    if norm == np.inf:
        s = np.where(G > 0, np.float32(1), np.where(G < 0, np.float32(-1), np.float32(0))).astype(np.float32)
        return clamp((noise + np.float32(alpha) * s).astype(np.float32), -np.float32(eps), np.float32(eps))
    t = dtype
    G = G.astype(t)
    with np.errstate(over="ignore", invalid="ignore"):
        N = np.sqrt((G * G).sum(dtype=t))
        d = noise.astype(t)
        if np.isfinite(N):
            d = d + (t(np.float32(alpha)) * G) / (N + t(TOL))
        M = np.sqrt((d * d).sum(dtype=t))
        scale = t(1.0)
        if np.float32(eps) < np.inf:
            r = t(np.float32(eps)) / (M + t(TOL))
            scale = r if r < 1 else t(1.0)
        return (d * scale).astype(t)


def fit(grad, predict, x, labels, eps, eps_step, max_iter, batch_size, norm=np.inf, delta=0.2, targeted=False, P=None, random_shift=False,
        seed=0, n_valid=None, lo=-np.inf, hi=np.inf):
    """UniversalPerturbation.generate over ``grad(xa, labels) -> float32 [b, n]`` and ``predict(xa) -> logits [b, classes]`` ->
    dict(noise float32 [P], fooling_rate, converged, epochs)."""
    x = np.asarray(x, dtype=np.float32)
    B, n = x.shape
    P = n if P is None else P
    labels = np.asarray(labels)
    noise = np.zeros(P, dtype=np.float32)
    alpha = -eps_step if targeted else eps_step
    cut = lambda a, s: None if a is None else a[s:s + batch_size]
    rate, converged, epochs = 0.0, False, 0
    for epoch in range(max_iter):
        offs = shifts(B, P, epoch, seed) if random_shift else None
        for s in range(0, B, batch_size):
            xa = apply(x[s:s + batch_size], noise, cut(offs, s), cut(n_valid, s), lo, hi)
            g = np.asarray(grad(xa, labels[s:s + batch_size]), dtype=np.float32)
            noise = step(noise, reduce(g, P, cut(offs, s), cut(n_valid, s)), norm, alpha, eps).astype(np.float32)
        epochs = epoch + 1
        eval_offs = shifts(B, P, EVAL_IT + epoch, seed) if random_shift else None
        pred = np.asarray(predict(apply(x, noise, eval_offs, n_valid, lo, hi))).argmax(axis=1)
        rate = float(np.mean(pred == labels if targeted else pred != labels))
        if rate >= 1.0 - delta:
            converged = True
            break
    return dict(noise=noise, fooling_rate=rate, converged=converged, epochs=epochs)
