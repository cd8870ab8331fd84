"""Randomized smoothing (Cohen, Rosenfeld, Kolter 2019, algorithms CERTIFY and PREDICT) over the estimators of lipasr.estimators.

The smoothed classifier g(x) = argmax_c P(f(x + N(0, sigma^2 I)) = c) of ANY base classifier f does not change within the L2 radius
sigma Phi^-1(p_A) of x, p_A a lower bound of the vote share of its majority class.  The reference's black-box experiment
(attacks.py:73-86, 335-339: accuracy under add_white_noise over a grid of sigmas) is the mean of p_A over the test set; CERTIFY
turns the same draws into a guarantee per clip, over MFCC rows and -- where the Lipschitz bound of get_robustness_radius has
nothing to say -- over audio.

Device side, per chunk of at most ``estimator.batch_limit`` noisy rows: lipasr_smooth_expand writes the noisy copies once (Philox
counters keyed by seed, clip, draw and element, so a clip's draws depend on neither its neighbours nor the chunking), the
estimator's ``predict_device(..., logits=True)`` classifies them, lipasr_smooth_vote adds the argmax histogram to [B, C + 1]
int32 counts (the last bin: rows with a NaN).  Host side, on purpose: the Clopper-Pearson bound and the binomial test are B
numbers per call in float64 and the result is returned as NumPy anyway.
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np
import torch

from . import _native as N
from ._rows import clip_pair, rows2d
from .estimators import _Estimator

_PHI_INV = NormalDist().inv_cdf


# ------------------------------------------------------------------------------------------------ host statistics (float64)
def _betacf(a, b, x):
    """The continued fraction of the incomplete beta function (modified Lentz), converging for x < (a + 1) / (a + b + 2)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h


def _betainc(a, b, x):
    """The regularized incomplete beta function I_x(a, b), a, b > 0."""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def cp_lower(k, n, alpha):
    """The one-sided Clopper-Pearson lower bound of a binomial proportion: BetaInv(alpha; k, n - k + 1), the p with
    P(Bin(n, p) >= k) = alpha.  k = 0 gives 0, k = n gives alpha ** (1 / n).  Bisection runs on q = 1 - p (I_q(n - k + 1, k) =
    1 - alpha), where the answer keeps its relative precision when p is close to 1 -- Phi^-1 amplifies an error there."""
    k, n, alpha = int(k), int(n), float(alpha)
    if not (0 <= k <= n and n >= 1):
        raise ValueError(f"cp_lower: k = {k}, n = {n}")
    if not (0.0 < alpha < 1.0):
        raise ValueError(f"cp_lower: alpha = {alpha}")
    if k == 0:
        return 0.0
    if k == n:
        return alpha ** (1.0 / n)
    a, b, want = float(n - k + 1), float(k), 1.0 - alpha
    lo, hi = 0.0, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if _betainc(a, b, mid) < want:
            lo = mid
        else:
            hi = mid
    return 1.0 - 0.5 * (lo + hi)


def binom_p_two_sided(n_a, n_b):
    """The two-sided p-value of n_a successes in n_a + n_b trials under p = 1/2 (PREDICT's test): 2 P(Bin(n, 1/2) <= min(n_a,
    n_b)), and 1 where the two counts are equal or there is no trial."""
    n_a, n_b = int(n_a), int(n_b)
    if n_a < 0 or n_b < 0:
        raise ValueError(f"binom_p_two_sided: counts {n_a}, {n_b}")
    if n_a == n_b:
        return 1.0
    m, n = min(n_a, n_b), n_a + n_b
    return min(1.0, 2.0 * _betainc(float(n - m), float(m + 1), 0.5))


# ------------------------------------------------------------------------------------------------ device entry points
def smooth_expand(x, draws, sigma, seed=0, *, clip0=0, draw0=0, n_valid=None, clip_values=None, out=None):
    """lipasr_smooth_expand on device tensors (include/lipasr.h fixes the conventions): x float32 [B, n] contiguous along its rows,
    n_valid int32 [B] or None -> float32 [B * draws, n], row b * draws + j the copy of row b with draw ``draw0 + j`` of clip
    ``clip0 + b`` added below n_valid[b]."""
    b, n = rows2d(x, "x")
    draws = int(draws)
    if n_valid is not None and (tuple(n_valid.shape) != (b,) or n_valid.dtype != torch.int32 or not n_valid.is_contiguous()):
        raise ValueError(f"n_valid must be a contiguous int32 tensor [{b}]")
    if out is None:
        out = torch.empty(b * max(draws, 0), n, device=x.device)
    elif tuple(out.shape) != (b * draws, n) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor [{b * draws}, {n}]")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x.device.index)
    N.check(N.lib.lipasr_smooth_expand(h.h, N.ptr(x), N.ptr(n_valid), b, n, draws, int(clip0), int(draw0), float(sigma), int(seed), lo, hi,
                                       N.ptr(out), N.stream_ptr()))
    return out


def smooth_vote(logits, batch, counts):
    """lipasr_smooth_vote: float32 logits [batch * draws, classes] -> the argmax histogram of every clip ADDED to the int32
    ``counts`` [batch, classes + 1] (last bin: rows with a NaN)."""
    rows, c = rows2d(logits, "logits", "[batch * draws, classes]")
    batch = int(batch)
    if batch < 0 or (batch == 0 and rows) or (batch and rows % batch):
        raise ValueError(f"{rows} rows of logits are no multiple of batch = {batch}")
    if tuple(counts.shape) != (batch, c + 1) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError(f"counts must be a contiguous int32 tensor [{batch}, {c + 1}]")
    h = N.get_handle(logits.device.index)
    N.check(N.lib.lipasr_smooth_vote(h.h, N.ptr(logits), batch, rows // batch if batch else 0, c, N.ptr(counts), N.stream_ptr()))
    return counts


class Smooth:
    """The smoothed classifier g of ``estimator`` under N(0, sigma^2 I): ``certify`` is Cohen's CERTIFY, ``predict`` his PREDICT.
    What is certified is g, NOT the base classifier: g(x + d) = g(x) for every ||d||_2 < radius, with probability at least
    1 - alpha over the draws.  The norm is taken where the noise is added: over the rows of features of a TensorFlowV2Classifier,
    over the samples of a WaveformClassifier (either domain; ``lengths=`` as there: the noise -- and so the guarantee -- covers
    each clip's own positions in its row, the rest of the row stays as it is; a short-window extractor takes no lengths).
    ``seed``: the Philox key; a clip's draws are a function of (seed, its row index in x, draw index, element).
    ``clip_values``: (lo, hi) clamps the noisy rows; the clamp then counts as the base classifier's first stage, and the guarantee
    holds for that composition.  None (default): no clamp."""

    def __init__(self, estimator, sigma, *, seed=0, clip_values=None):
        if not isinstance(estimator, _Estimator):
            raise TypeError("estimator must be a lipasr TensorFlowV2Classifier or WaveformClassifier")
        if not (0.0 <= float(sigma) < math.inf):
            raise ValueError(f"sigma = {sigma}: a finite, non-negative number is required")
        if not 1 <= estimator.nb_classes <= 32:
            raise ValueError(f"{estimator.nb_classes} classes; 1 to 32 are supported")
        if clip_values is not None and not float(clip_values[0]) <= float(clip_values[1]):
            raise ValueError(f"clip_values = {clip_values}")
        self.estimator = estimator
        self.sigma, self.seed = float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.clip_values = None if clip_values is None else (float(clip_values[0]), float(clip_values[1]))

    # ---- device
    def counts_device(self, xt, n, *, draw0=0, lengths=None):
        """The votes of draws [draw0, draw0 + n) for every row of the float32 device tensor ``xt`` [B, features or samples] ->
        int32 device tensor [B, classes + 1] (last bin: noisy rows whose logits held a NaN).  Chunks of at most
        ``estimator.batch_limit`` noisy rows: expand, predict_device(..., logits=True), vote; nothing synchronises."""
        est = self.estimator
        xt = est.rows_device(xt)
        n, draw0 = int(n), int(draw0)
        if n < 0 or draw0 < 0 or draw0 + n > 0xFFFFFFFF:
            raise ValueError(f"draws [{draw0}, {draw0 + n}) are outside the 32-bit counter")
        b, c = xt.shape[0], est.nb_classes
        lt = est.lengths_device(lengths, b)  # as the estimator takes them; pos: the valid positions per row for the expand kernel
        pos = None if lt is None else est.clip_mask(lt).sum(dim=1).to(torch.int32).contiguous()
        counts = torch.zeros(b, c + 1, dtype=torch.int32, device=xt.device)
        if b == 0 or n == 0:
            return counts
        limit = max(1, int(est.batch_limit))
        d_chunk = min(n, limit)
        b_chunk = max(1, limit // d_chunk)
        buf = torch.empty(min(b, b_chunk) * d_chunk, xt.shape[1], device=xt.device)
        for s in range(0, b, b_chunk):
            xb = xt[s:s + b_chunk]
            bb = xb.shape[0]
            for j0 in range(0, n, d_chunk):
                d = min(d_chunk, n - j0)
                noisy = smooth_expand(xb, d, self.sigma, self.seed, clip0=s, draw0=draw0 + j0, n_valid=None if pos is None else pos[s:s + bb],
                                      clip_values=self.clip_values, out=buf[:bb * d])
                z = est.predict_device(noisy, logits=True, lengths=None if lt is None else lt[s:s + bb].repeat_interleave(d))
                smooth_vote(z, bb, counts[s:s + bb])
        return counts

    # ---- Cohen's algorithms
    def certify(self, x, n0=100, n=100_000, alpha=0.001, lengths=None):
        """CERTIFY per row of ``x``: a dict of NumPy arrays [B]
          class          c_A, the majority class of draws [0, n0); -1: abstain (p_lower <= 1/2)
          p_lower        cp_lower(counts[c_A], n, alpha) from the disjoint draws [n0, n0 + n)
          radius         sigma Phi^-1(p_lower) where p_lower > 1/2, else 0
          counts         int64 [B, classes], the votes of the n estimation draws;  counts_select: those of the n0 selection draws
          invalid        the estimation draws whose logits held a NaN: they count in n and for no class, which is conservative."""
        n0, n, alpha = int(n0), int(n), float(alpha)
        if n0 < 1 or n < 1 or not (0.0 < alpha < 1.0):
            raise ValueError(f"certify: n0 = {n0}, n = {n}, alpha = {alpha}")
        xt = self.estimator.rows_device(x)
        c = self.estimator.nb_classes
        sel = self.counts_device(xt, n0, draw0=0, lengths=lengths).cpu().numpy().astype(np.int64)
        est = self.counts_device(xt, n, draw0=n0, lengths=lengths).cpu().numpy().astype(np.int64)
        b = xt.shape[0]
        c_a = sel[:, :c].argmax(axis=1) if b else np.zeros(0, dtype=np.int64)
        p_lower = np.array([cp_lower(est[i, c_a[i]], n, alpha) for i in range(b)], dtype=np.float64)
        ok = p_lower > 0.5
        radius = np.array([self.sigma * _PHI_INV(p) if good else 0.0 for p, good in zip(p_lower, ok)], dtype=np.float64)
        return {"class": np.where(ok, c_a, -1).astype(np.int64), "p_lower": p_lower, "radius": radius, "counts": est[:, :c],
                "counts_select": sel[:, :c], "invalid": est[:, c]}

    def predict(self, x, n=1000, alpha=0.001, lengths=None):
        """PREDICT per row of ``x`` -> int64 NumPy [B]: the class with the most of n votes where the two-sided binomial test of
        its count against the runner-up's rejects a tie at level alpha (binom_p_two_sided(n_A, n_B) <= alpha), else -1."""
        n, alpha = int(n), float(alpha)
        if n < 1 or not (0.0 < alpha < 1.0):
            raise ValueError(f"predict: n = {n}, alpha = {alpha}")
        xt = self.estimator.rows_device(x)
        c = self.estimator.nb_classes
        counts = self.counts_device(xt, n, lengths=lengths).cpu().numpy().astype(np.int64)[:, :c]
        out = np.full(xt.shape[0], -1, dtype=np.int64)
        for i, row in enumerate(counts):
            order = np.argsort(-row, kind="stable")
            n_a, n_b = int(row[order[0]]), int(row[order[1]]) if c > 1 else 0
            if binom_p_two_sided(n_a, n_b) <= alpha:
                out[i] = order[0]
        return out
