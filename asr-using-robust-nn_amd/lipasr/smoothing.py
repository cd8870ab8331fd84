"""Randomized smoothing (Cohen, Rosenfeld, Kolter 2019, algorithms CERTIFY and PREDICT) over the estimators of lipasr.estimators.

The smoothed classifier g(x) = argmax_c P(f(x + N(0, sigma^2 I)) = c) of ANY base classifier f does not change within the L2 radius
sigma Phi^-1(p_A) of x, p_A a lower bound of the vote share of its majority class.  The reference's black-box experiment
(attacks.py:73-86, 335-339: accuracy under add_white_noise over a grid of sigmas) is the mean of p_A over the test set; CERTIFY
turns the same draws into a guarantee per clip, over MFCC rows and -- where the Lipschitz bound of get_robustness_radius has
nothing to say -- over audio.

Training FOR smoothing (the reference trains on clean rows only): GaussianCrossentropy (Cohen et al.: cross-entropy on noisy
copies) and MACERCrossentropy (Zhai et al., ICLR 2020: the certified radius of the soft smoothed classifier, maximised without an
attack) are losses for ``Model.compile``; DESIGN.md, "Training for smoothing".

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
from .keras import CategoricalCrossentropy

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


# ------------------------------------------------------------------------------------------------ training for smoothing
def smooth_loss(logits, label, draws, sigma, lam, gamma, beta, scale, dz, loss, correct=None, radius=None):
    """lipasr_smooth_loss on device tensors (include/lipasr.h fixes the definitions): float32 logits [clips * draws, classes] and
    int32 label [clips] -> dz [clips * draws, classes], loss [clips] and, where given, correct and radius [clips], all float32."""
    rows, c = rows2d(logits, "logits", "[clips * draws, classes]")
    clips, draws = int(label.numel()), int(draws)
    if label.dtype != torch.int32 or not label.is_contiguous() or rows != clips * draws:
        raise ValueError(f"label must be a contiguous int32 tensor [clips] with clips * {draws} = {rows} rows of logits")
    for name, t, shape in (("dz", dz, (rows, c)), ("loss", loss, (clips,)), ("correct", correct, (clips,)), ("radius", radius, (clips,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 tensor {list(shape)}")
    h = N.get_handle(logits.device.index)
    N.check(N.lib.lipasr_smooth_loss(h.h, N.ptr(logits), N.ptr(label), clips, draws, c, float(sigma), float(lam), float(gamma), float(beta),
                                     float(scale), N.ptr(dz), N.ptr(loss), N.ptr(correct), N.ptr(radius), N.stream_ptr()))
    return dz


class GaussianCrossentropy(CategoricalCrossentropy):
    """Gaussian-noise training (Cohen, Rosenfeld, Kolter 2019) as a loss for ``Model.compile``: the cross-entropy of ``draws`` noisy
    copies x + N(0, sigma^2 I) of every row, fresh at every step.  The copies are lipasr_smooth_expand's at clip0 = 0 and draw0 =
    step * draws -- a pure function of (seed, step, row, draw, element) --, the step is the existing lipasr_mlp_train_fwd_bwd on the
    clips * draws rows at inv_batch = 1 / (clips * draws), so it runs in every ``compute_dtype``.  ``fit`` logs the mean loss and
    accuracy of every clip's copies.  ``sigma == 0 and draws == 1`` makes the plain step's calls.  ``clip_values``: (lo, hi) clamps the
    noisy rows, as ``Smooth``'s.  The step counter lives here, on the host: one count per ``train_on_batch``.  ``evaluate`` and ``save``
    of the model stay on plain cross-entropy.  Not built: data parallel, TrainPipeline."""

    name = "gaussian_categorical_crossentropy"
    certified = True  # Model.train_on_batch hands the step to train_step below

    def __init__(self, sigma, draws=1, seed=0, clip_values=None):
        if not (0.0 <= float(sigma) < math.inf):
            raise ValueError(f"sigma = {sigma!r}: a finite number >= 0")
        if not 1 <= int(draws) <= 64 or int(draws) != draws:
            raise ValueError(f"draws = {draws!r}: an integer in [1, 64]")
        if clip_values is not None and not float(clip_values[0]) <= float(clip_values[1]):
            raise ValueError(f"clip_values = {clip_values!r}: low <= high")
        self.sigma, self.draws, self.seed = float(sigma), int(draws), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.clip_values = None if clip_values is None else (float(clip_values[0]), float(clip_values[1]))
        self.step = 0

    def _buffers(self, model, width):
        """The device floats of one step, once per model at its max_batch."""
        buf = getattr(model, "_smooth_buffers", None)
        if buf is None:
            b, dev = model._max_batch, model._device
            c = model._widths[-1]
            buf = {"x": torch.zeros(b, width, device=dev), "logits": torch.zeros(b, c, device=dev), "dz": torch.zeros(b, c, device=dev)}
            model._smooth_buffers = buf
        return buf

    def _expand(self, model, xb):
        """The noisy copies of this step's rows [clips * draws, width] (a view of the model's buffer) and their count."""
        clips = xb.shape[0]
        rows = clips * self.draws
        if rows > model._max_batch:
            raise ValueError(f"{clips} clips x {self.draws} draws = {rows} noisy rows exceed the plan's max_batch {model._max_batch}")
        if self.step * self.draws + self.draws > 0xFFFFFFFF:
            raise ValueError(f"step {self.step} x {self.draws} draws is outside the 32-bit draw counter")
        noisy = self._buffers(model, xb.shape[1])["x"][:rows]
        smooth_expand(xb, self.draws, self.sigma, self.seed, clip0=0, draw0=self.step * self.draws, clip_values=self.clip_values, out=noisy)
        return noisy, rows

    def train_step(self, model, xb, yb, masks=None, dropout=True):
        """One step of ``model`` under this loss; False at sigma == 0 and draws == 1 (the caller then makes the plain step's calls).
        ``masks``: [clips * draws, width] per layer.  Stream-ordered; nothing synchronises."""
        if self.sigma == 0.0 and self.draws == 1:
            self.step += 1
            return False
        clips, m = xb.shape[0], self.draws
        noisy, rows = self._expand(model, xb)
        self.step += 1
        model.train_fwd_bwd(noisy, yb.repeat_interleave(m, dim=0), inv_batch=1.0 / rows, masks=masks, dropout=dropout)
        if m > 1:  # what fit() logs: per clip, the mean over its copies
            for t in (model._loss_rows, model._correct_rows):
                t[:clips] = t[:rows].view(clips, m).mean(dim=1)
        model.apply_adam()
        return True


class MACERCrossentropy(GaussianCrossentropy):
    """MACER (Zhai et al., ICLR 2020) as a loss for ``Model.compile``: per clip, over ``draws`` noisy copies,

        loss = -log mean_j softmax(z_j)_y + lam_t (sigma / 2) max(0, gamma - xi) [the smoothed soft classifier is right],
        xi = Phi^-1(q_y) - Phi^-1(max_{c != y} q_c),  q = mean_j softmax(beta z_j)

    (lipasr_smooth_loss; DESIGN.md, "Training for smoothing").  The step: lipasr_smooth_expand, lipasr_mlp_train_fwd,
    lipasr_smooth_loss at scale 1 / clips, lipasr_mlp_train_bwd, Adam.  lam_t is 0 for the first ``warmup_steps`` steps -- there the
    loss is the cross-entropy of the smoothed soft classifier -- and ``lam`` after.  Built for ``compute_dtype="float32"`` only.
    ``fit`` logs the loss above and the accuracy of the mean softmax.  Not built: data parallel, TrainPipeline."""

    name = "macer_categorical_crossentropy"

    def __init__(self, sigma, draws=16, lam=12.0, gamma=8.0, beta=16.0, warmup_steps=0, seed=0, clip_values=None):
        super().__init__(sigma, draws=draws, seed=seed, clip_values=clip_values)
        if not (0.0 <= float(lam) < math.inf):
            raise ValueError(f"lam = {lam!r}: a finite number >= 0")
        for k, v in (("gamma", gamma), ("beta", beta)):
            if not (0.0 < float(v) < math.inf):
                raise ValueError(f"{k} = {v!r}: a finite number > 0")
        if int(warmup_steps) < 0:
            raise ValueError(f"warmup_steps = {warmup_steps!r}: >= 0")
        self.lam, self.gamma, self.beta, self.warmup_steps = float(lam), float(gamma), float(beta), int(warmup_steps)

    def schedule(self, step):
        """lam_t of the ``step``-th call of train_on_batch, counted from 0."""
        return 0.0 if int(step) < self.warmup_steps else self.lam

    def dz_bound(self, clips, lam_t):
        """A bound of max |dz| for lipasr_mlp_train_bwd.  The classification term is at most 1 / clips per entry (w_j <= 1).  The
        robust term has no bound that holds a priori (a_c grows like 1 / q_c): exact fp32, the only arithmetic this loss runs in,
        ignores the figure."""
        return (1.0 + lam_t * 0.5 * self.sigma * self.beta) / clips

    def train_step(self, model, xb, yb, masks=None, dropout=True):
        """One MACER step of ``model``; always True.  ``masks``: [clips * draws, width] per layer.  Nothing synchronises."""
        if model._compute_dtype != "float32":
            raise NotImplementedError(f"MACERCrossentropy is built for compute_dtype='float32', not {model._compute_dtype!r}: the fp16 "
                                      "planes scale the gradient at the logits by a bound known beforehand, and MACER's robust "
                                      "gradient (sqrt(2 pi) exp(Phi^-1(q)^2 / 2) grows without limit as q -> 0) has none")
        clips, m = xb.shape[0], self.draws
        lam_t = self.schedule(self.step)
        noisy, rows = self._expand(model, xb)
        self.step += 1
        buf = self._buffers(model, xb.shape[1])
        logits, dz = buf["logits"][:rows], buf["dz"][:rows]
        cfg = model._dropout_cfg(masks, dropout)
        N.check(N.lib.lipasr_mlp_train_fwd(model._plan, N.ptr(model._params), N.ptr(model._bnstate), N.ptr(noisy), rows, N.C.byref(cfg),
                                           N.ptr(logits), N.stream_ptr()))
        smooth_loss(logits, yb.argmax(dim=1).to(torch.int32), m, self.sigma, lam_t, self.gamma, self.beta, 1.0 / clips, dz,
                    model._loss_rows[:clips], model._correct_rows[:clips])
        N.check(N.lib.lipasr_mlp_train_bwd(model._plan, N.ptr(model._params), N.ptr(noisy), N.ptr(dz), rows, self.dz_bound(clips, lam_t),
                                           N.C.byref(cfg), N.ptr(model._grads), N.stream_ptr()))
        model.apply_adam()
        return True
