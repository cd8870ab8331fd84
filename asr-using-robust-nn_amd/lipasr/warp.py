"""The time-warp threat model: the worst case over a small delay, a small change of speed and a small change of level -- the
perturbations a keyword spotter meets every day, none of which is small in any norm (a 10 ms delay of a one-second clip moves it by
about its own L2 norm).  ART's closest name is ``SpatialTransformation`` (Engstrom et al. 2019: the worst of a grid of translations
and rotations of an image); this is the audio form, ours.

    warp_table()                       the interpolation table on the device, float32 [Z P + 1, 2] = (win, delta); cached per device
    warp_apply(x, params, K, ...)      [B, n] -> [B * K, n]: row b * K + j is clip b under the triple params[b * K + j]
    warp_param_vjp(x, g, params, K)    [B * K, n] cotangents -> float64 [B * K, 3]: d sum_t g out / d (shift, rate, gain)
    candidate_grid(...)                the product grid of triples, float64 [K, 3]
    TimeWarp(estimator, max_shift, .)  worst of the grid per clip (scores only), then optional projected sign steps on each clip's
                                       own triple (gradients: loss_gradient_device through the MFCC backward pass, then warp_param_vjp)

A triple is (shift in samples of the row, rate, linear gain): out[t] = gain * x(c + rate (t - c) - shift) with c the clip's centre,
so a positive shift delays, a rate above 1 plays faster, and the word stays where it was.  x(.) is band-limited interpolation
with a Kaiser-windowed sinc whose cutoff is FIXED at Nyquist (include/lipasr.h, lipasr_warp_apply): integer delays reproduce the
samples exactly, and the interpolation is accurate to 4e-5 at 0.8 of Nyquist, 7e-2 at 0.9.  The 22 050 Hz rows of 16 kHz files
hold nothing above 0.73 of Nyquist, and TimeWarp keeps the rate within [0.8, 1.25], so nothing there aliases; a caller with
full-band audio should low-pass to 0.8 of Nyquist over max_rate first -- there is no per-rate anti-aliasing cutoff.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from ._rows import _dev_tensor, check_estimator, generate_host, labels_device, rows2d
from .estimators import WaveformClassifier
from .square import margin_device

Z, P = 16, 512
TABLE = Z * P + 1
MAX_RATE = 1.25  # TimeWarp's limit; the kernel itself takes rates in [0.5, 2]

_tables = {}


def warp_table(device=None):
    """The table of lipasr_warp_table_host on ``device`` (default: the current one), float32 [Z P + 1, 2]: one copy per device."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev not in _tables:
        win, delta = N.warp_table_host()
        _tables[dev] = torch.as_tensor(np.stack([win, delta], axis=1)).to(dev).contiguous()
    return _tables[dev]


def _params(params, rows, dev):
    t = params if torch.is_tensor(params) else torch.as_tensor(np.asarray(params))
    if tuple(t.shape) != (rows, 3):
        raise ValueError(f"params must be [{rows}, 3] = (shift, rate, gain) per output row, got {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _check(x, K, lengths):
    b, n = rows2d(x, "x")
    K = int(K)
    if K < 1:
        raise ValueError(f"K = {K}: at least one candidate per clip")
    if lengths is not None:
        _dev_tensor(lengths, torch.int32, (b,), "lengths")
    return b, n, K


def warp_apply(x, params, K, lengths=None, out=None):
    """lipasr_warp_apply on device tensors: x float32 [B, n]; params [B * K, 3] (any float kind; the kernel reads float32);
    ``lengths``: int32 [B], the POSITIONS of each row that belong to its clip (None: all n) -- the output is 0 from there on;
    ``out``: float32 [B * K, n] or None.  A row whose triple is not finite or whose rate is outside [0.5, 2] comes back as NaN."""
    b, n, K = _check(x, K, lengths)
    p = _params(params, b * K, x.device)
    out = torch.empty(b * K, n, device=x.device) if out is None else _dev_tensor(out, torch.float32, (b * K, n), "out")
    N.check(N.lib.lipasr_warp_apply(N.ptr(x), N.ptr(lengths), N.ptr(p), N.ptr(warp_table(x.device)), b, K, n, N.ptr(out), N.stream_ptr()))
    return out


def warp_param_vjp(x, g, params, K, lengths=None):
    """lipasr_warp_param_vjp on device tensors: x float32 [B, n], g float32 [B * K, n] -> float64 [B * K, 3], the derivative of
    sum_t g[r, t] out[r, t] with respect to row r's (shift, rate, gain)."""
    b, n, K = _check(x, K, lengths)
    _dev_tensor(g, torch.float32, (b * K, n), "g")
    p = _params(params, b * K, x.device)
    gp = torch.empty(b * K, 3, dtype=torch.float64, device=x.device)
    N.check(N.lib.lipasr_warp_param_vjp(N.ptr(x), N.ptr(g), N.ptr(lengths), N.ptr(p), N.ptr(warp_table(x.device)), b, K, n, N.ptr(gp),
                                        N.stream_ptr()))
    return gp


def _axis(half_width, count):
    """``count`` (odd) points from -half_width to half_width, exactly symmetric, the middle exactly 0."""
    half = np.linspace(0.0, float(half_width), (count + 1) // 2)
    return np.concatenate([-half[:0:-1], half])


def candidate_axes(max_shift, max_rate=1.0, max_gain_db=0.0, counts=(9, 3, 3)):
    """The three axes of candidate_grid: shifts linspace(-max_shift, max_shift), rates evenly spaced in the log from 1 / max_rate
    to max_rate, gains evenly spaced in dB from -max_gain_db to max_gain_db (as linear factors)."""
    counts = tuple(int(c) for c in counts)
    if len(counts) != 3 or any(c < 1 or c % 2 == 0 for c in counts):
        raise ValueError(f"counts = {counts}: three odd numbers, so that the identity is always a candidate")
    max_shift, max_rate, max_gain_db = float(max_shift), float(max_rate), float(max_gain_db)
    if not (0.0 <= max_shift < math.inf and 1.0 <= max_rate <= 2.0 and 0.0 <= max_gain_db < math.inf):
        raise ValueError(f"max_shift = {max_shift} (>= 0), max_rate = {max_rate} (1 to 2), max_gain_db = {max_gain_db} (>= 0)")
    return (_axis(max_shift, counts[0]), np.exp(_axis(math.log(max_rate), counts[1])),
            10.0 ** (_axis(max_gain_db, counts[2]) / 20.0))


def candidate_grid(max_shift, max_rate=1.0, max_gain_db=0.0, counts=(9, 3, 3)):
    """float64 [K, 3], K = counts[0] * counts[1] * counts[2]: every (shift, rate, gain) of candidate_axes, the shift slowest and the
    gain fastest -- candidate (i, j, k) sits at index (i * counts[1] + j) * counts[2] + k.  The counts are odd, so the middle
    candidate is the identity (0, 1, 1)."""
    s, r, g = candidate_axes(max_shift, max_rate, max_gain_db, counts)
    return np.stack([a.reshape(-1) for a in np.meshgrid(s, r, g, indexing="ij")], axis=1)


class TimeWarp:
    """TimeWarp(estimator, max_shift, max_rate=1.0, max_gain_db=0.0, counts=(9, 3, 3), refine_steps=0, targeted=False) over a
    WaveformClassifier or an OverTheAirClassifier, in either domain, with ``lengths=``.

    ``max_shift``: the largest delay either way, in SAMPLES OF THE ROW (22 050 Hz rows in domain "22k"); ``max_rate`` in
    [1, 1.25]: speeds from 1 / max_rate to max_rate; ``max_gain_db``: levels from -max_gain_db to +max_gain_db.  The three define the
    box; ``counts`` the grid inside it (candidate_grid).

    generate / generate_device(x, y=None, lengths=None): clips go through in chunks of max(1, batch_limit // K).  Per chunk ONE
    warp_apply, ONE predict_device(logits=True), and per row the margin z_y - max_{k != y} z_k (targeted: max_{k != t} z_k - z_t,
    y the class to reach); per clip the candidate with the smallest margin is kept, ties to the lowest index, a NaN margin never
    over a number.  y=None: the estimator's own predictions.  The grid search uses scores only.
    ``refine_steps`` > 0: that many projected sign steps on each clip's own triple (K = 1): loss_gradient_device at the warped rows,
    warp_param_vjp, a step of 1/4 of each parameter's grid spacing (of the box's half-width where its count is 1) along the sign that
    lowers the margin, clipped to the box; a step is kept only if the margin fell, and a clip whose margin did not fall halves its
    step.
    Returns the warped rows (0 beyond each clip) in the shape and kind given.  Afterwards ``params_`` float64 [B, 3], the triple of
    every returned row (the rows are warp_apply(x, params_, 1) bit for bit), and ``margins_`` float32 [B], device tensors."""

    def __init__(self, estimator, max_shift, max_rate=1.0, max_gain_db=0.0, counts=(9, 3, 3), refine_steps=0, targeted=False):
        check_estimator(estimator, WaveformClassifier, "estimator")
        if not 1.0 <= float(max_rate) <= MAX_RATE:
            raise ValueError(f"max_rate = {max_rate}: 1 to {MAX_RATE} (the interpolation's cutoff is fixed at Nyquist)")
        self.axes = candidate_axes(max_shift, max_rate, max_gain_db, counts)
        self.grid = candidate_grid(max_shift, max_rate, max_gain_db, counts)
        self.estimator, self.targeted, self.refine_steps = estimator, bool(targeted), int(refine_steps)
        if self.refine_steps < 0:
            raise ValueError(f"refine_steps = {refine_steps}: not negative")
        self.K = self.grid.shape[0]
        if self.K > estimator.batch_limit:
            raise ValueError(f"a grid of {self.K} candidates does not fit the estimator's batch_limit {estimator.batch_limit}")
        self.lo = np.array([a[0] for a in self.axes])
        self.hi = np.array([a[-1] for a in self.axes])
        self.step = np.array([0.25 * (a[len(a) // 2 + 1] - a[len(a) // 2]) if len(a) > 1 else 0.125 * (a[-1] - a[0]) for a in self.axes])
        self.params_ = self.margins_ = None

    def _margins(self, est, rows, lt, lab):
        return margin_device(est.predict_device(rows, logits=True, lengths=lt).contiguous(), lab, self.targeted)

    def generate_device(self, xt, yt=None, lengths=None):
        est, K = self.estimator, self.K
        xt = est.rows_device(xt)
        b, n = xt.shape
        dev = xt.device
        lt = est.lengths_device(lengths, b)
        nv = None if lt is None else est.clip_positions(lt).to(torch.int32).contiguous()
        cut = lambda t, sl: None if t is None else t[sl]
        self.params_ = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev).repeat(b, 1)
        self.margins_ = torch.full((b,), math.inf, device=dev)
        if b == 0 or n == 0:
            return xt.clone()
        lab = labels_device(xt, yt, self.targeted, lambda: est.own_labels_device(xt, lengths=lt))
        grid = torch.as_tensor(self.grid, device=dev)
        per = max(1, int(est.batch_limit) // K)
        order = torch.arange(K, device=dev)
        for s in range(0, b, per):
            sl = slice(s, min(s + per, b))
            c = sl.stop - sl.start
            rows = warp_apply(xt[sl], grid.repeat(c, 1), K, lengths=cut(nv, sl))
            m = self._margins(est, rows, None if lt is None else lt[sl].repeat_interleave(K), lab[sl].repeat_interleave(K)).view(c, K)
            m = torch.where(torch.isnan(m), torch.full_like(m, math.inf), m)
            best = m.min(dim=1).values
            pick = torch.where(m == best[:, None], order[None, :], torch.full_like(order, K)[None, :]).min(dim=1).values
            self.params_[sl] = grid[pick]
            self.margins_[sl] = best
        if self.refine_steps:
            self._refine(est, xt, lt, nv, lab)
        return warp_apply(xt, self.params_, 1, lengths=nv)

    def _refine(self, est, xt, lt, nv, lab):
        b, dev = xt.shape[0], xt.device
        lo, hi = (torch.as_tensor(a, device=dev) for a in (self.lo, self.hi))
        step = torch.as_tensor(self.step, device=dev).repeat(b, 1)
        onehot = torch.zeros(b, est.nb_classes, device=dev)
        onehot[torch.arange(b, device=dev), lab.long()] = 1.0
        for _ in range(self.refine_steps):
            rows = warp_apply(xt, self.params_, 1, lengths=nv)
            g = est.loss_gradient_device(rows, onehot, lengths=lt)  # a positive factor per chunk apart; only the sign is used
            gp = warp_param_vjp(xt, g, self.params_, 1, lengths=nv)
            # the margin falls where the loss of the label rises (targeted: where the loss of the target falls)
            d = torch.sign(torch.nan_to_num(gp, nan=0.0, posinf=0.0, neginf=0.0)) * (-1.0 if self.targeted else 1.0)
            cand = torch.minimum(torch.maximum(self.params_ + step * d, lo), hi)
            m = self._margins(est, warp_apply(xt, cand, 1, lengths=nv), lt, lab)
            fell = m < self.margins_  # false for a NaN
            self.params_ = torch.where(fell[:, None], cand, self.params_)
            self.margins_ = torch.where(fell, m, self.margins_)
            step = torch.where(fell[:, None], step, 0.5 * step)

    def generate(self, x, y=None, lengths=None):
        return generate_host(self, x, y, lengths)
