"""Universal adversarial perturbations (Moosavi-Dezfooli, Fawzi, Fawzi and Frossard 2017, "Universal adversarial perturbations";
over audio: Vadillo and Santana 2019, "Universal adversarial examples in speech command classification", on Google Speech
Commands, and Neekhara, Hussain, Pandey, Dubnov, McAuley and Koushanfar 2019, "Universal adversarial perturbations for speech
recognition systems"): ONE noise vector, fitted once, that fools the model on rows it has never seen -- over the estimators of
lipasr.estimators.

Every other attack of this package solves a new problem per row.  Here the rows of a minibatch share the perturbation, so the
arithmetic that is new is a broadcast with a shift per row on the way in (lipasr_universal_apply) and a sum ACROSS rows on the way
back (lipasr_universal_reduce: fp64, a fixed order, no atomics -- the same bits on every run, whatever the grid).  The noise has a
period P of its own: equal to the row width, shorter (a snippet that loops) or longer (a row sees a window); with
``random_shift`` every row meets it at a Philox-drawn offset, anew in every epoch, as a loudspeaker that plays whenever the victim
happens to speak.  include/lipasr.h fixes the conventions.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from ._rows import _dev_tensor, check_estimator, clip_pair, labels_device, resolve_clip_values, rows2d
from .estimators import _as_given, _to_dev

GROUP = N.UNIVERSAL_GROUP
EVAL_IT = 1 << 23  # the iteration word of the shifts the fooling rate is measured at: 2^23 + epoch


def _norm(norm):
    if norm in (np.inf, math.inf, "inf"):
        return math.inf
    if norm in (2, 2.0, "2"):
        return 2.0
    raise ValueError(f"norm = {norm!r}: 2 or np.inf")


def _period(noise):
    if not (torch.is_tensor(noise) and noise.is_cuda and noise.dtype == torch.float32 and noise.dim() == 1 and noise.is_contiguous()):
        raise ValueError("noise must be a contiguous float32 device tensor [P]")
    return noise.shape[0]


def _row_ints(b, offs, n_valid):
    if offs is not None:
        _dev_tensor(offs, torch.int32, (b,), "offs")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")


def universal_shifts(batch, P, it, seed, *, clip0=0, device=None, out=None):
    """lipasr_universal_shifts: int32 device tensor [batch], the shifts in [0, P) of rows clip0 .. clip0 + batch - 1 at iteration
    ``it`` -- a function of (seed, row index, it, P) alone."""
    batch = int(batch)
    if out is None:
        out = torch.empty(max(batch, 0), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()) if device is None else device)
    _dev_tensor(out, torch.int32, (batch,), "out")
    if not (0 <= int(it) < 1 << 32 and 0 <= int(clip0) < 1 << 32):
        raise ValueError(f"it = {it}, clip0 = {clip0}: 32-bit counters")
    h = N.get_handle(out.device.index)
    N.check(N.lib.lipasr_universal_shifts(h.h, batch, int(P), int(clip0), int(it), int(seed) & 0xFFFFFFFFFFFFFFFF, N.ptr(out), N.stream_ptr()))
    return out


def universal_apply(x, noise, *, offs=None, n_valid=None, clip_values=None, out=None):
    """lipasr_universal_apply on device tensors: x float32 [B, n], noise float32 [P], offs and n_valid int32 [B] or None -> out
    float32 [B, n] (a new tensor unless given): clamp(x + noise[(k + offs) mod P]) inside each row's n_valid, x's bits beyond."""
    b, n = rows2d(x, "x")
    P = _period(noise)
    _row_ints(b, offs, n_valid)
    out = torch.empty_like(x) if out is None else _dev_tensor(out, torch.float32, (b, n), "out")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x.device.index)
    N.check(N.lib.lipasr_universal_apply(h.h, N.ptr(x), N.ptr(noise), N.ptr(offs), N.ptr(n_valid), b, n, P, lo, hi, N.ptr(out), N.stream_ptr()))
    return out


def universal_reduce(g, P, *, offs=None, n_valid=None, sums=None):
    """lipasr_universal_reduce on device tensors: g float32 [B, n] -> sums float64 [ceil(B / 64), P] (written, never added to): per
    group of 64 rows the fp64 sum of the gradient rows carried back onto the period, rows and positions in ascending order."""
    b, n = rows2d(g, "g")
    P = int(P)
    _row_ints(b, offs, n_valid)
    groups = (b + GROUP - 1) // GROUP
    if sums is None:
        sums = torch.empty(groups, max(P, 0), dtype=torch.float64, device=g.device)
    _dev_tensor(sums, torch.float64, (groups, P), "sums")
    h = N.get_handle(g.device.index)
    N.check(N.lib.lipasr_universal_reduce(h.h, N.ptr(g), N.ptr(offs), N.ptr(n_valid), b, n, P, N.ptr(sums), N.stream_ptr()))
    return sums


def universal_step(noise, sums, norm, alpha, eps):
    """lipasr_universal_step on device tensors, in place on noise float32 [P]; sums float64 [groups, P] as universal_reduce wrote it.
    norm inf: a sign step of ``alpha`` clamped to [-eps, eps]; norm 2: a step of length ``alpha`` along the summed gradient,
    projected onto the ball of radius ``eps``.  alpha < 0 descends; eps = inf does not project."""
    P = _period(noise)
    if not (torch.is_tensor(sums) and sums.is_cuda and sums.dtype == torch.float64 and sums.dim() == 2 and sums.is_contiguous()
            and sums.shape[1] == P):
        raise ValueError(f"sums must be a contiguous float64 device tensor [groups, {P}]")
    h = N.get_handle(noise.device.index)
    N.check(N.lib.lipasr_universal_step(h.h, N.ptr(noise), N.ptr(sums), sums.shape[0], P, _norm(norm), float(alpha), float(eps), N.stream_ptr()))
    return noise


class UniversalPerturbation:
    """ART UniversalPerturbation(classifier, attacker=, delta=, max_iter=, eps=, norm=, batch_size=) and
    TargetedUniversalPerturbation in one class (Moosavi-Dezfooli et al. 2017; over audio Vadillo and Santana 2019, Neekhara et al.
    2019): ONE perturbation for every row, in the L-inf or L2 ball of radius ``eps`` -- over the features of a
    TensorFlowV2Classifier, or over the samples of a WaveformClassifier (either domain; ``lengths=``: the noise is added inside
    each clip and the rest of a row comes back bit for bit; a short-window extractor takes no lengths) or an OverTheAirClassifier.

    ``attacker``: "pgd" is the only value.  ART's default runs DeepFool clip after clip, each run starting from the noise the clip
    before it left -- a sequence that cannot be batched.  What is built is the minibatch form: projected gradient steps on the
    loss summed over a minibatch, as in Shafahi, Najibi, Xu, Dickerson, Davis and Goldstein 2020 ("Universal adversarial
    training") and Mummadi, Brox and Metzen 2019 ("Defending against universal perturbations with shared adversarial
    training").  ``delta``: stop once the fooling rate reaches 1 - delta.  ``max_iter``: passes over the rows at most.
    ``eps_step``: the step per minibatch, None: eps / 10.  ``norm``: np.inf or 2.  ``targeted``: y holds the class to reach
    (required then) and the steps descend.  ``length``: the period P of the noise, None: the row width; shorter loops, longer
    shows each row a window.  ``random_shift``: every row meets the noise at an offset drawn per (seed, row index, epoch).
    ``clip_values``: (lo, hi) clamps the perturbed rows; default: the estimator's.

    The algorithm, exactly (tests/universal_ref.py restates it):

        noise = 0;  y = own labels at x (one pass, untargeted) or the targets;  bs = min(batch_size, estimator.batch_limit)
        for epoch in 0 .. max_iter - 1:
            offs_all = universal_shifts(all rows, P, clip0=0, it=epoch, seed)  if random_shift else None   # one launch per epoch
            for every minibatch s of bs rows, in the order given (no shuffling):
                xa   = universal_apply(x[s], noise, offs[s], nv[s], clip)                                # 1 launch
                g    = estimator.loss_gradient_device(xa, y[s], lengths=lt[s])                           # the estimator's passes
                sums = universal_reduce(g, P, offs[s], nv[s])                                            # 1 launch
                universal_step(noise, sums, norm, +-eps_step, eps)                                       # 1 launch
            fooling_rate = share of rows with argmax(apply(x, noise, eval offs)) != own label (targeted: == target)
                eval offs: None, or with random_shift a fresh draw with it = 2^23 + epoch
            if fooling_rate >= 1 - delta: converged = True; stop

    generate / generate_device return the rows with the fitted noise applied at shift 0 and leave behind ``noise_`` (float32
    device tensor [P]), ``noise`` (its NumPy copy), ``fooling_rate``, ``converged`` and ``epochs_``.  ``apply`` puts the fitted
    noise on rows the fit never saw."""

    _UNSET = object()
    _SEED = 0x0A11C11200000000  # no Philox counter is shared with the other attacks

    def __init__(self, estimator, attacker="pgd", delta=0.2, max_iter=20, eps=10.0, eps_step=None, norm=np.inf, batch_size=32,
                 targeted=False, length=None, random_shift=False, seed=None, clip_values=_UNSET):
        check_estimator(estimator)
        if attacker != "pgd":
            raise ValueError(f"attacker = {attacker!r}: only 'pgd' is built -- ART's default, one DeepFool run per clip in sequence, "
                             "cannot be batched")
        self.estimator, self.attacker = estimator, "pgd"
        self.delta, self.max_iter, self.eps = float(delta), int(max_iter), float(eps)
        if not 0.0 <= self.delta <= 1.0:
            raise ValueError(f"delta = {delta}: a share in [0, 1]")
        if not 1 <= self.max_iter <= EVAL_IT:
            raise ValueError(f"max_iter = {max_iter}: 1 to 2^23")
        if not self.eps >= 0.0:
            raise ValueError(f"eps = {eps}: a non-negative number (inf: no projection)")
        self.eps_step = self.eps / 10.0 if eps_step is None else float(eps_step)
        if not 0.0 <= self.eps_step < math.inf:
            raise ValueError(f"eps_step = {self.eps_step}: finite and not negative")
        self.norm = _norm(norm)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size = {batch_size}: at least 1")
        self.targeted, self.random_shift = bool(targeted), bool(random_shift)
        self.length = None if length is None else int(length)
        if self.length is not None and not 1 <= self.length <= 1 << 17:
            raise ValueError(f"length = {length}: 1 to 2^17")
        self.seed = (self._SEED + int(seed or 0)) & 0xFFFFFFFFFFFFFFFF
        self.clip_values = resolve_clip_values(estimator, clip_values, UniversalPerturbation._UNSET)
        self.noise_ = self.noise = None
        self.fooling_rate, self.converged, self.epochs_ = 0.0, False, 0

    def _positions(self, lt):
        return None if lt is None else self.estimator.clip_positions(lt).to(torch.int32).contiguous()

    def _predict(self, xt, lt, nv, offs, bs):
        """argmax of the estimator at the rows with the noise applied, chunk by chunk."""
        out = []
        for s in range(0, xt.shape[0], bs):
            cut = lambda t: None if t is None else t[s:s + bs]
            xa = universal_apply(xt[s:s + bs], self.noise_, offs=cut(offs), n_valid=cut(nv), clip_values=self.clip_values)
            out.append(self.estimator.predict_device(xa, logits=True, lengths=cut(lt)).argmax(dim=1))
        return torch.cat(out)

    def generate_device(self, xt, yt=None, lengths=None):
        """xt: float32 device tensor [B, features or samples]; yt: one-hot [B, classes] or class indices [B] or None; returns a NEW
        device tensor: the rows with the fitted noise applied at shift 0."""
        est = self.estimator
        xt = est.rows_device(xt)
        b, n = xt.shape
        dev = xt.device
        lt = est.lengths_device(lengths, b)
        nv = self._positions(lt)
        P = n if self.length is None else self.length
        bs = min(self.batch_size, int(est.batch_limit))
        self.noise_ = torch.zeros(P, device=dev)
        self.fooling_rate, self.converged, self.epochs_ = 0.0, False, 0
        if b == 0 or n == 0:
            self.noise = self.noise_.cpu().numpy()
            return xt.clone()
        cut = lambda t, s: None if t is None else t[s:s + bs]
        own = lambda: torch.cat([est.predict_device(xt[s:s + bs], logits=True, lengths=cut(lt, s)).argmax(dim=1) for s in range(0, b, bs)])
        labels = labels_device(xt, yt, self.targeted, own).long()
        onehot = torch.nn.functional.one_hot(labels.clamp(0, est.nb_classes - 1), est.nb_classes).to(torch.float32).contiguous()
        alpha = -self.eps_step if self.targeted else self.eps_step
        xa = torch.empty(min(b, bs), n, device=dev)
        g = torch.empty(min(b, bs), n, device=dev)
        sums = torch.empty((min(b, bs) + GROUP - 1) // GROUP, P, dtype=torch.float64, device=dev)
        for epoch in range(self.max_iter):
            offs = universal_shifts(b, P, epoch, self.seed, device=dev) if self.random_shift else None
            for s in range(0, b, bs):
                x = xt[s:s + bs]
                bb = x.shape[0]
                groups = (bb + GROUP - 1) // GROUP
                universal_apply(x, self.noise_, offs=cut(offs, s), n_valid=cut(nv, s), clip_values=self.clip_values, out=xa[:bb])
                est.loss_gradient_device(xa[:bb], onehot[s:s + bb], out=g[:bb], lengths=cut(lt, s))
                universal_reduce(g[:bb], P, offs=cut(offs, s), n_valid=cut(nv, s), sums=sums[:groups])
                universal_step(self.noise_, sums[:groups], self.norm, alpha, self.eps)
            self.epochs_ = epoch + 1
            eval_offs = universal_shifts(b, P, EVAL_IT + epoch, self.seed, device=dev) if self.random_shift else None
            pred = self._predict(xt, lt, nv, eval_offs, bs)
            self.fooling_rate = float(((pred == labels) if self.targeted else (pred != labels)).double().mean())
            if self.fooling_rate >= 1.0 - self.delta:
                self.converged = True
                break
        self.noise = self.noise_.cpu().numpy()
        return self.apply(xt, lengths=lt)

    def generate(self, x, y=None, lengths=None):
        xt = _to_dev(x)
        yt = None if y is None else (y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y)))
        return _as_given(self.generate_device(xt, yt, lengths), x)

    def apply(self, x, lengths=None, offs=None):
        """The fitted noise on the rows ``x`` (array or tensor, the fitted rows or any others of the estimator's width), at shift 0
        or at ``offs`` (int32 [B], in [0, P)): NumPy in, NumPy out."""
        if self.noise_ is None:
            raise RuntimeError("apply() needs a fitted noise: call generate first")
        est = self.estimator
        xt = est.rows_device(x)
        b = xt.shape[0]
        nv = self._positions(est.lengths_device(lengths, b))
        if offs is not None:
            offs = (offs if torch.is_tensor(offs) else torch.as_tensor(np.asarray(offs).astype(np.int32))).to(device=xt.device, dtype=torch.int32)
            offs = offs.contiguous()
        return _as_given(universal_apply(xt, self.noise_, offs=offs, n_valid=nv, clip_values=self.clip_values), x)
