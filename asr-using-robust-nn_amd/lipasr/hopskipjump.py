"""HopSkipJump (Chen, Jordan and Wainwright 2020, "HopSkipJumpAttack: a query-efficient decision-based attack"; ART's
``HopSkipJump``) over the estimators of lipasr.estimators: a minimum-norm attack in L2 or L-inf that asks the model one thing only,
"is this point still misclassified?" -- neither a gradient (FGM, PGD, Auto-PGD, DeepFool) nor a score (GeneticAttack, SquareAttack).

Why it is here: a deployed recogniser returns the word and nothing else; it is the L2 side of the query-only check that
``SquareAttack`` (L-inf only) leaves open; and its distance per clip is a cross-check of DeepFool's that rests on no gradient
(``get_robustness_radius(found_by="hopskipjump")``).  One run gives a distance per clip and with it the whole accuracy-versus-eps
curve.

Per clip: a start point that is adversarial (uniform draws in the clip range, or ``x_adv_init``), a bisection towards the clean
row, and then ``max_iter`` times: a Monte-Carlo estimate of the boundary's normal from up to ``max_eval`` perturbed copies
(lipasr_hsj_expand writes them, the estimator's ``predict_device`` classifies them, lipasr_hsj_accumulate adds them up in fp64,
lipasr_hsj_direction normalises), a step whose size is halved until it lands on the adversarial side, and a bisection back to the
boundary (lipasr_hsj_search, ONE launch per query).  The only synchronisation inside a phase is ``active.any()`` every
``check_every`` queries.  Philox counters are keyed by seed, row index, iteration and draw, so a row's run depends on neither its
neighbours nor the chunking.  include/lipasr.h fixes the conventions.  ART and the paper's code are absent here: the algorithm is
restated from memory, parity is unpinned, and every constant is a keyword.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from ._rows import _dev_tensor, check_estimator, clip_pair, generate_host, labels_device, resolve_clip_values, rows2d

START, HALVE, BISECT = N.HSJ_START, N.HSJ_HALVE, N.HSJ_BISECT
FIRST, LAST = N.HSJ_FIRST, N.HSJ_LAST
F, I = N.HSJ_F, N.HSJ_I
MAX_DRAWS = 16384  # per lipasr_hsj_accumulate call


def _norm(norm):
    if norm in (2, 2.0, "2"):
        return 2.0
    if norm in (np.inf, math.inf, "inf"):
        return math.inf
    raise ValueError(f"norm = {norm!r}: 2 and np.inf are supported")


def hsj_expand(x, delta, draws, it, seed, norm, *, out, n_valid=None, clip0=0, draw0=0, clip_values=None):
    """lipasr_hsj_expand on device tensors: x float32 [B, n], delta float32 [B] -> out float32 [B * draws, n], row b * draws + j the
    copy ``draw0 + j`` of clip ``clip0 + b`` at iteration ``it``."""
    b, n = rows2d(x, "x")
    draws = int(draws)
    _dev_tensor(delta, torch.float32, (b,), "delta")
    _dev_tensor(out, torch.float32, (b * draws, n), "out")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    if not 0 <= int(it) < 1 << 24:
        raise ValueError(f"it = {it}: 0 to 2^24 - 1")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x.device.index)
    N.check(N.lib.lipasr_hsj_expand(h.h, N.ptr(x), N.ptr(delta), N.ptr(n_valid), b, n, draws, int(clip0), int(it), int(draw0),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, _norm(norm), lo, hi, N.ptr(out), N.stream_ptr()))
    return out


def hsj_accumulate(logits, labels, p, x, *, sums, counts, n_valid=None, targeted=False):
    """lipasr_hsj_accumulate on device tensors, in place on sums float64 [B, 2, n] and counts int32 [B, 2]: logits float32
    [B * draws, classes] at the rows p float32 [B * draws, n] around x float32 [B, n]; labels int32 [B]."""
    b, n = rows2d(x, "x")
    rows2d(p, "p")
    if p.shape[1] != n or (b and p.shape[0] % b):
        raise ValueError(f"p must be [{b} * draws, {n}], got {tuple(p.shape)}")
    draws = p.shape[0] // b if b else 0
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
            and logits.shape[0] == p.shape[0]):
        raise ValueError(f"logits must be a contiguous float32 device tensor [{p.shape[0]}, classes]")
    _dev_tensor(labels, torch.int32, (b,), "labels")
    _dev_tensor(sums, torch.float64, (b, 2, n), "sums")
    _dev_tensor(counts, torch.int32, (b, 2), "counts")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    h = N.get_handle(x.device.index)
    N.check(N.lib.lipasr_hsj_accumulate(h.h, N.ptr(logits), N.ptr(labels), N.ptr(p), N.ptr(x), N.ptr(n_valid), b, logits.shape[1], n, draws,
                                        1 if targeted else 0, N.ptr(sums), N.ptr(counts), N.stream_ptr()))


def hsj_direction(sums, counts, norm, *, u, n_valid=None):
    """lipasr_hsj_direction on device tensors: sums float64 [B, 2, n], counts int32 [B, 2] -> u float32 [B, n]."""
    if not (torch.is_tensor(sums) and sums.is_cuda and sums.dtype == torch.float64 and sums.dim() == 3 and sums.shape[1] == 2
            and sums.is_contiguous()):
        raise ValueError("sums must be a contiguous float64 device tensor [B, 2, n]")
    b, _, n = sums.shape
    _dev_tensor(counts, torch.int32, (b, 2), "counts")
    _dev_tensor(u, torch.float32, (b, n), "u")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    h = N.get_handle(sums.device.index)
    N.check(N.lib.lipasr_hsj_direction(h.h, N.ptr(sums), N.ptr(counts), N.ptr(n_valid), b, n, _norm(norm), N.ptr(u), N.stream_ptr()))
    return u


def hsj_search(logits, labels, x0, mode, flags, seed, norm, *, x_cand, x_far, x_adv, x_best, fstate, istate, start_lo, start_hi, theta,
               u=None, n_valid=None, targeted=False, clip0=0, draw=0, step_scale=1.0, max_halvings=25, clip_values=None, classes=None):
    """lipasr_hsj_search on device tensors, in place: logits float32 [B, classes] at x_cand (None under FIRST, then ``classes`` says
    how many), labels int32 [B], the five row buffers float32 [B, n], fstate float32 [B, 8] and istate int32 [B, 8] (columns:
    lipasr._native.HSJ_F, HSJ_I), start_lo, start_hi, theta float32 [B]."""
    b, n = rows2d(x0, "x0")
    if logits is not None:
        if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
                and logits.shape[0] == b):
            raise ValueError(f"logits must be a contiguous float32 device tensor [{b}, classes]")
        classes = logits.shape[1]
    elif not int(flags) & FIRST:
        raise ValueError("logits are required outside FIRST")
    _dev_tensor(labels, torch.int32, (b,), "labels")
    for t, what in ((x_cand, "x_cand"), (x_far, "x_far"), (x_adv, "x_adv"), (x_best, "x_best")):
        _dev_tensor(t, torch.float32, (b, n), what)
    if u is not None:
        _dev_tensor(u, torch.float32, (b, n), "u")
    _dev_tensor(fstate, torch.float32, (b, 8), "fstate")
    _dev_tensor(istate, torch.int32, (b, 8), "istate")
    for t, what in ((start_lo, "start_lo"), (start_hi, "start_hi"), (theta, "theta")):
        _dev_tensor(t, torch.float32, (b,), what)
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x0.device.index)
    N.check(N.lib.lipasr_hsj_search(h.h, N.ptr(logits), N.ptr(labels), N.ptr(x0), N.ptr(n_valid), N.ptr(u), N.ptr(start_lo), N.ptr(start_hi),
                                    N.ptr(theta), b, int(classes or 1), n, int(mode), int(flags), 1 if targeted else 0, int(clip0), int(draw),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, _norm(norm), float(step_scale), int(max_halvings), lo, hi,
                                    N.ptr(x_cand), N.ptr(x_far), N.ptr(x_adv), N.ptr(x_best), N.ptr(fstate), N.ptr(istate), N.stream_ptr()))


def adversarial_device(logits, labels, targeted=False):
    """bool [B]: argmax != label (targeted: == label); a row with a NaN logit or a label outside [0, classes) is not adversarial --
    the decision of the kernels, for the clean rows and ``x_adv_init``."""
    c = logits.shape[1]
    lab = labels.long()
    pred = torch.nan_to_num(logits, nan=-math.inf).argmax(dim=1)
    ok = ~torch.isnan(logits).any(dim=1) & (lab >= 0) & (lab < c)
    return ((pred == lab) if targeted else (pred != lab)) & ok


class HopSkipJump:
    """ART HopSkipJump(classifier, batch_size=64, targeted=False, norm=2, max_iter=50, max_eval=10000, init_eval=100, init_size=100,
    verbose=True) over a TensorFlowV2Classifier (features) or a WaveformClassifier (samples, either domain; ``lengths=`` as
    SquareAttack takes them: the perturbation stays inside each clip and the rest of the row is returned bit for bit).

    ``norm``: 2 or np.inf -- the norm the distance is minimised in.  ``max_iter`` iterations, each with
    E = min(int(init_eval sqrt(t)), max_eval) perturbed copies; ``init_size``: the uniform draws tried for a start (untargeted).
    ``targeted``: y holds the class to reach and ``x_adv_init`` (every row already classified as its target) is required.
    ``verbose`` is accepted for ART's argument order and does nothing.
    Ours, after the ``*``.  ``seed``: the Philox key, offset by a constant of this class.  ``clip_values``: (lo, hi) clamps every
    point; default: the estimator's; None (a TensorFlowV2Classifier): no clamp, and the start draws and the first iteration's delta
    take each row's own [min, max].  ``gamma``: theta = gamma / sqrt(d) (L2) or gamma / d (L-inf), d the row's own elements.
    ``max_halvings``: the queries one step may spend halving its size.  ``check_every``: the queries between two looks at
    ``active.any()``, the only synchronisation inside a phase.

    Clips go through in chunks of min(batch_size, estimator.batch_limit), the draws of an iteration in sub-chunks so that clips x
    draws <= batch_limit.  A row misclassified when clean comes back bit for bit with distance 0 and 0 queries; a row for which no
    start is found comes back bit for bit with ``success_`` false.  The returned row is the closest adversarial point seen.
    After generate / generate_device, as device tensors: ``success_`` bool [B]; ``distance_`` float32 [B] in the attack's norm (+inf
    without a start); ``queries_`` int64 [B], the ALGORITHM's queries for that clip: every point whose label decided something for the
    row (a start draw, a perturbed copy, a halving, a bisection step), counted on the device, so the figure does not depend on the
    chunking.  It is not the number of rows forwarded: the clean prediction is not counted, and a row that has finished a phase
    (or has nothing to search for) still travels with its chunk through ``predict_device`` until the next look at ``active``, up
    to ``check_every`` - 1 calls per phase after the last row has finished; those forwards are counted nowhere.
    ``start_distance_`` float32 [B], the distance after the first bisection."""

    _UNSET = object()

    def __init__(self, classifier, batch_size=64, targeted=False, norm=2, max_iter=50, max_eval=10000, init_eval=100, init_size=100,
                 verbose=True, *, seed=0, clip_values=_UNSET, gamma=0.01, max_halvings=25, check_every=4):
        check_estimator(classifier, what="classifier")
        self.estimator = classifier
        self.norm = _norm(norm)
        self.batch_size, self.targeted, self.verbose = int(batch_size), bool(targeted), bool(verbose)
        self.max_iter, self.max_eval, self.init_eval, self.init_size = int(max_iter), int(max_eval), int(init_eval), int(init_size)
        self.gamma, self.max_halvings, self.check_every = float(gamma), int(max_halvings), int(check_every)
        if self.batch_size < 1 or self.check_every < 1 or self.max_halvings < 1:
            raise ValueError(f"batch_size = {batch_size}, check_every = {check_every}, max_halvings = {max_halvings}: at least 1")
        if not 0 <= self.max_iter < 1 << 24:
            raise ValueError(f"max_iter = {max_iter}: 0 to 2^24 - 1")
        if self.max_eval < 1 or self.init_eval < 1 or self.init_size < 1:
            raise ValueError(f"max_eval = {max_eval}, init_eval = {init_eval}, init_size = {init_size}: at least 1")
        if not 0.0 < self.gamma < math.inf:
            raise ValueError(f"gamma = {gamma}: a positive number is required")
        self.seed = (0x48534A0000000000 + int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.clip_values = resolve_clip_values(classifier, clip_values, HopSkipJump._UNSET)
        self.success_ = self.distance_ = self.queries_ = self.start_distance_ = None

    def evals(self, t):
        """E of iteration ``t``: min(int(init_eval sqrt(t)), max_eval)."""
        return min(int(self.init_eval * math.sqrt(t)), self.max_eval)

    def _phase(self, mode, limit, predict, kw, **first):
        """One phase of lipasr_hsj_search: FIRST, then one query per call until no row is active."""
        hsj_search(None, mode=mode, flags=FIRST, **kw, **first)
        active = kw["istate"][:, I["active"]]
        for i in range(limit):
            if i % self.check_every == 0 and not bool(active.any()):
                break
            hsj_search(predict(kw["x_cand"]), mode=mode, flags=0, **kw, **first)

    def generate_device(self, xt, yt=None, x_adv_init=None, lengths=None):
        """xt: float32 device tensor [B, features or samples]; yt: one-hot [B, classes] or class indices [B] or None (the model's
        own prediction); x_adv_init: [B, n] or None; returns a NEW device tensor."""
        est = self.estimator
        xt = est.rows_device(xt)
        b, n = xt.shape
        dev = xt.device
        lt = est.lengths_device(lengths, b)
        pos = None if lt is None else est.clip_mask(lt).sum(dim=1).to(torch.int32).contiguous()
        limit = int(est.batch_limit)
        cb = min(self.batch_size, limit)
        adv = xt.clone()
        self.success_ = torch.zeros(b, dtype=torch.bool, device=dev)
        self.queries_ = torch.zeros(b, dtype=torch.int64, device=dev)
        self.distance_ = torch.full((b,), math.inf, device=dev)
        self.start_distance_ = torch.full((b,), math.inf, device=dev)
        if self.targeted and (yt is None or x_adv_init is None):
            raise ValueError("a targeted attack needs the target labels `y` and `x_adv_init`, rows already classified as their target")
        if b == 0 or n == 0:
            return adv
        predict_all = lambda rows, ls: torch.cat([est.predict_device(rows[s:s + cb], logits=True, lengths=None if ls is None else ls[s:s + cb])
                                                  for s in range(0, b, cb)])
        clean = predict_all(xt, lt)
        labels = labels_device(xt, yt, self.targeted, lambda: clean.argmax(dim=1))
        already = adversarial_device(clean, labels, self.targeted)
        init = None
        if x_adv_init is not None:
            init = est.rows_device(x_adv_init)
            if tuple(init.shape) != (b, n):
                raise ValueError(f"x_adv_init must be [{b}, {n}], got {tuple(init.shape)}")
            if self.clip_values is not None:
                init = init.clamp(*self.clip_values)
            if pos is not None:
                init = torch.where(est.clip_mask(lt), init, xt)
            init_ok = adversarial_device(predict_all(init, lt), labels, self.targeted)
            if self.targeted and not bool((init_ok | already).all()):
                raise ValueError("x_adv_init: every row must already be classified as its target")
        # per row: d, theta, and the range of the start draws
        inside = None if pos is None else torch.arange(n, device=dev, dtype=torch.int32)[None, :] < pos[:, None]
        d = np.full(b, n, dtype=np.float64) if pos is None else pos.cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore"):
            theta = (self.gamma / np.sqrt(d) if self.norm == 2.0 else self.gamma / d).astype(np.float32)
        theta = torch.as_tensor(np.where(d > 0, theta, np.float32(0))).to(dev)
        if self.clip_values is not None:
            start_lo = torch.full((b,), self.clip_values[0], device=dev)
            start_hi = torch.full((b,), self.clip_values[1], device=dev)
        else:
            start_lo = (xt if inside is None else torch.where(inside, xt, torch.full_like(xt, math.inf))).amin(dim=1)
            start_hi = (xt if inside is None else torch.where(inside, xt, torch.full_like(xt, -math.inf))).amax(dim=1)
            empty = start_lo > start_hi
            start_lo, start_hi = start_lo.masked_fill(empty, 0.0).contiguous(), start_hi.masked_fill(empty, 0.0).contiguous()
        for s in range(0, b, cb):
            x0 = xt[s:s + cb]
            bb = x0.shape[0]
            lb = None if lt is None else lt[s:s + bb]
            dc = max(1, min(limit // bb, MAX_DRAWS))
            x_cand, x_far, x_adv, x_best, u = (torch.empty(bb, n, device=dev) for _ in range(5))
            fstate = torch.zeros(bb, 8, device=dev)
            istate = torch.zeros(bb, 8, dtype=torch.int32, device=dev)
            sums = torch.empty(bb, 2, n, dtype=torch.float64, device=dev)
            counts = torch.empty(bb, 2, dtype=torch.int32, device=dev)
            rows = torch.empty(bb * min(dc, max(self.max_eval, 1)), n, device=dev)
            nv = None if pos is None else pos[s:s + bb]
            lab = labels[s:s + bb]
            kw = dict(labels=lab, x0=x0, seed=self.seed, norm=self.norm, x_cand=x_cand, x_far=x_far, x_adv=x_adv, x_best=x_best,
                      fstate=fstate, istate=istate, start_lo=start_lo[s:s + bb], start_hi=start_hi[s:s + bb], theta=theta[s:s + bb], u=u,
                      n_valid=nv, targeted=self.targeted, clip0=s, max_halvings=self.max_halvings, clip_values=self.clip_values,
                      classes=est.nb_classes)
            predict = lambda r: est.predict_device(r, logits=True, lengths=lb)
            attack = ~already[s:s + bb]
            active, found = istate[:, I["active"]], istate[:, I["found"]]
            # ---- 1. the start
            if init is None:
                active.copy_(attack.to(torch.int32))
                hsj_search(None, mode=START, flags=FIRST, **kw)
                for k in range(self.init_size):
                    if k % self.check_every == 0 and not bool(active.any()):
                        break
                    hsj_search(predict(x_cand), mode=START, flags=LAST if k + 1 == self.init_size else 0, draw=k, **kw)
            else:
                hsj_search(None, mode=START, flags=FIRST, **kw)  # active is 0: every row is set up and none draws
                take = attack & init_ok[s:s + bb]
                x_far.copy_(torch.where(take[:, None], init[s:s + bb], x0))
                found.copy_(take.to(torch.int32))
                istate[:, I["ok"]].copy_(take.to(torch.int32))
            self._phase(BISECT, 256, predict, kw)
            self.start_distance_[s:s + bb] = fstate[:, F["dist"]]
            # ---- 2. the iterations
            span = (start_hi[s:s + bb] - start_lo[s:s + bb]) * 0.1
            for t in range(1, self.max_iter + 1):
                if t == 1 and not bool(found.any()):
                    break
                delta = (span if t == 1 else fstate[:, F["dist"]] * self.gamma).contiguous()
                evals = self.evals(t)
                sums.zero_()
                counts.zero_()
                for j0 in range(0, evals, dc):
                    dn = min(dc, evals - j0)
                    p = hsj_expand(x_adv, delta, dn, t, self.seed, self.norm, out=rows[:bb * dn], n_valid=nv, clip0=s, draw0=j0,
                                   clip_values=self.clip_values)
                    z = est.predict_device(p, logits=True, lengths=None if lb is None else lb.repeat_interleave(dn))
                    hsj_accumulate(z, lab, p, x_adv, sums=sums, counts=counts, n_valid=nv, targeted=self.targeted)
                hsj_direction(sums, counts, self.norm, u=u, n_valid=nv)
                istate[:, I["queries"]] += found * evals
                self._phase(HALVE, self.max_halvings, predict, kw, step_scale=1.0 / math.sqrt(t))
                self._phase(BISECT, 256, predict, kw)
            got = found != 0
            adv[s:s + bb] = torch.where(got[:, None], x_best, x0)
            self.distance_[s:s + bb] = torch.where(attack, fstate[:, F["dist_best"]], torch.zeros(bb, device=dev))
            self.queries_[s:s + bb] = istate[:, I["queries"]].long()
            self.success_[s:s + bb] = got | ~attack
        return adv

    def generate(self, x, y=None, x_adv_init=None, lengths=None):
        return generate_host(self, x, y, x_adv_init, lengths)
