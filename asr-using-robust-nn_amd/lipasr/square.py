"""Square Attack (Andriushchenko, Croce, Flammarion and Hein 2020, "Square Attack: a query-efficient black-box adversarial attack via
random search"), the L-inf form, over the estimators of lipasr.estimators: it queries scores only, never a gradient, and spends ONE
query per iteration where GeneticAttack spends ``pop_size``.

Why it is here: it is the fourth member of the AutoAttack ensemble (lipasr.attacks.AutoAttack) and the stronger query-only check
for masked gradients -- a constrained network (NonNeg kernels, a small Lipschitz constant, a saturating softmax) is where those
can happen.

Every point of the search is x0 + s eps element by element, s = +-1, clamped to the clip range.  A row is a height x width
picture (an MFCC row: 20 x frames; a clip: a 1 x n strip in which a "square" is a segment of samples).  The start gives every
column one random sign; a proposal overwrites one window with one random sign and is kept where the margin loss goes down.  Per
query, per chunk: the estimator's ``predict_device(x_cand, logits=True)`` and ONE lipasr_square_step, which moves only the window's
bytes; the only synchronisation is ``done.all()`` every ``check_every`` iterations.  Philox counters are keyed by seed, row index,
restart and iteration, so a row's run depends on neither its neighbours nor the chunking.  include/lipasr.h fixes the conventions.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from ._rows import _dev_tensor, check_estimator, clip_pair, generate_host, labels_device, resolve_clip_values, rows2d

LAST = N.SQUARE_LAST
SCHEDULE = (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)  # of a run rescaled to 10 000 iterations


def square_p(it, max_iter, p_init):
    """The paper's piecewise-constant schedule AS REMEMBERED: the share of the row a window covers at iteration ``it`` of
    ``max_iter`` -- ``p_init`` halved after each of the rescaled iterations 10, 50, 200, 500, 1000, 2000, 4000, 6000 and 8000, the run
    rescaled to 10 000 (integers: it * 10000 // max_iter)."""
    scaled = int(it) * 10000 // max(int(max_iter), 1)
    return float(p_init) / (1 << sum(scaled > t for t in SCHEDULE))


def square_window(p, height, width):
    """(win_h, win_w) of a window that covers the share ``p`` of a height x width row: a square of side round(sqrt(p height width))
    clamped to [1, height] and [1, width]; for a strip (height 1) the segment (1, clamp(round(p width), 1, width))."""
    p, height, width = float(p), int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"a row of {height} x {width}")
    if height == 1:
        return 1, min(max(int(round(p * width)), 1), width)
    side = int(round(math.sqrt(max(p, 0.0) * height * width)))
    return min(max(side, 1), height), min(max(side, 1), width)


def square_p_q(p):
    """round(p * 2^24) with p clamped to [0, 1]: the integer lipasr_square_step sizes a ragged clip's segment with."""
    return int(round(min(max(float(p), 0.0), 1.0) * 16777216.0))


def _rows(x0, height, width):
    b, n = rows2d(x0, "x0")
    height, width = int(height), int(width)
    if height < 0 or width < 0 or height * width != n:
        raise ValueError(f"shape = ({height}, {width}) does not multiply to the row length {n}")
    return b, n, height, width


def square_init(x0, height, width, restart, seed, eps, *, x_best, x_cand, win, n_valid=None, clip0=0, clip_values=None):
    """lipasr_square_init on device tensors: x0 float32 [B, height * width], n_valid int32 [B] or None (height 1 only); writes the
    stripe start of rows ``clip0 + b`` into x_best and x_cand float32 [B, n] and zeroes win int32 [B, 4]."""
    b, n, height, width = _rows(x0, height, width)
    _dev_tensor(x_best, torch.float32, (b, n), "x_best")
    _dev_tensor(x_cand, torch.float32, (b, n), "x_cand")
    _dev_tensor(win, torch.int32, (b, 4), "win")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    if not 0 <= int(restart) < 256:
        raise ValueError(f"restart = {restart}: 0 to 255")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x0.device.index)
    N.check(N.lib.lipasr_square_init(h.h, N.ptr(x0), N.ptr(n_valid), b, height, width, int(clip0), int(restart),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, float(eps), lo, hi, N.ptr(x_best), N.ptr(x_cand), N.ptr(win),
                                     N.stream_ptr()))


def square_step(logits, labels, x0, height, width, win_h, win_w, p_q, restart, it, seed, eps, *, x_best, x_cand, loss_best, done, win,
                n_valid=None, targeted=False, last=False, clip0=0, clip_values=None):
    """lipasr_square_step on device tensors, in place: logits float32 [B, classes] at x_cand, labels int32 [B], x0, x_best, x_cand
    float32 [B, height * width], loss_best float32 [B], done int32 [B] (sticky; it + 1 where the row succeeds), win int32 [B, 4],
    n_valid int32 [B] or None (height 1 only)."""
    b, n, height, width = _rows(x0, height, width)
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
            and logits.shape[0] == b):
        raise ValueError(f"logits must be a contiguous float32 device tensor [{b}, classes]")
    _dev_tensor(labels, torch.int32, (b,), "labels")
    _dev_tensor(x_best, torch.float32, (b, n), "x_best")
    _dev_tensor(x_cand, torch.float32, (b, n), "x_cand")
    _dev_tensor(loss_best, torch.float32, (b,), "loss_best")
    _dev_tensor(done, torch.int32, (b,), "done")
    _dev_tensor(win, torch.int32, (b, 4), "win")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (b,), "n_valid")
    if not 0 <= int(it) < 1 << 24:
        raise ValueError(f"it = {it}: 0 to 2^24 - 1")
    if not 0 <= int(restart) < 256:
        raise ValueError(f"restart = {restart}: 0 to 255")
    if not 0 <= int(p_q) <= 1 << 24:
        raise ValueError(f"p_q = {p_q}: 0 to 2^24")
    lo, hi = clip_pair(clip_values)
    h = N.get_handle(x0.device.index)
    N.check(N.lib.lipasr_square_step(h.h, N.ptr(logits), N.ptr(labels), N.ptr(x0), N.ptr(n_valid), b, logits.shape[1], height, width,
                                     int(win_h), int(win_w), int(p_q), 1 if targeted else 0, int(clip0), int(restart), int(it),
                                     LAST if last else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, float(eps), lo, hi, N.ptr(x_best),
                                     N.ptr(x_cand), N.ptr(loss_best), N.ptr(done), N.ptr(win), N.stream_ptr()))


def margin_device(logits, labels, targeted=False):
    """float32 [B]: z_y - max_{c != y} z_c (targeted: its negative), the loss of lipasr_square_step, on finite logits with labels
    inside [0, classes) the same bits; +inf with one class."""
    b, c = logits.shape
    if c == 1:
        return torch.full((b,), math.inf, device=logits.device)
    own = torch.arange(c, device=logits.device)[None, :] == labels.long()[:, None]
    m = logits.gather(1, labels.long()[:, None])[:, 0] - logits.masked_fill(own, -math.inf).max(dim=1).values
    return -m if targeted else m


class SquareAttack:
    """ART SquareAttack(estimator=, norm=, max_iter=, eps=, p_init=, nb_restarts=, batch_size=) (Andriushchenko et al. 2020) in the
    L-inf ball of radius ``eps`` around every row: over the features of a TensorFlowV2Classifier, or over the samples of a
    WaveformClassifier (either domain; ``lengths=`` as GeneticAttack takes them: the perturbation stays inside each clip and the rest
    of the row is returned bit for bit; a short-window extractor takes no lengths).

    ``norm``: np.inf only -- the paper's L2 variant redistributes mass between windows and is not built.  ``max_iter``: the queries
    per row and restart, the stripe start counted as the first.  ``p_init`` and the schedule ``p_schedule(it, max_iter, p_init)``
    (default ``square_p``: p_init halved after rescaled iterations 10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000 of 10 000) are the
    paper's settings AS REMEMBERED, and the defaults are ART's as remembered; nothing in this repository can check them against
    either, so they are keywords (ART is absent: parity unpinned).  ``nb_restarts`` (1 .. 256): a fooled row keeps the first restart
    that fooled it, any other row the restart with the lowest loss.
    Ours, after the ``*``.  ``shape``: (height, width) of a row as a picture, must multiply to the row length; None: (1, n), a strip,
    which is also what every call with ``lengths`` needs.  ``targeted``: y holds the class to reach (required then); otherwise the
    class to leave, y=None: the model's own prediction.  The loss is the logit margin z_y - max_{c != y} z_c (targeted: its
    negative); a row is done when it is negative and is left alone from then on.  ``seed``: the Philox key, offset by a constant of
    this class so that no counter is shared with the other attacks; a row's draws are a function of (seed, its row index in x,
    restart, iteration).  ``clip_values``: (lo, hi) clamps every point; default: the estimator's (a TensorFlowV2Classifier has
    none).  ``check_every``: the iterations between two looks at ``done`` -- the only synchronisation inside a restart.

    Rows go through in chunks of min(batch_size, estimator.batch_limit).  A row whose clean margin is already negative comes back
    bit for bit with ``success_`` true and ``queries_`` 0.  After generate / generate_device: ``success_`` bool [B], ``queries_`` int64
    [B] (the queries spent on the row over its restarts, up to and including the one that fooled it) and ``loss_`` float32 [B] (the
    margin of the returned row), as device tensors."""

    _UNSET = object()

    def __init__(self, estimator, norm=np.inf, max_iter=100, eps=0.3, p_init=0.8, nb_restarts=1, batch_size=128, *, shape=None,
                 targeted=False, seed=0, clip_values=_UNSET, p_schedule=square_p, check_every=10):
        check_estimator(estimator)
        if norm not in (np.inf, "inf", math.inf):
            raise ValueError(f"norm = {norm!r}: only np.inf is built -- the L2 Square Attack redistributes mass between windows and is "
                             "out of scope")
        self.estimator, self.norm = estimator, np.inf
        self.eps, self.p_init = float(eps), float(p_init)
        if not 0.0 <= self.eps < math.inf:
            raise ValueError(f"eps = {eps}: a finite, non-negative number is required")
        if not 0.0 < self.p_init <= 1.0:
            raise ValueError(f"p_init = {p_init}: a share in (0, 1] is required")
        self.max_iter, self.nb_restarts = int(max_iter), int(nb_restarts)
        self.batch_size, self.check_every = int(batch_size), int(check_every)
        if not 1 <= self.max_iter <= 1 << 24:
            raise ValueError(f"max_iter = {max_iter}: 1 to 2^24")
        if not 1 <= self.nb_restarts <= 256:
            raise ValueError(f"nb_restarts = {nb_restarts}: 1 to 256")
        if self.batch_size < 1 or self.check_every < 1:
            raise ValueError(f"batch_size = {batch_size}, check_every = {check_every}: at least 1")
        if shape is not None:
            if len(tuple(shape)) != 2:
                raise ValueError(f"shape = {shape!r}: (height, width) is required")
            shape = (int(shape[0]), int(shape[1]))
            if shape[0] < 1 or shape[1] < 1 or shape[0] * shape[1] != estimator.input_shape[0]:
                raise ValueError(f"shape = {shape} does not multiply to the row length {estimator.input_shape[0]}")
        self.shape = shape
        if not callable(p_schedule):
            raise TypeError("p_schedule must be callable: p_schedule(it, max_iter, p_init) -> share of the row")
        self.p_schedule = p_schedule
        self.targeted = bool(targeted)
        self.seed = (0x5CA2E00000000000 + int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.clip_values = resolve_clip_values(estimator, clip_values, SquareAttack._UNSET)
        self.success_ = self.queries_ = self.loss_ = None

    def window(self, it, height, width):
        """(win_h, win_w, p_q) of proposal ``it``."""
        p = self.p_schedule(it, self.max_iter, self.p_init)
        return (*square_window(p, height, width), square_p_q(p))

    def generate_device(self, xt, yt=None, lengths=None):
        """xt: float32 device tensor [B, features or samples]; yt: one-hot [B, classes] or class indices [B] or None; returns a NEW
        device tensor: per row the best point found -- the adversarial one where the row is done, the lowest margin otherwise."""
        est = self.estimator
        xt = est.rows_device(xt)
        b, n = xt.shape
        dev = xt.device
        lt = est.lengths_device(lengths, b)
        height, width = (1, n) if self.shape is None else self.shape
        if lt is not None and height != 1:
            raise ValueError(f"lengths= goes with a 1 x n strip, shape = {self.shape}")
        pos = None if lt is None else est.clip_mask(lt).sum(dim=1).to(torch.int32).contiguous()
        bs = min(self.batch_size, int(est.batch_limit))
        adv = xt.clone()
        self.success_ = torch.zeros(b, dtype=torch.bool, device=dev)
        self.queries_ = torch.zeros(b, dtype=torch.int64, device=dev)
        self.loss_ = torch.full((b,), math.inf, device=dev)
        if b == 0 or n == 0:
            return adv
        clean = torch.cat([est.predict_device(xt[s:s + bs], logits=True, lengths=None if lt is None else lt[s:s + bs])
                           for s in range(0, b, bs)])
        labels = labels_device(xt, yt, self.targeted, lambda: clean.argmax(dim=1))
        margin = margin_device(clean, labels, self.targeted)
        already = margin < 0
        self.loss_ = torch.where(already, margin, self.loss_)
        windows = [self.window(it + 1, height, width) for it in range(self.max_iter)]
        bufs = [torch.empty(min(b, bs), n, device=dev) for _ in range(2)]
        for s in range(0, b, bs):
            x0 = xt[s:s + bs]
            bb = x0.shape[0]
            lb = None if lt is None else lt[s:s + bb]
            lab = labels[s:s + bb]
            x_best, x_cand = bufs[0][:bb], bufs[1][:bb]
            win = torch.empty(bb, 4, dtype=torch.int32, device=dev)
            loss_best = torch.empty(bb, device=dev)
            kw = dict(x_best=x_best, x_cand=x_cand, win=win, n_valid=None if pos is None else pos[s:s + bb], clip0=s,
                      clip_values=self.clip_values)
            fooled = already[s:s + bb].clone()  # rows that take no further part: misclassified when clean, or fooled by a restart
            for r in range(self.nb_restarts):
                if bool(fooled.all()):
                    break
                done = fooled.to(torch.int32)
                square_init(x0, height, width, r, self.seed, self.eps, **kw)
                evaluated = 0
                for it in range(self.max_iter):
                    last = it + 1 == self.max_iter
                    wh, ww, pq = windows[it]
                    square_step(est.predict_device(x_cand, logits=True, lengths=lb), lab, x0, height, width, wh, ww, pq, r, it, self.seed,
                                self.eps, loss_best=loss_best, done=done, targeted=self.targeted, last=last, **kw)
                    evaluated = it + 1
                    if not last and evaluated % self.check_every == 0 and bool((done != 0).all()):
                        break
                now = (done != 0) & ~fooled
                take = (now | (loss_best < self.loss_[s:s + bb])) & ~fooled
                adv[s:s + bb] = torch.where(take[:, None], x_best, adv[s:s + bb])
                self.loss_[s:s + bb] = torch.where(take, loss_best, self.loss_[s:s + bb])
                spent = torch.where(now, done, torch.full_like(done, evaluated)).long()
                self.queries_[s:s + bb] += torch.where(fooled, torch.zeros_like(spent), spent)
                fooled = fooled | now
            self.success_[s:s + bb] = fooled
        return adv

    def generate(self, x, y=None, lengths=None):
        return generate_host(self, x, y, lengths)
