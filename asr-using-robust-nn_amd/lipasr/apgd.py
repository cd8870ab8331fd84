"""Auto-PGD (Croce & Hein 2020, "Reliable evaluation of adversarial robustness with an ensemble of diverse parameter-free attacks"):
the two native calls of one iteration and the checkpoint schedule.  ``lipasr.attacks.AutoProjectedGradientDescent`` is the attack.

One iteration is the estimator's forward pass, ``apgd_loss`` (lipasr_apgd_loss: the objective to maximise -- cross-entropy or the
Difference-of-Logits-Ratio -- its gradient at the logits and whether the row is misclassified), the estimator's backward pass, and
``apgd_step`` (lipasr_apgd_step: per row the step size, the best point, the counters, the checkpoint decision and the momentum
step with its two projections).  Every row carries its own state, so nothing returns to the host inside a run.
include/lipasr.h fixes the conventions.
"""
from __future__ import annotations

import math

import torch

from . import _native as N
from ._rows import _dev_tensor, clip_pair, rows2d

LOSS_TYPES = {"cross_entropy": 0, "difference_logits_ratio": 1}
FIRST, LAST = 1, 2
STATE = (("eta", torch.float32), ("f_best", torch.float32), ("f_prev", torch.float32), ("f_best_ckpt", torch.float32),
         ("improved", torch.int32), ("reduced_last", torch.int32), ("fooled", torch.int32), ("halvings", torch.int32))


def apgd_checkpoints(max_iter):
    """The iterations at which Auto-PGD looks at its step size, in integer hundredths (0.22 * 100 is not 22 in binary):
    p_0 = 0, p_1 = 22, p_{j+1} = p_j + max(p_j - p_{j-1} - 3, 6) while <= 100; w_j = ceil(p_j max_iter / 100) -> the sorted unique
    w_j in 1 .. max_iter - 1."""
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError(f"max_iter = {max_iter}: at least 1")
    p = [0, 22]
    while True:
        nxt = p[-1] + max(p[-1] - p[-2] - 3, 6)
        if nxt > 100:
            break
        p.append(nxt)
    return sorted({-((-q * max_iter) // 100) for q in p} & set(range(1, max_iter)))


def _loss_code(loss_type):
    if loss_type in (0, 1):
        return int(loss_type)
    try:
        return LOSS_TYPES[loss_type]
    except (KeyError, TypeError):
        raise ValueError(f"loss_type = {loss_type!r}: 'cross_entropy' or 'difference_logits_ratio'") from None


def apgd_state(rows, device):
    """The per-row state of lipasr_apgd_step as a dict of device tensors [rows] (a FIRST step initialises it)."""
    return {k: torch.zeros(rows, dtype=dt, device=device) for k, dt in STATE}


def apgd_loss(logits, labels, loss_type="cross_entropy", targeted=False, *, f=None, dz=None, hit=None):
    """lipasr_apgd_loss on device tensors: logits float32 [B, C], labels int32 [B] -> (f float32 [B], dz float32 [B, C], hit int32
    [B]); ``f``, ``dz``, ``hit``: tensors to write into."""
    b, c = rows2d(logits, "logits", "[B, classes]")
    code = _loss_code(loss_type)
    _dev_tensor(labels, torch.int32, (b,), "labels")
    f = torch.empty(b, device=logits.device) if f is None else _dev_tensor(f, torch.float32, (b,), "f")
    dz = torch.empty(b, c, device=logits.device) if dz is None else _dev_tensor(dz, torch.float32, (b, c), "dz")
    hit = torch.empty(b, dtype=torch.int32, device=logits.device) if hit is None else _dev_tensor(hit, torch.int32, (b,), "hit")
    h = N.get_handle(logits.device.index)
    N.check(N.lib.lipasr_apgd_loss(h.h, N.ptr(logits), N.ptr(labels), b, c, code, 1 if targeted else 0, N.ptr(f), N.ptr(dz), N.ptr(hit),
                                   N.stream_ptr()))
    return f, dz, hit


def apgd_step(x, x_prev, x0, g, x_best, g_best, x_adv, f, hit, state, *, norm, eps, eta0, clip_values=None, momentum=0.75, rho=0.75,
              first=False, last=False, ckpt_len=0, n_valid=None):
    """lipasr_apgd_step on device tensors, in place: the seven row arrays float32 [rows, n], f float32 [rows] and hit int32 [rows]
    at x, ``state`` the dict of ``apgd_state``, n_valid int32 [rows] or None.  Returns x."""
    rows, n = rows2d(x, "x", "[rows, n]")
    for t, what in ((x_prev, "x_prev"), (x0, "x0"), (g, "g"), (x_best, "x_best"), (g_best, "g_best"), (x_adv, "x_adv")):
        _dev_tensor(t, torch.float32, (rows, n), what)
    _dev_tensor(f, torch.float32, (rows,), "f")
    _dev_tensor(hit, torch.int32, (rows,), "hit")
    if n_valid is not None:
        _dev_tensor(n_valid, torch.int32, (rows,), "n_valid")
    if set(state) != {k for k, _ in STATE}:
        raise ValueError(f"state must hold {[k for k, _ in STATE]}")
    for k, dt in STATE:
        _dev_tensor(state[k], dt, (rows,), k)
    nrm = float(norm)
    if not (nrm == 2.0 or nrm == math.inf):
        raise ValueError(f"norm = {norm!r}: 2 and inf are supported")
    lo, hi = clip_pair(clip_values)
    flags = (FIRST if first else 0) | (LAST if last else 0)
    h = N.get_handle(x.device.index)
    N.check(N.lib.lipasr_apgd_step(h.h, N.ptr(x), N.ptr(x_prev), N.ptr(x0), N.ptr(g), N.ptr(x_best), N.ptr(g_best), N.ptr(x_adv), N.ptr(f),
                                   N.ptr(hit), N.ptr(n_valid), *(N.ptr(state[k]) for k, _ in STATE), rows, n, nrm, float(eps), float(eta0),
                                   lo, hi, float(momentum), float(rho), flags, int(ckpt_len), N.stream_ptr()))
    return x


def apgd_path(n, aligned=True):
    """lipasr_debug_apgd_path: (instance 0 .. 7, float4 loads) for rows of n floats."""
    code = int(N.lib.lipasr_debug_apgd_path(int(n), 1 if aligned else 0))
    if code < 0:
        raise ValueError(f"n = {n}")
    return code & 7, bool(code & 8)
