"""Float64 NumPy restatement of ART's FastGradientMethod / ProjectedGradientDescent in norm 1, 2 and inf, targeted and with
random restarts (adversarial-robustness-toolbox 1.9-1.10, fast_gradient.py / projected_gradient_descent_numpy.py /
utils.projection / utils.random_sphere / utils.compute_success(_array), restated from the published code: parity unpinned,
as for oracle.attacks_ref).  TEST INFRASTRUCTURE for tests/test_lp_*: built on oracle.mlp_ref.input_gradient_infer and
oracle.attacks_ref._own_labels.

Random starts are not drawn here: the caller passes the deltas of every restart (``deltas[r]``: [N, n]), which is what the
product's ``_random_init`` is replaced by in the restart tests.
"""
from __future__ import annotations

import numpy as np

from oracle import attacks_ref as AR, mlp_ref as P

TOL = 1e-7  # ART's tol = 10e-8


def _is_inf(norm):
    return norm in (np.inf, "inf")


def direction(g, norm):
    """ART's _compute_perturbation without the targeted factor: NaN -> 0, then sign(g) | g / (|g|_1 + tol) | g / (|g|_2 + tol);
    a row whose norm is not finite takes no step (norm 1, 2)."""
    g = np.where(np.isnan(g), 0.0, np.asarray(g, dtype=np.float64))
    if _is_inf(norm):
        return np.sign(g)
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.abs(g).sum(axis=1, keepdims=True) if norm == 1 else np.sqrt((g * g).sum(axis=1, keepdims=True))
        d = g / (nrm + TOL)
    return np.where(np.isfinite(nrm), d, 0.0)


def project(dl, eps, norm):
    """ART's projection(values, eps, norm_p) on rows; eps = inf: none."""
    if np.isinf(eps):
        return dl
    if _is_inf(norm):
        return np.clip(dl, -eps, eps)
    nrm = np.abs(dl).sum(axis=1, keepdims=True) if norm == 1 else np.sqrt((dl * dl).sum(axis=1, keepdims=True))
    return dl * np.minimum(1.0, eps / (nrm + TOL))


def lp_step(x_adv, x0, g, alpha, eps, norm):
    """What lipasr_lp_step computes: x0 + P_eps(x_adv + alpha d(g) - x0)."""
    xp = np.asarray(x_adv, np.float64) + alpha * direction(g, norm)
    return np.asarray(x0, np.float64) + project(xp - np.asarray(x0, np.float64), eps, norm)


def _grad(spec, p, xa, yb):
    return P.input_gradient_infer(spec, p, xa, yb)


def labels(spec, p, x, y=None, targeted=False, batch_size=32):
    if y is None:
        if targeted:
            raise ValueError("targeted needs y")
        return AR._own_labels(spec, p, x, batch_size)
    return np.asarray(y, np.float64)


def success(spec, p, x0, y, xa, targeted):
    """ART compute_success_array."""
    pa = P.forward_infer(spec, p, xa).argmax(axis=1)
    if targeted:
        return pa == np.asarray(y).argmax(axis=1)
    return pa != P.forward_infer(spec, p, x0).argmax(axis=1)


def fgm(spec, p, x, eps, norm=np.inf, y=None, targeted=False, batch_size=32, deltas=None):
    """FastGradientMethod.generate: one step of eps from x (+ delta), projected on the eps ball (ART's project=True);
    with len(deltas) > 1 the restart with the highest success rate (first on ties)."""
    x = np.asarray(x, np.float64)
    y = labels(spec, p, x, y, targeted, batch_size)
    sgn = -1.0 if targeted else 1.0
    best, best_rate = None, None
    runs = deltas if deltas is not None else [None]
    for dlt in runs:
        start = x if dlt is None else x + dlt
        adv = np.empty_like(x)
        for i in range(0, len(x), batch_size):
            sl = slice(i, i + batch_size)
            adv[sl] = lp_step(start[sl], x[sl], _grad(spec, p, start[sl], y[sl]), sgn * eps, eps, norm)
        if len(runs) > 1:
            rate = success(spec, p, x, y, adv, targeted).mean()
            if best_rate is None or rate > best_rate:
                best, best_rate = adv, rate
        else:
            best = adv
    return best


def pgd(spec, p, x, eps, eps_step=0.1, max_iter=100, norm=np.inf, y=None, targeted=False, batch_size=32, deltas=None):
    """ProjectedGradientDescent.generate: per batch and restart, max_iter steps from x (+ delta); restart 0 is kept, later
    restarts overwrite the rows where they succeed."""
    x = np.asarray(x, np.float64)
    y = labels(spec, p, x, y, targeted, batch_size)
    sgn = -1.0 if targeted else 1.0
    adv = x.copy()
    runs = deltas if deltas is not None else [None]
    for i in range(0, len(x), batch_size):
        sl = slice(i, i + batch_size)
        x0, yb = x[sl], y[sl]
        for r, dlt in enumerate(runs):
            xa = x0.copy() if dlt is None else x0 + dlt[sl]
            for _ in range(max_iter):
                xa = lp_step(xa, x0, _grad(spec, p, xa, yb), sgn * eps_step, eps, norm)
            if r == 0:
                adv[sl] = xa
            else:
                ok = success(spec, p, x0, yb, xa, targeted)
                adv[sl][ok] = xa[ok]
    return adv
