"""Oracle of Square Attack (lipasr_square_init, lipasr_square_step, their host twins, lipasr.square.SquareAttack): a NumPy
restatement.  TEST INFRASTRUCTURE for tests/test_square_* and tests/test_autoattack_gpu.py: nothing here is used by the library.

    philox        philox_ref's, re-exported
    init          the vertical-stripe start (include/lipasr.h, lipasr_square_init)
    margin        the loss of one row of logits, in float32
    draw          proposal it + 1 of a row: window and sign
    step          one lipasr_square_step, in place on a state dict
    square_p, square_window, p_q    the schedule and the window of lipasr.square, restated
    run           a whole restart over any ``predict`` (float32 rows -> float32 logits)

Everything the kernels do is integer arithmetic, one fp32 add, two clamps and one fp32 subtract, so the restatement is exact: the
tests compare bits.
"""
from __future__ import annotations

import math

import numpy as np

from philox_ref import MASK, nv as _row_nv, philox  # noqa: F401  (philox: re-exported under the name the tests import)

STRIPE_TAG = 1 << 62
SCHEDULE = (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)


def value(x, minus, eps, lo=-np.inf, hi=np.inf):
    """min(max(fl(x + s eps), lo), hi) in float32, element by element; a NaN stays."""
    x = np.asarray(x, dtype=np.float32)
    t = (x + (-np.float32(eps) if minus else np.float32(eps))).astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        return np.where(t < lo, lo, np.where(t > hi, hi, t)).astype(np.float32)


def _nv(n_valid, b, n):
    return None if n_valid is None else _row_nv(n_valid, b, n)  # None: no lengths, as the kernel's -1


def stripe_signs(seed, clip, restart, width):
    """bool [width]: column c takes s = -1."""
    blocks = [philox(seed, (q | STRIPE_TAG), clip, (restart << 24) & MASK) for q in range((width + 127) // 128)]
    return np.array([(blocks[c >> 7][(c >> 5) & 3] >> (c & 31)) & 1 for c in range(width)], dtype=bool)


def init(x0, height, width, restart, seed, eps, n_valid=None, clip0=0, lo=-np.inf, hi=np.inf):
    """-> state dict: x_best, x_cand float32 [B, n], win int32 [B, 4] (loss_best and done are the caller's)."""
    x0 = np.asarray(x0, dtype=np.float32)
    B, n = x0.shape
    assert height * width == n
    best = x0.copy()
    for b in range(B):
        nv = _nv(n_valid, b, n)
        minus = stripe_signs(seed, clip0 + b, restart, width)
        pic = x0[b].reshape(height, width)
        v = np.where(minus[None, :], value(pic, True, eps, lo, hi), value(pic, False, eps, lo, hi)).reshape(n)
        inside = np.arange(n) < (n if nv is None else nv)
        best[b] = np.where(inside, v, x0[b])
    return dict(x_best=best, x_cand=best.copy(), win=np.zeros((B, 4), dtype=np.int32))


def margin(z, y, targeted=False):
    """float32: z_y - max_{c != y} z_c (targeted: its negative); one class or a label outside [0, classes): +inf; any NaN: NaN."""
    z = np.asarray(z, dtype=np.float32)
    C = z.shape[0]
    if C == 1 or not 0 <= y < C:
        return np.float32(np.inf)
    if np.isnan(z).any():
        return np.float32(np.nan)
    other = np.max(np.delete(z, y))
    with np.errstate(invalid="ignore"):
        m = np.float32(z[y] - other)
    return np.float32(-m) if targeted else m


def draw(seed, clip, restart, it1, height, width, nv, win_h, win_w, p_q):
    """-> ((r, c, h, w), minus) of proposal ``it1``; nv None: no n_valid."""
    o = philox(seed, 0, clip, ((restart << 24) | it1) & MASK)
    h, w, rows, cols = win_h, win_w, height, width
    if nv is not None:
        h, rows, cols = 1, 1, nv
        w = min(max((nv * p_q + (1 << 23)) >> 24, 1), nv)
    return ((o[0] * (rows - h + 1)) >> 32, (o[1] * (cols - w + 1)) >> 32, h, w), bool(o[2] & 1)


def step(st, logits, labels, x0, height, width, win_h, win_w, p_q, restart, it, seed, eps, n_valid=None, targeted=False, last=False,
         clip0=0, lo=-np.inf, hi=np.inf):
    """One lipasr_square_step in place on st = dict(x_best, x_cand, loss_best float32 [B], done int32 [B], win int32 [B, 4]);
    returns the float32 losses [B]."""
    x0 = np.asarray(x0, dtype=np.float32)
    B, n = x0.shape
    losses = np.zeros(B, dtype=np.float32)
    for b in range(B):
        nv = _nv(n_valid, b, n)
        loss = losses[b] = margin(logits[b], int(labels[b]), targeted)
        best, cand = st["x_best"][b].reshape(height, width), st["x_cand"][b].reshape(height, width)
        r, c, h, w = (int(v) for v in st["win"][b])
        arrived_done = st["done"][b] != 0
        if it == 0:
            st["loss_best"][b] = np.float32(np.inf) if np.isnan(loss) else loss
        elif not arrived_done and loss < st["loss_best"][b]:
            best[r:r + h, c:c + w] = cand[r:r + h, c:c + w]
            st["loss_best"][b] = loss
        else:
            cand[r:r + h, c:c + w] = best[r:r + h, c:c + w]
        if not arrived_done and st["loss_best"][b] < 0:
            st["done"][b] = it + 1
        st["win"][b] = 0
        if st["done"][b] != 0 or nv == 0 or last:
            continue
        (r, c, h, w), minus = draw(seed, clip0 + b, restart, it + 1, height, width, nv, win_h, win_w, p_q)
        pic = x0[b].reshape(height, width)
        cand[r:r + h, c:c + w] = value(pic[r:r + h, c:c + w], minus, eps, lo, hi)
        st["win"][b] = (r, c, h, w)
    return losses


def square_p(it, max_iter, p_init):
    scaled = int(it) * 10000 // max(int(max_iter), 1)
    return float(p_init) / (1 << sum(scaled > t for t in SCHEDULE))


def square_window(p, height, width):
    if height == 1:
        return 1, min(max(int(round(p * width)), 1), width)
    side = int(round(math.sqrt(max(p, 0.0) * height * width)))
    return min(max(side, 1), height), min(max(side, 1), width)


def p_q(p):
    return int(round(min(max(float(p), 0.0), 1.0) * 16777216.0))


def run(predict, x0, labels, eps, max_iter, p_init=0.8, shape=None, restart=0, seed=0, n_valid=None, targeted=False, clip0=0,
        lo=-np.inf, hi=np.inf, schedule=square_p):
    """One restart of SquareAttack over all rows at once -> dict: x_best float32 [B, n], loss_best float32 [B], done int32 [B],
    trace float32 [queries, B] (loss_best after every query), losses float32 [queries, B] (what every query returned)."""
    x0 = np.asarray(x0, dtype=np.float32)
    B, n = x0.shape
    height, width = (1, n) if shape is None else shape
    st = init(x0, height, width, restart, seed, eps, n_valid, clip0, lo, hi)
    st["loss_best"], st["done"] = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int32)
    trace, losses = [], []
    for it in range(max_iter):
        p = schedule(it + 1, max_iter, p_init)
        wh, ww = square_window(p, height, width)
        z = np.asarray(predict(st["x_cand"]), dtype=np.float32)
        losses.append(step(st, z, labels, x0, height, width, wh, ww, p_q(p), restart, it, seed, eps, n_valid, targeted,
                           it + 1 == max_iter, clip0, lo, hi))
        trace.append(st["loss_best"].copy())
    return dict(x_best=st["x_best"], x_cand=st["x_cand"], loss_best=st["loss_best"], done=st["done"], trace=np.array(trace),
                losses=np.array(losses))
