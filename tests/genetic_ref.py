"""Oracle of the genetic black-box attack (lipasr_genetic_breed, lipasr_genetic_breed_host, lipasr_genetic_select,
lipasr.genetic.GeneticAttack): a NumPy restatement in float64.  TEST INFRASTRUCTURE for tests/test_genetic_*: nothing here is used
by the library.

    breed       one generation's children (include/lipasr.h, lipasr_genetic_breed): which parent every element takes, which
                elements mutate, picked + step v in float64, the two clamps (the ball's bounds are the fp32 numbers x0 -+ eps, as the
                kernel forms them), the padding
    select      fitness, best, done, parents (lipasr_genetic_select) with, per parent draw, the two indices a draw within
                1e-5 * total of a cumulative weight may come out as
    attack      the whole algorithm over any ``classify`` (float64 rows -> logits), members stored as float32 between generations
"""
from __future__ import annotations

import numpy as np

from apgd_ref import within_ball as _within_ball
from smoothing_ref import linear_case, linear_classify, philox4x32  # noqa: F401

AMBIGUITY = 1e-5  # of the total weight: the issue's definition of an ambiguous draw


def _words(seed, n, hi0, hi1, flag=0):
    """uint64 [n]: word k & 3 of the block gen(seed; (k >> 2) | flag, hi0, hi1) for every element k."""
    quads = (n + 3) // 4
    o = philox4x32(seed, np.arange(quads, dtype=np.uint64) | np.uint64(flag), hi0, hi1)  # [4, quads]
    return o.T.reshape(-1)[:n]


def breed(x0, pop, generation, seed, thresh, step, eps, pop_in=None, parents=None, n_valid=None, clip0=0, lo=-np.inf, hi=np.inf):
    """x0 float32 [B, n] -> dict: want float64 [B, pop, n]; pick, mut, valid bool [B, pop, n] (pick: the element comes from parent
    c); copied bool [B, pop]; low / high bool [B, pop, n]: the clamp that binds in exact arithmetic (there the result is the bound
    itself); v float64 [B, pop, n] the amplitudes."""
    x0 = np.asarray(x0, dtype=np.float32)
    B, n = x0.shape
    nv = np.full(B, n) if n_valid is None else np.clip(np.asarray(n_valid, dtype=np.int64), 0, n)
    want = np.zeros((B, pop, n))
    pick, mut, valid = (np.zeros((B, pop, n), dtype=bool) for _ in range(3))
    low, high = np.zeros((B, pop, n), dtype=bool), np.zeros((B, pop, n), dtype=bool)
    amp = np.zeros((B, pop, n))
    copied = np.zeros((B, pop), dtype=bool)
    eps32 = np.float32(eps)
    for b in range(B):
        l32, h32 = (x0[b] - eps32).astype(np.float32), (x0[b] + eps32).astype(np.float32)  # one fp32 rounding each, as the kernel's
        inside = np.arange(n) < nv[b]
        for p in range(pop):
            valid[b, p] = inside
            if pop_in is None:
                a = c = x0[b].astype(np.float64)
            else:
                ia, ic = int(parents[b][p][0]), int(parents[b][p][1])
                a = np.asarray(pop_in[b][min(max(ia, 0), pop - 1)], dtype=np.float64)
                if ic < 0:
                    copied[b, p] = True
                    want[b, p] = np.where(inside, a, x0[b])
                    continue
                c = np.asarray(pop_in[b][min(ic, pop - 1)], dtype=np.float64)
            key = generation * 256 + p
            o = _words(seed, n, clip0 + b, key)
            m = _words(seed, n, clip0 + b, key, flag=1 << 63)
            pk = (o & np.uint64(1)) == 1
            mu = (o >> np.uint64(8)) < np.uint64(thresh)
            v = 2.0 * (((m >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0) - 1.0
            t = np.where(pk, c, a) + np.where(mu, float(np.float32(step)) * v, 0.0)
            # clamp to the ball, then to the clip range: the later clamp wins where the two disagree
            t1 = np.clip(t, l32, h32)
            t2 = np.clip(t1, lo, hi)
            low[b, p] = inside & (t2 != t) & (t2 > t)
            high[b, p] = inside & (t2 != t) & (t2 < t)
            want[b, p] = np.where(inside, t2, x0[b])
            pick[b, p], mut[b, p], amp[b, p] = pk, mu, v
    return dict(want=want, pick=pick, mut=mut, valid=valid, copied=copied, low=low, high=high, v=amp)


def fitness(logits, labels, pop, targeted=False):
    """float32 logits [B * pop, C] -> float64 [B, pop]."""
    z = np.asarray(logits, dtype=np.float64)
    rows, C = z.shape
    B = rows // pop
    y = np.repeat(np.asarray(labels, dtype=np.int64), pop)
    ok = (y >= 0) & (y < C)
    yc = np.clip(y, 0, C - 1)
    zy = z[np.arange(rows), yc]
    masked = np.where(np.isnan(z), -np.inf, z)
    masked[np.arange(rows), yc] = -np.inf
    other = masked.max(axis=1)
    with np.errstate(invalid="ignore"):
        f = zy - other if targeted else other - zy
    f[np.isnan(z).any(axis=1) | np.isnan(f) | ~ok] = -np.inf
    return f.reshape(B, pop)


def select(logits, labels, pop, generation, seed, temperature, targeted=False, clip0=0, done=None):
    """-> dict: fitness float64 [B, pop], best int [B] (-1: the clip arrived done, best is kept), done int [B], parents int
    [B, pop, 2], alt int [B, pop, 2] (the other index an ambiguous draw may give; equal to parents elsewhere), drawn bool [B, pop]:
    the children whose parents were drawn."""
    f = fitness(logits, labels, pop, targeted)
    B = f.shape[0]
    done = np.zeros(B, dtype=np.int64) if done is None else np.array(done, dtype=np.int64)
    best = np.full(B, -1, dtype=np.int64)
    parents = np.zeros((B, pop, 2), dtype=np.int64)
    alt = np.zeros((B, pop, 2), dtype=np.int64)
    drawn = np.zeros((B, pop), dtype=bool)
    T = float(np.float32(temperature))
    for b in range(B):
        bi = int(np.argmax(f[b]))  # the lowest index on a tie
        frozen = done[b] != 0
        if not frozen:
            best[b] = bi
            if f[b, bi] > 0:
                done[b] = generation + 1
                frozen = True
        if frozen or not f[b, bi] > -np.inf:
            parents[b, :, 0], parents[b, :, 1] = np.arange(pop), -1
            alt[b] = parents[b]
            continue
        with np.errstate(over="ignore"):
            w = np.where(f[b] > -np.inf, np.exp((f[b] - f[b, bi]) / T), 0.0)
        cum = np.cumsum(w)
        total = cum[-1]
        parents[b, 0] = alt[b, 0] = (bi, -1)
        for p in range(1, pop):
            o = philox4x32(seed, np.array([p | (1 << 62)], dtype=np.uint64), clip0 + b, generation * 256)[:, 0]
            for k in range(2):
                u = (float(int(o[k]) >> 8) + 1.0) / 16777216.0
                t = u * total
                first = lambda x: min(int(np.searchsorted(cum, x, side="left")), pop - 1)
                parents[b, p, k] = first(t)
                lo_i, hi_i = first(t - AMBIGUITY * total), first(t + AMBIGUITY * total)
                alt[b, p, k] = hi_i if lo_i == parents[b, p, k] else lo_i
            drawn[b, p] = True
    return dict(fitness=f, best=best, done=done, parents=parents, alt=alt, drawn=drawn)


def attack(classify, x, labels, eps, pop=20, max_iter=500, mutation_p=0.0005, step=None, temperature=0.01, targeted=False, seed=0,
           n_valid=None, lo=-np.inf, hi=np.inf):
    """The loop of GeneticAttack.generate_device without chunks -> dict: adv float32 [B, n], success bool [B], generations int [B]
    (populations evaluated until the clip was done, or max_iter), fitness float64 [B]."""
    x = np.asarray(x, dtype=np.float32)
    B, n = x.shape
    thresh = int(round(float(mutation_p) * 16777216.0))
    step = eps if step is None else step
    kw = dict(n_valid=n_valid, lo=lo, hi=hi)
    cur = breed(x, pop, 0, seed, thresh, step, eps, **kw)["want"].astype(np.float32)
    done = np.zeros(B, dtype=np.int64)
    best = np.zeros(B, dtype=np.int64)
    fit = np.full(B, -np.inf)
    for g in range(max_iter):
        r = select(classify(cur.reshape(B * pop, n).astype(np.float64)), labels, pop, g, seed, temperature, targeted, done=done)
        done = r["done"]
        best = np.where(r["best"] >= 0, r["best"], best)
        fit = r["fitness"][np.arange(B), best]
        if g + 1 == max_iter or (done != 0).all():
            break
        cur = breed(x, pop, g + 1, seed, thresh, step, eps, pop_in=cur, parents=r["parents"], **kw)["want"].astype(np.float32)
    return dict(adv=cur[np.arange(B), best], success=done != 0, generations=np.where(done != 0, done, g + 1), fitness=fit)


def within_ball(adv, x, eps):
    """|adv - x| <= eps plus one unit in the last place of the bound: the ball's bounds are the fp32 numbers x -+ eps."""
    return _within_ball(np.asarray(adv, dtype=np.float32), np.asarray(x, dtype=np.float32), float(np.float32(eps)), np.inf)


# ---- the linear two-class case, restated for L-inf: six rows at (almost) the same distance from the boundary
LINEAR_SEED = 0
LINEAR = dict(pop=16, mutation_p=0.05, temperature=0.01)


def linear_case_inf(seed=LINEAR_SEED, n=880):
    """smoothing_ref.linear_case with six rows at L2 distance 0.25 -> (W, bias, x float32 [6, n], d float64 [6], cls int [6]): d is the
    L-inf distance of each float32 row to the boundary, |w . x + c| / ||w||_1 -- no perturbation of a smaller L-inf norm changes the
    class (Hoelder), and x -+ d sign(w) reaches the boundary."""
    W, bias, x, _, cls = linear_case(seed, 0.25, n=n, factors=(1.0,) * 6)
    w = W[:, 0].astype(np.float64) - W[:, 1].astype(np.float64)
    c = float(bias[0]) - float(bias[1])
    d = np.abs(x.astype(np.float64) @ w + c) / np.abs(w).sum()
    return W, bias, x, d, cls
