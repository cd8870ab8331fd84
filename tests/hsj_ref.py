"""Oracle of HopSkipJump (lipasr_hsj_expand / _accumulate / _direction / _search, their host twins, lipasr.hopskipjump.HopSkipJump):
a NumPy restatement.  TEST INFRASTRUCTURE for tests/test_hsj_*: nothing here is used by the library.

    philox_np     philox_ref's, re-exported (pinned against philox, Python integers, by test_hsj_cpu)
    fmaf32 / fma64   a * b + c rounded once: float32 through round-to-odd in float64, float64 through an exact product and fsum
    adversarial   the decision on one row of logits
    draw          one draw r (before scaling): L-inf exact, L2 Box-Muller in float64 or float32
    expand, accumulate, direction, search   the four calls (search in place on a state dict)
    run           a whole attack over any ``predict`` (float32 rows -> float32 logits) for one chunk of rows

Everything is float64 except where bits are claimed: the L-inf draws, the points fmaf writes, the fp64 sums in ascending j, g, the
sign, and every scalar of the search are the kernels' bits; the L2 norms are serial or pairwise float64 sums (n 2^-52 relative)."""
from __future__ import annotations

import math

import numpy as np

from philox_ref import nv as _nv, philox, philox_np  # noqa: F401  (re-exported under the names the tests import)

TAG_START, TAG_L2, TAG_LINF = 1 << 28, 2 << 28, 3 << 28
START, HALVE, BISECT = 0, 1, 2
FIRST, LAST = 1, 2
F = {"lo": 0, "hi": 1, "mid": 2, "thresh": 3, "eps": 4, "dist": 5, "dist_best": 6, "dist_far": 7}
I = {"active": 0, "found": 1, "ok": 2, "moved": 3, "halvings": 4, "queries": 5}
f32 = np.float32
INF = f32(np.inf)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fmaf32(a, b, c):
    """float32 fmaf(a, b, c): the product of two float32 is exact in float64; the sum is rounded to odd there, so that the second
    rounding, to float32, is the only one that counts."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        s, e = _two_sum(a * b, c)
        bits = np.ascontiguousarray(s).view(np.int64)
        odd = np.where((e != 0) & np.isfinite(s) & (bits & 1 == 0), np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return odd.astype(np.float32)


def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp / Dekker, no overflow or underflow assumed)."""
    p = a * b
    split = 134217729.0
    ah = a * split
    ah = ah - (ah - a)
    al = a - ah
    bh = b * split
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """float64 fma(a, b, c) element by element: the exact product as two doubles, then math.fsum, which rounds the exact sum once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p, e = _two_prod(a, b)
    return np.array([math.fsum(t) for t in zip(p.ravel().tolist(), e.ravel().tolist(), c.ravel().tolist())], dtype=np.float64).reshape(a.shape)


def clampf(v, lo, hi):
    v = np.asarray(v, dtype=np.float32)
    lo, hi = f32(lo), f32(hi)
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(np.float32)


def adversarial(z, y, targeted=False):
    z = np.asarray(z, dtype=np.float32)
    if not 0 <= y < z.shape[0] or np.isnan(z).any():
        return False
    p = int(np.argmax(z))  # the first maximum
    return p == y if targeted else p != y


def draw(l2, seed, clip, it, j, n, nv, dtype=np.float64):
    """Draw ``j`` of iteration ``it`` of clip ``clip`` -> (r [n] (float32 for L-inf, ``dtype`` for L2), sum of squares: a Python
    integer of (r 2^23)^2 for L-inf, a float64 for L2).  Elements at or beyond nv are 0."""
    quads = (n + 3) // 4
    w = philox_np(seed, np.arange(quads), j, clip, (TAG_L2 if l2 else TAG_LINF) | it)  # [4, quads]
    if not l2:
        k = ((w >> np.uint64(8)).astype(np.int64) + 1 - (1 << 23)).T.reshape(-1)[:n]
        k[nv:] = 0
        assert n <= 1 << 17  # the sum below fits 64 bits
        return (k.astype(np.float32) / f32(8388608.0)).astype(np.float32), int(np.sum((k * k).astype(np.uint64)))
    u = (((w >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0).astype(np.float32).astype(dtype)  # u01, exact in float32
    two_pi = dtype(6.283185307179586) if dtype is np.float32 else 2.0 * np.pi
    r0, r1 = np.sqrt(dtype(-2.0) * np.log(u[0])), np.sqrt(dtype(-2.0) * np.log(u[2]))
    t0, t1 = two_pi * u[1], two_pi * u[3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)]).astype(dtype).T.reshape(-1)[:n]
    z[nv:] = 0
    return z, float(np.sum(z.astype(np.float64) ** 2))


def scale(l2, ss, delta):
    """delta / ||r||_2 as the kernels round it: float32 of a float64 quotient; 0 for an empty draw or a delta that is not finite."""
    nrm = math.sqrt(ss) if l2 else math.sqrt(float(ss)) / 8388608.0
    if not (nrm > 0.0 and math.isfinite(nrm) and math.isfinite(float(delta))):
        return f32(0.0)
    return f32(float(f32(delta)) / nrm)


def expand(x, delta, draws, it, seed, norm, n_valid=None, clip0=0, draw0=0, lo=-np.inf, hi=np.inf, dtype=np.float64):
    """-> [B * draws, n].  L-inf: float32, the kernels' bits.  L2: ``dtype`` float64 is the real-number statement (the point in
    float64, from float64 draws); float32 is the kernels' arithmetic with NumPy's float32 log / sin / cos."""
    x = np.asarray(x, dtype=np.float32)
    B, n = x.shape
    l2 = norm == 2
    exact = not l2 or dtype is np.float32
    out = np.zeros((B * draws, n), dtype=np.float32 if exact else np.float64)
    for b in range(B):
        nv = _nv(n_valid, b, n)
        for j in range(draws):
            r, ss = draw(l2, seed, clip0 + b, it, draw0 + j, n, nv, dtype)
            if exact:
                v = clampf(fmaf32(scale(l2, ss, delta[b]), r, x[b]), lo, hi)
            else:
                nrm = math.sqrt(ss)
                s = float(delta[b]) / nrm if nrm > 0 and math.isfinite(float(delta[b])) else 0.0
                v = np.clip(x[b].astype(np.float64) + s * r, lo, hi)
            out[b * draws + j] = np.where(np.arange(n) < nv, v, x[b])
    return out


def accumulate(logits, labels, p, x, sums, counts, n_valid=None, targeted=False):
    """In place on sums float64 [B, 2, n] and counts int32 [B, 2], ascending j: the kernels' bits."""
    x = np.asarray(x, dtype=np.float32)
    B, n = x.shape
    draws = len(p) // B
    for b in range(B):
        nv = _nv(n_valid, b, n)
        for j in range(draws):
            plus = adversarial(logits[b * draws + j], int(labels[b]), targeted)
            d = np.where(np.arange(n) < nv, p[b * draws + j].astype(np.float64) - x[b].astype(np.float64), 0.0)
            sums[b, 0] += d
            sums[b, 1] += d if plus else -d
            counts[b, 1] += int(plus)
        counts[b, 0] += draws


def g_of(s0, s1, total, pos):
    if total <= 0:
        return np.zeros_like(s0)
    if pos >= total:
        return s0.copy()
    if pos <= 0:
        return -s0
    return fma64(-((2 * pos - total) / total), s0, s1)


def direction(sums, counts, norm, n_valid=None):
    """-> (u float32 [B, n], g float64 [B, n]).  g and sign(g) are the kernels' bits; the L2 norm is a NumPy float64 sum."""
    B, _, n = sums.shape
    u, g = np.zeros((B, n), dtype=np.float32), np.zeros((B, n))
    for b in range(B):
        nv = _nv(n_valid, b, n)
        g[b, :nv] = g_of(sums[b, 0, :nv], sums[b, 1, :nv], int(counts[b, 0]), int(counts[b, 1]))
        if norm == 2:
            nrm = math.sqrt(float(np.sum(g[b, :nv] ** 2)))
            if nrm > 0 and math.isfinite(nrm):
                with np.errstate(invalid="ignore"):
                    u[b, :nv] = np.where(np.isnan(g[b, :nv]), 0.0, g[b, :nv] / nrm).astype(np.float32)
        else:
            u[b, :nv] = np.sign(np.nan_to_num(g[b, :nv], nan=0.0)).astype(np.float32)
    return u, g


def proj(l2, a, x0, xf, lo, hi):
    a = f32(a)
    if l2:
        v = fmaf32(a, xf, fmaf32(-a, x0, x0))
    else:
        with np.errstate(invalid="ignore"):
            l, h = (x0 - a).astype(np.float32), (x0 + a).astype(np.float32)
            v = np.where(xf < l, l, np.where(xf > h, h, xf)).astype(np.float32)
    return clampf(v, lo, hi)


def start_draw(seed, clip, j, n, sl, sh):
    quads = (n + 3) // 4
    w = philox_np(seed, np.arange(quads), j, clip, TAG_START)
    u = (((w >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0).astype(np.float32).T.reshape(-1)[:n]
    with np.errstate(invalid="ignore"):
        return clampf(fmaf32(u, f32(sh) - f32(sl), f32(sl)), sl, sh)


def new_state(B, n, attack=None):
    st = dict(x_cand=np.zeros((B, n), dtype=np.float32), x_far=np.zeros((B, n), dtype=np.float32), x_adv=np.zeros((B, n), dtype=np.float32),
              x_best=np.zeros((B, n), dtype=np.float32), f=np.zeros((B, 8), dtype=np.float32), i=np.zeros((B, 8), dtype=np.int32))
    if attack is not None:
        st["i"][:, 0] = np.asarray(attack).astype(np.int32)
    return st


def search(st, logits, labels, x0, mode, flags, seed, norm, start_lo, start_hi, theta, u=None, n_valid=None, targeted=False, clip0=0,
           draw=0, step_scale=1.0, max_halvings=25, lo=-np.inf, hi=np.inf):
    """One lipasr_hsj_search in place on st = dict(x_cand, x_far, x_adv, x_best float32 [B, n], f float32 [B, 8], i int32 [B, 8])."""
    x0 = np.asarray(x0, dtype=np.float32)
    B, n = x0.shape
    l2 = norm == 2
    first, last = bool(flags & FIRST), bool(flags & LAST)
    inside_all = np.arange(n)
    for b in range(B):
        nv = _nv(n_valid, b, n)
        inside = inside_all < nv
        f, i, c = st["f"][b], st["i"][b], x0[b]
        adv = False if first else adversarial(logits[b], int(labels[b]), targeted)
        cand = far_from_cand = finish = 0
        if mode == START:
            if first:
                act = int(i[0] != 0 and nv > 0)
                f[:5] = 0
                f[5:] = INF
                i[:] = 0
                i[0] = act
                st["x_adv"][b] = st["x_best"][b] = c
                st["x_cand"][b] = np.where(inside, start_draw(seed, clip0 + b, 0, n, start_lo[b], start_hi[b]), c) if act else c
            elif i[0]:
                i[5] += 1
                if adv:
                    far_from_cand, i[1], i[2], i[0] = 1, 1, 1, 0
                elif last:
                    i[0] = 0
                else:
                    st["x_cand"][b] = np.where(inside, start_draw(seed, clip0 + b, draw + 1, n, start_lo[b], start_hi[b]), c)
        elif mode == HALVE:
            if first:
                i[0], i[2], i[4] = int(i[1] != 0 and nv > 0), 0, 0
                with np.errstate(invalid="ignore"):
                    f[4] = f[5] * f32(step_scale)
                cand = 2 if i[0] else 0
            elif i[0]:
                i[5] += 1
                if adv:
                    far_from_cand, i[2], i[0] = 1, 1, 0
                else:
                    i[4] += 1
                    if i[4] >= max_halvings:
                        i[0] = 0
                    else:
                        f[4] = f[4] * f32(0.5)
                        cand = 2
        else:
            advance = False
            if first:
                i[0], i[3] = int(i[2] != 0 and nv > 0), 0
                if i[0]:
                    dist_far = f32(0.0) if l2 else np.max(np.abs(st["x_far"][b, :nv] - c[:nv]), initial=f32(0.0)).astype(np.float32)
                    f[7], f[0] = dist_far, 0
                    f[1] = f32(1.0) if l2 else dist_far
                    with np.errstate(invalid="ignore"):
                        dt = f32(dist_far * theta[b])
                    f[3] = theta[b] if l2 else (dt if dt < theta[b] else theta[b])
                    advance = True
            elif i[0]:
                i[5] += 1
                if adv:
                    f[1], i[3] = f[2], 1
                else:
                    f[0] = f[2]
                advance = True
            if advance:
                with np.errstate(invalid="ignore"):
                    mid = f32(0.5) * (f[0] + f[1])
                    done = not (f[1] - f[0] > f[3]) or not (mid > f[0] and mid < f[1])
                if done:
                    finish, i[0] = 1, 0
                else:
                    f[2] = mid
                    st["x_cand"][b] = np.where(inside, proj(l2, mid, c, st["x_far"][b], lo, hi), c)
        if far_from_cand:
            st["x_far"][b] = st["x_cand"][b]
        if cand == 2:
            st["x_cand"][b] = np.where(inside, clampf(fmaf32(f[4], u[b], st["x_adv"][b]), lo, hi), c)
        if finish:
            v = np.where(inside, proj(l2, f[1], c, st["x_far"][b], lo, hi) if i[3] else st["x_far"][b], c)
            st["x_adv"][b] = v
            d = v[:nv].astype(np.float64) - c[:nv].astype(np.float64)
            f[5] = f32(math.sqrt(float(np.sum(d * d)))) if l2 else np.max(np.abs(v[:nv] - c[:nv]), initial=f32(0.0))
            if f[5] < f[6]:
                f[6] = f[5]
                st["x_best"][b] = v


def distance(a, x0, norm, nv=None):
    d = (np.asarray(a, dtype=np.float64) - np.asarray(x0, dtype=np.float64))[..., :nv]
    return np.sqrt(np.sum(d * d, axis=-1)) if norm == 2 else np.max(np.abs(d), axis=-1, initial=0.0)


def evals(t, init_eval, max_eval):
    return min(int(init_eval * math.sqrt(t)), max_eval)


def run(predict, x0, labels, norm, max_iter, init_eval=100, max_eval=1000, init_size=100, seed=0, gamma=0.01, max_halvings=25, clip=None,
        n_valid=None, targeted=False, x_adv_init=None, clip0=0, dtype=np.float32):
    """HopSkipJump over all rows at once -> dict: x_best, dist_best, start_dist float32, queries, found, dists [max_iter + 1, B] (the
    iterate's distance after the start and after every iteration).  ``dtype``: of the L2 draws (see expand)."""
    x0 = np.asarray(x0, dtype=np.float32)
    B, n = x0.shape
    l2 = norm == 2
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    nvs = np.array([_nv(n_valid, b, n) for b in range(B)])
    with np.errstate(divide="ignore"):
        theta = np.where(nvs > 0, gamma / np.sqrt(nvs.astype(np.float64)) if l2 else gamma / nvs.astype(np.float64), 0.0).astype(np.float32)
    if clip is None:
        sl = np.array([x0[b, :nvs[b]].min(initial=np.inf) for b in range(B)], dtype=np.float32)
        sh = np.array([x0[b, :nvs[b]].max(initial=-np.inf) for b in range(B)], dtype=np.float32)
        sl[nvs == 0] = sh[nvs == 0] = 0
    else:
        sl, sh = np.full(B, lo, dtype=np.float32), np.full(B, hi, dtype=np.float32)
    z = predict(x0)
    already = np.array([adversarial(z[b], int(labels[b]), targeted) for b in range(B)])
    st = new_state(B, n, ~already if x_adv_init is None else None)
    kw = dict(labels=labels, x0=x0, seed=seed, norm=norm, start_lo=sl, start_hi=sh, theta=theta, n_valid=n_valid, targeted=targeted,
              clip0=clip0, max_halvings=max_halvings, lo=lo, hi=hi)
    search(st, None, mode=START, flags=FIRST, **kw)
    if x_adv_init is None:
        for k in range(init_size):
            if not st["i"][:, 0].any():
                break
            search(st, predict(st["x_cand"]), mode=START, flags=LAST if k + 1 == init_size else 0, draw=k, **kw)
    else:
        zi = predict(np.asarray(x_adv_init, dtype=np.float32))
        take = ~already & np.array([adversarial(zi[b], int(labels[b]), targeted) for b in range(B)])
        st["x_far"][:] = np.where(take[:, None], x_adv_init, x0)
        st["i"][:, 1] = st["i"][:, 2] = take

    def phase(mode, limit, **more):
        search(st, None, mode=mode, flags=FIRST, **kw, **more)
        for _ in range(limit):
            if not st["i"][:, 0].any():
                break
            search(st, predict(st["x_cand"]), mode=mode, flags=0, **kw, **more)

    phase(BISECT, 256)
    start_dist = st["f"][:, 5].copy()
    dists = [start_dist.copy()]
    u = np.zeros((B, n), dtype=np.float32)
    kw["u"] = u
    for t in range(1, max_iter + 1):
        if not st["i"][:, 1].any():
            break
        with np.errstate(invalid="ignore"):
            delta = ((sh - sl) * f32(0.1) if t == 1 else st["f"][:, 5] * f32(gamma)).astype(np.float32)
        E = evals(t, init_eval, max_eval)
        p = expand(st["x_adv"], delta, E, t, seed, norm, n_valid, clip0, 0, lo, hi, dtype=dtype if l2 else np.float64).astype(np.float32)
        sums, counts = np.zeros((B, 2, n)), np.zeros((B, 2), dtype=np.int32)
        accumulate(predict(p), labels, p, st["x_adv"], sums, counts, n_valid, targeted)
        u[:] = direction(sums, counts, norm, n_valid)[0]
        st["i"][:, 5] += st["i"][:, 1] * E
        phase(HALVE, max_halvings, step_scale=f32(1.0 / math.sqrt(t)))
        phase(BISECT, 256)
        dists.append(st["f"][:, 5].copy())
    found = st["i"][:, 1] != 0
    return dict(x_best=np.where(found[:, None], st["x_best"], x0), dist_best=np.where(already, f32(0), st["f"][:, 6]).astype(np.float32),
                start_dist=start_dist, queries=st["i"][:, 5].astype(np.int64), found=found, already=already, dists=np.array(dists), state=st)
