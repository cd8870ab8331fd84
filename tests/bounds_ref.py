"""float64 NumPy restatement of bound propagation for the dense classifier: IBP, the margins, CROWN-IBP and the bisection driver,
written from the formulas of DESIGN.md ("Bound propagation"), not from the kernels.  Also the float64 network, the widening
constants as functions of K, and the case builder of tests/test_bounds_cpu.py and tests/test_bounds_gpu.py.

A model is a dict: widths [n_0 .. n_L], W[l] float32 [n_l, n_{l+1}], b[l] float32, bn[l] = None or (gamma, beta, mean, var).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
D = 2.0 ** -40
BN_EPS = float(np.float32(1e-3))
INF = float("inf")


def gamma(n):
    return n * U / (1.0 - n * U)


def widen(K, S):
    """What two fp32 fmaf chains of K products plus the bias can be off by together, S = sum |W| (|c| + r) + |b|."""
    return gamma(K + 1) * S + 2.0 * (K + 1) * TINY


# ------------------------------------------------------------------------------------------------------------------- the model
def make_model(widths, seed, *, bn=(), signed=True, scale=1.0):
    rng = np.random.default_rng(seed)
    L = len(widths) - 1
    m = {"widths": list(widths), "W": [], "b": [], "bn": []}
    for l in range(L):
        ni, no = widths[l], widths[l + 1]
        W = rng.standard_normal((ni, no)) * scale / np.sqrt(ni)
        if not signed and l + 1 < L:
            W = np.abs(W)  # NonNeg on the hidden kernels, as the reference constrains them
        m["W"].append(W.astype(np.float32))
        m["b"].append((0.1 * rng.standard_normal(no)).astype(np.float32))
        if l in bn and l + 1 < L:
            g = rng.uniform(0.5, 1.5, no) * np.where(rng.random(no) < 0.3, -1.0, 1.0)
            g[0] = 0.0
            g[1] = -abs(g[1]) - 0.1
            m["bn"].append((g.astype(np.float32), (0.1 * rng.standard_normal(no)).astype(np.float32),
                            (0.2 * rng.standard_normal(no)).astype(np.float32), rng.uniform(0.5, 2.0, no).astype(np.float32)))
        else:
            m["bn"].append(None)
    return m


def bn_flags(m):
    return [0 if p is None else 1 for p in m["bn"]]


def pack(m, layout):
    """(params, bnstate) float32 in the flat layout `layout` = lipasr._native.bounds_layout(widths, bn)."""
    offs, n_params, n_state = layout
    params, state = np.zeros(max(n_params, 1), np.float32), np.zeros(max(n_state, 1), np.float32)
    for l, d in enumerate(offs):
        W, b = m["W"][l], m["b"][l]
        params[d["W"]:d["W"] + W.size] = W.reshape(-1)
        params[d["b"]:d["b"] + b.size] = b
        if m["bn"][l] is not None:
            g, be, mean, var = m["bn"][l]
            params[d["gamma"]:d["gamma"] + g.size] = g
            params[d["beta"]:d["beta"] + g.size] = be
            state[d["mean"]:d["mean"] + g.size] = mean
            state[d["var"]:d["var"] + g.size] = var
    return params, state


def affine(m, l):
    n = m["widths"][l + 1]
    if m["bn"][l] is None:
        return np.ones(n), np.zeros(n)
    g, be, mean, var = (a.astype(np.float64) for a in m["bn"][l])
    s = g / np.sqrt(var + BN_EPS)
    return s, be - s * mean


def forward(m, x):
    """float64 logits [.., C] of float64 inputs [.., n_0]."""
    h = np.asarray(x, np.float64)
    L = len(m["W"])
    for l in range(L):
        z = h @ m["W"][l].astype(np.float64) + m["b"][l].astype(np.float64)
        if l + 1 == L:
            return z
        s, t = affine(m, l)
        h = s * np.maximum(z, 0.0) + t


def true_margins(m, x, y):
    z = forward(m, x)
    return z[..., [y]] - z


def margin_grad(m, x, y, k):
    """Gradient of z_y - z_k at x (float64), by backpropagation."""
    h = np.asarray(x, np.float64)
    L = len(m["W"])
    masks = []
    for l in range(L - 1):
        z = h @ m["W"][l].astype(np.float64) + m["b"][l]
        masks.append(z > 0)
        s, t = affine(m, l)
        h = s * np.maximum(z, 0.0) + t
    g = m["W"][L - 1][:, y].astype(np.float64) - m["W"][L - 1][:, k]
    for l in range(L - 2, -1, -1):
        s, _ = affine(m, l)
        g = m["W"][l].astype(np.float64) @ (g * s * masks[l])
    return g


# ------------------------------------------------------------------------------------------------------------------------ IBP
def input_box(x, eps, clip):
    x = np.asarray(x, np.float64)
    e = np.asarray(eps, np.float64)[:, None]
    return np.maximum(x - e, clip[0]), np.minimum(x + e, clip[1])


def ibp_layer(m, l, lo, hi, l2=None):
    """(z_lo, z_hi, S) of layer l over the box [lo, hi] of its input; l2 = (x, eps): the first layer under norm 2."""
    W, b = m["W"][l].astype(np.float64), m["b"][l].astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if l2 is None:
        c, r = (lo + hi) / 2, (hi - lo) / 2
    else:
        c = np.asarray(l2[0], np.float64)
        r = np.maximum(np.maximum(hi - c, c - lo), 0.0)
    rad = r @ np.abs(W)
    if l2 is not None:
        rad = np.minimum(rad, np.asarray(l2[1], np.float64)[:, None] * np.sqrt((W * W).sum(0))[None, :])
    zc = c @ W + b
    S = (np.abs(c) + r) @ np.abs(W) + np.abs(b)
    return zc - rad, zc + rad, S


def post_box(m, l, zlo, zhi):
    s, t = affine(m, l)
    a, bb = np.maximum(zlo, 0.0), np.maximum(zhi, 0.0)
    return np.where(s >= 0, s * a + t, s * bb + t), np.where(s >= 0, s * bb + t, s * a + t)


def ibp(m, x, eps, norm, clip):
    """dict(box=(lo0, hi0), z=[(zlo, zhi)], h=[(hlo, hhi)]) over the hidden layers, in float64."""
    lo, hi = input_box(x, eps, clip)
    out = {"box": (lo, hi), "z": [], "h": []}
    for l in range(len(m["W"]) - 1):
        zlo, zhi, _ = ibp_layer(m, l, lo, hi, (x, eps) if (norm == 2 and l == 0) else None)
        lo, hi = post_box(m, l, zlo, zhi)
        out["z"].append((zlo, zhi))
        out["h"].append((lo, hi))
    return out


def input_min(a, lo, hi, norm, x, eps):
    """min over the input set of a . v for rows a [.., n]: the box coordinate by coordinate, under norm 2 also the ball."""
    v = np.minimum(a * lo, a * hi).sum(-1)
    if norm == 2:
        v = np.maximum(v, (a * x).sum(-1) - eps * np.sqrt((a * a).sum(-1)))
    return v


def margins_ibp(m, b, y, lo, hi, norm=INF, x=None, eps=0.0):
    """IBP margins [C] of row b from the box of the last hidden layer (or, for one layer, the input set)."""
    WL, bL = m["W"][-1].astype(np.float64), m["b"][-1].astype(np.float64)
    d = (WL[:, [y]] - WL).T  # [C, n]
    one = len(m["W"]) == 1
    out = input_min(d, lo[b], hi[b], norm if one else INF, None if x is None else np.asarray(x[b], np.float64), eps) + bL[y] - bL
    out[y] = INF
    return out


def crown(m, b, y, boxes, norm, x, eps):
    """CROWN-IBP margins [C] of row b from the pre-activation boxes `boxes` = dict(box=, z=), and `drift` [C]: a bound on how far an
    fp32 run of the same chain (every coefficient rounded once, every product an fmaf chain) can move the value before its own
    slack is taken off; and `gap` [C]: what the ReLU lines themselves can lose against the true margin (half the width of every
    unstable box times its coefficient, pushed down to the input as is: 0 where every neuron is stable).  All computed, in float64."""
    L = len(m["W"])
    WL, bL = m["W"][-1].astype(np.float64), m["b"][-1].astype(np.float64)
    lam = (WL[:, [y]] - WL).T  # [C, n_{L-1}]
    const = bL[y] - bL
    dl = U * np.abs(lam)  # coefficient uncertainty of the fp32 chain
    dc = np.zeros_like(const)
    gap = np.zeros_like(const)
    for l in range(L - 2, -1, -1):
        zlo, zhi = (np.asarray(a[b], np.float64) for a in boxes["z"][l])
        s, t = affine(m, l)
        const = const + lam @ t
        dc = dc + dl @ np.abs(t)
        p = lam * s
        unstable = (zlo < 0) & (zhi > 0)
        sig = np.where(unstable, zhi / np.where(unstable, zhi - zlo, 1.0), 0.0)
        slope = np.where(zhi <= 0, 0.0, np.where(zlo >= 0, 1.0, np.where(p < 0, sig, np.where(zhi >= -zlo, 1.0, 0.0))))
        icpt = np.where(unstable & (p < 0), -p * sig * zlo, 0.0)
        const = const + icpt.sum(-1)
        nu = p * slope
        gap = gap + (np.abs(p) * np.where(unstable, (zhi - zlo) / 2, 0.0)).sum(-1)
        # a coefficient that is off by dl gives a slope-1 change at most (opposite signs included), and moves the intercept
        dp = dl * np.abs(s)
        dc = dc + (dp * np.where(unstable, sig * np.abs(zlo), 0.0)).sum(-1) + D * (np.abs(lam) @ np.abs(t) + np.abs(icpt).sum(-1))
        dnu = dp * np.where(unstable, 1.0, slope) * (1 + U) + 2 * U * np.abs(nu) + TINY
        W, bb = m["W"][l].astype(np.float64), m["b"][l].astype(np.float64)
        K = W.shape[1]
        const = const + nu @ bb
        dc = dc + dnu @ np.abs(bb)
        lam = nu @ W.T
        dl = dnu @ np.abs(W).T + gamma(K + 1) * ((np.abs(nu) + dnu) @ np.abs(W).T) + (K + 1) * TINY
    lo0, hi0 = boxes["box"][0][b].astype(np.float64), boxes["box"][1][b].astype(np.float64)
    xb = np.asarray(x[b], np.float64)
    out = input_min(lam, lo0, hi0, norm, xb, eps) + const
    H = np.maximum(np.maximum(np.abs(lo0), np.abs(hi0)), np.abs(xb))
    drift = dc + dl @ H + (eps * np.sqrt((dl * dl).sum(-1)) if norm == 2 else 0.0) + 4 * D * (np.abs(lam) @ H + np.abs(const))
    out[y] = INF
    drift[y] = 0.0
    return out, drift, gap


def bound_margins(m, x, eps, norm, clip, y, method="crown-ibp"):
    """float64 margins [B, C]: max(IBP, CROWN-IBP), or IBP alone."""
    x = np.asarray(x, np.float64)
    eps = np.asarray(eps, np.float64)
    bx = ibp(m, x, eps, norm, clip)
    lo, hi = bx["h"][-1] if bx["h"] else bx["box"]
    out = np.zeros((x.shape[0], m["widths"][-1]))
    for b in range(x.shape[0]):
        out[b] = margins_ibp(m, b, int(y[b]), lo, hi, norm, x, eps[b])
        if method == "crown-ibp":
            out[b] = np.maximum(out[b], crown(m, b, int(y[b]), bx, norm, x, eps[b])[0])
    return out


def certified_radius(m, x, norm, clip, y, eps_max, steps, method="crown-ibp"):
    """Per-row bisection: the largest eps tested at which the row was certified; 0 if none, 0 for a misclassified row.  Also the
    list of (eps, min margin) per step, for a test that allows one step of disagreement."""
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    ok0 = forward(m, x).argmax(-1) == np.asarray(y)
    lo, hi, best = np.zeros(B), np.full(B, float(eps_max)), np.zeros(B)
    eps = hi.copy()
    trace = []
    for _ in range(steps):
        mm = bound_margins(m, x, eps, norm, clip, y, method).min(-1)
        trace.append((eps.copy(), mm))
        cert = (mm > 0) & ok0
        best = np.where(cert, np.maximum(best, eps), best)
        lo = np.where(cert, eps, lo)
        hi = np.where(cert, hi, eps)
        eps = (lo + hi) / 2
    return best, trace


# ---------------------------------------------------------------------------------------------------------------------- cases
CLIP = (-2.5, 2.5)


def case_eps(B, seed):
    """Per row: 0, tiny (every neuron stable), large (most unstable), and one so large that the clip box cuts it."""
    base = np.array([0.0, 1e-4, 0.3, 4.0, 0.02, 0.1], np.float32)
    return np.resize(np.roll(base, seed), B).astype(np.float32)


def cases():
    """name -> (model, batch).  37 -> 33 -> 18 -> 5 has no multiple of 4, one width above 32 and a K that ends mid-tile."""
    return {
        "signed": (make_model([37, 33, 18, 5], 1, bn=(0, 1)), 3),
        "signed70": (make_model([37, 33, 18, 5], 2, bn=(0, 1)), 70),
        "nonneg": (make_model([37, 33, 18, 5], 3, bn=(0, 1), signed=False), 3),
        "nonneg1": (make_model([37, 33, 18, 5], 3, bn=(0, 1), signed=False), 1),
        "linear": (make_model([7, 3], 4), 3),
        "wide": (make_model([37, 1025, 5], 5, bn=(0,)), 3),
    }


def case_inputs(m, B, seed):
    rng = np.random.default_rng(100 + seed)
    x = np.clip(rng.standard_normal((B, m["widths"][0])), CLIP[0] + 0.1, CLIP[1] - 0.1).astype(np.float32)
    y = forward(m, x).argmax(-1).astype(np.int32)
    return x, case_eps(B, seed), y


def sample_points(m, xb, eb, norm, clip, y, rng, n=200):
    """n points of row's input set: the centre, random interior points, random corners, the projected-gradient corner per class."""
    xb = np.asarray(xb, np.float64)
    n0 = xb.size
    pts = [xb]
    for k in range(m["widths"][-1]):
        if k == y:
            continue
        g = margin_grad(m, xb, y, k)
        pts.append(xb - eb * (np.sign(g) if norm != 2 else g / max(np.linalg.norm(g), 1e-300)))
    while len(pts) < n:
        if norm == 2:
            v = rng.standard_normal(n0)
            v *= (eb if len(pts) % 2 else eb * rng.random()) / np.linalg.norm(v)
        elif len(pts) % 2:
            v = eb * rng.choice([-1.0, 1.0], n0)
        else:
            v = eb * rng.uniform(-1, 1, n0)
        pts.append(xb + v)
    p = np.clip(np.stack(pts), clip[0], clip[1])
    if norm == 2:  # clipping moves a point towards the box, never out of the ball around an x inside the box; rounding may
        d = p - xb
        nn = np.linalg.norm(d, axis=1, keepdims=True)
        p = xb + d * np.minimum(1.0, eb / np.maximum(nn, 1e-300)) * (1 - 1e-12)
    else:
        p = np.clip(p, xb - eb, xb + eb)
    return p
