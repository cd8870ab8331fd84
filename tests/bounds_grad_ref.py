"""The oracle of IBP certified training: the interval forward pass of tests/bounds_ref.py restated in torch on the CPU and
differentiated by autograd, so that nothing here shares a line with the hand-derived backward pass of csrc/bounds_grad.hip.

    loss_and_grads   per row logsumexp of u (u_k = -margin_ibp_k, u_y = 0) and d(sum_b loss_b) / d(W, b, gamma, beta), in float64
                     (the oracle) or float32 (the same graph: what fp32 arithmetic alone loses, which sets the tests' tolerance)
    gate_distance    how many widenings the float64 pre-activation bound closest to 0 is away from 0
    flat / segments  the gradients in lipasr_mlp_create's flat layout, and that layout's segments by name
    train            the float64 trainer of the functional test: plain or IBP training of a model with BatchNorm

The widening bounds_ref.widen(K, S) of every pre-activation box is added as a detached constant, as DESIGN.md ("Certified
training") says the device treats it.  torch's own conventions are the ones the kernels follow: relu'(0) = 0, d|w|/dw = 0 at 0,
torch.where takes the first branch where its condition holds (s >= 0; a difference row > 0).
"""
from __future__ import annotations

import numpy as np
import torch

import bounds_ref as R


def _tensors(m, dtype):
    """Leaves: W, b per layer and gamma, beta per BatchNorm layer; the running statistics as constants."""
    t = {"W": [], "b": [], "gamma": [], "beta": [], "mean": [], "var": []}
    for l in range(len(m["W"])):
        t["W"].append(torch.tensor(m["W"][l], dtype=dtype, requires_grad=True))
        t["b"].append(torch.tensor(m["b"][l], dtype=dtype, requires_grad=True))
        if m["bn"][l] is None:
            for k in ("gamma", "beta", "mean", "var"):
                t[k].append(None)
        else:
            g, be, mean, var = m["bn"][l]
            t["gamma"].append(torch.tensor(g, dtype=dtype, requires_grad=True))
            t["beta"].append(torch.tensor(be, dtype=dtype, requires_grad=True))
            t["mean"].append(torch.tensor(mean, dtype=dtype))
            t["var"].append(torch.tensor(var, dtype=dtype))
    return t


def ibp_loss_rows(t, x, eps, y, clip, dtype, boxes=None):
    """[B] robust cross-entropy per row from the leaves ``t``; boxes (a list) receives (z_lo, z_hi, widening) per hidden layer."""
    L = len(t["W"])
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    et = torch.tensor(np.asarray(eps), dtype=dtype)[:, None]
    lo = torch.clamp(xt - et, min=clip[0])
    hi = torch.clamp(xt + et, max=clip[1])
    for l in range(L - 1):
        W, b = t["W"][l], t["b"][l]
        K = W.shape[0]
        c, r = (lo + hi) / 2, (hi - lo) / 2
        zc, rad = c @ W + b, r @ W.abs()
        with torch.no_grad():
            w = R.widen(K, (c.abs() + r) @ W.abs() + b.abs())
        zlo, zhi = zc - rad - w, zc + rad + w
        if boxes is not None:
            boxes.append((zlo.detach(), zhi.detach(), w))
        a, bb = torch.relu(zlo), torch.relu(zhi)
        if t["gamma"][l] is None:
            lo, hi = a, bb
        else:
            s = t["gamma"][l] / torch.sqrt(t["var"][l] + R.BN_EPS)
            tt = t["beta"][l] - s * t["mean"][l]
            lo = torch.where(s >= 0, s * a + tt, s * bb + tt)
            hi = torch.where(s >= 0, s * bb + tt, s * a + tt)
    WL, bL = t["W"][-1], t["b"][-1]
    yt = torch.as_tensor(np.asarray(y), dtype=torch.long)
    d = WL[:, yt].T[:, None, :] - WL.T[None, :, :]                    # [B, C, n]: W_L[j][y_b] - W_L[j][k]
    margin = (torch.where(d > 0, lo[:, None, :], hi[:, None, :]) * d).sum(-1) + bL[yt][:, None] - bL[None, :]
    own = torch.nn.functional.one_hot(yt, WL.shape[1]).bool()
    u = torch.where(own, torch.zeros_like(margin), -margin)
    return torch.logsumexp(u, dim=1)


def loss_and_grads(m, x, eps, y, clip=R.CLIP, dtype=torch.float64):
    """(loss_rows [B], grads dict(dW, db, dgamma, dbeta: per layer, None where there is none)) as float64 NumPy."""
    t = _tensors(m, dtype)
    rows = ibp_loss_rows(t, x, eps, y, clip, dtype)
    rows.sum().backward()
    g = lambda v: None if v is None else v.grad.detach().double().numpy()
    grads = {"dW": [g(v) for v in t["W"]], "db": [g(v) for v in t["b"]], "dgamma": [g(v) for v in t["gamma"]],
             "dbeta": [g(v) for v in t["beta"]]}
    return rows.detach().double().numpy(), grads


def gate_distance(m, x, eps, y, clip=R.CLIP):
    """min over every float64 pre-activation bound of |bound| / widening (inf for a model without hidden layers): the smaller of
    the oracle's own boxes, which carry the widening, and the boxes of bounds_ref.ibp, which do not."""
    boxes = []
    with torch.no_grad():
        ibp_loss_rows(_tensors(m, torch.float64), x, eps, y, clip, torch.float64, boxes)
    best = min([float(torch.minimum(zlo.abs(), zhi.abs()).div(w).min()) for zlo, zhi, w in boxes], default=float("inf"))
    bx = R.ibp(m, np.asarray(x, np.float64), np.asarray(eps, np.float64), R.INF, clip)
    lo, hi = bx["box"]
    for l in range(len(m["W"]) - 1):
        zlo, zhi, S = R.ibp_layer(m, l, lo, hi)
        best = min(best, float((np.minimum(np.abs(zlo), np.abs(zhi)) / R.widen(m["W"][l].shape[0], S)).min()))
        lo, hi = bx["h"][l]
    return best


SEGMENTS = (("W", "dW"), ("b", "db"), ("gamma", "dgamma"), ("beta", "dbeta"))


def segments(m, layout):
    """[(name, offset, count)] of the trainable segments in the flat layout ``layout`` = lipasr._native.bounds_layout(...)."""
    out = []
    for l, d in enumerate(layout[0]):
        for key, _ in SEGMENTS:
            if key in d:
                n = m["W"][l].size if key == "W" else m["widths"][l + 1]
                out.append((f"{key}{l}", d[key], n))
    return out


def flat(grads, m, layout):
    """The gradient dict in the flat layout (float64; pad floats 0)."""
    out = np.zeros(layout[1])
    for l, d in enumerate(layout[0]):
        for key, gk in SEGMENTS:
            if key in d:
                v = grads[gk][l].reshape(-1)
                out[d[key]:d[key] + v.size] = v
    return out


def segment_errors(got, want, m, layout):
    """{segment: max |got - want| / max |want|} per parameter segment, and the pad floats' largest magnitude."""
    err, used = {}, np.zeros(layout[1], bool)
    for name, o, n in segments(m, layout):
        scale = np.abs(want[o:o + n]).max()
        err[name] = float(np.abs(np.asarray(got[o:o + n], np.float64) - want[o:o + n]).max() / scale) if scale > 0 else \
            float(np.abs(got[o:o + n]).max())
        used[o:o + n] = True
    pads = float(np.abs(np.asarray(got)[~used]).max()) if (~used).any() else 0.0
    return err, pads


def tolerances(m, x, eps, y, layout, clip=R.CLIP, factor=8.0, floor=2.0 ** -22):
    """(float64 loss_rows, float64 flat gradient, {segment: bound}): per segment ``factor`` times what the same graph loses in
    float32, not below ``floor``, in units of the segment's largest |float64 gradient|."""
    rows, g64 = loss_and_grads(m, x, eps, y, clip, torch.float64)
    _, g32 = loss_and_grads(m, x, eps, y, clip, torch.float32)
    want = flat(g64, m, layout)
    err32, _ = segment_errors(flat(g32, m, layout), want, m, layout)
    return rows, want, {k: max(factor * v, floor) for k, v in err32.items()}, err32


# -------------------------------------------------------------------------------------------------------- the float64 trainer
def blobs(n, seed, classes=4, dim=20, noise=0.35, clamp=2.5):
    """The functional test's data: ``classes`` Gaussian blobs whose means are drawn N(0, 1) from seed 0 of the recipe (the means do
    not depend on ``seed``, the rows do)."""
    means = np.random.default_rng(1000).standard_normal((classes, dim))
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    x = np.clip(means[y] + noise * rng.standard_normal((n, dim)), -clamp, clamp)
    return x.astype(np.float32), y.astype(np.int32)


def schedule(step, eps, kappa, warmup, ramp):
    f = min(max((step - warmup) / ramp, 0.0), 1.0)
    return eps * f, kappa * f


def train(widths=(20, 32, 16, 4), seed=0, steps=300, batch=64, eps=0.2, kappa=0.5, warmup=50, ramp=150, lr=1e-3, certified=True,
          clip=(-2.5, 2.5), momentum=0.99):
    """Adam training in float64 of widths with BatchNorm after every hidden ReLU, as lipasr.keras.Model.train_on_batch runs it: the
    plain cross-entropy in training mode (batch statistics, which also move the running ones), then -- certified -- the robust
    cross-entropy of the interval bounds in inference form on the running statistics the forward pass just updated.
    Returns the model as a bounds_ref dict."""
    dt = torch.float64
    gen = torch.Generator().manual_seed(seed)
    L = len(widths) - 1
    t = {"W": [], "b": [], "gamma": [], "beta": [], "mean": [], "var": []}
    for l in range(L):
        lim = np.sqrt(6.0 / (widths[l] + widths[l + 1]))
        t["W"].append(((torch.rand(widths[l], widths[l + 1], generator=gen, dtype=dt) * 2 - 1) * lim).requires_grad_())
        t["b"].append(torch.zeros(widths[l + 1], dtype=dt, requires_grad=True))
        bn = l + 1 < L
        t["gamma"].append(torch.ones(widths[l + 1], dtype=dt, requires_grad=True) if bn else None)
        t["beta"].append(torch.zeros(widths[l + 1], dtype=dt, requires_grad=True) if bn else None)
        t["mean"].append(torch.zeros(widths[l + 1], dtype=dt) if bn else None)
        t["var"].append(torch.ones(widths[l + 1], dtype=dt) if bn else None)
    leaves = [v for k in ("W", "b", "gamma", "beta") for v in t[k] if v is not None]
    opt = torch.optim.Adam(leaves, lr=lr, eps=1e-7)
    for step in range(steps):
        x, y = blobs(batch, 10_000 + 7919 * seed + step)
        eps_t, kappa_t = schedule(step, eps, kappa, warmup, ramp) if certified else (0.0, 0.0)
        h = torch.tensor(x, dtype=dt)
        for l in range(L - 1):
            a = torch.relu(h @ t["W"][l] + t["b"][l])
            mu, var = a.mean(0), a.var(0, unbiased=False)
            h = (a - mu) / torch.sqrt(var + R.BN_EPS) * t["gamma"][l] + t["beta"][l]
            with torch.no_grad():
                t["mean"][l] = t["mean"][l] * momentum + mu * (1 - momentum)
                t["var"][l] = t["var"][l] * momentum + var * (1 - momentum)
        logits = h @ t["W"][-1] + t["b"][-1]
        loss = (1 - kappa_t) * torch.nn.functional.cross_entropy(logits, torch.as_tensor(y, dtype=torch.long))
        if kappa_t > 0:
            loss = loss + kappa_t * ibp_loss_rows(t, x, np.full(batch, eps_t), y, clip, dt).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    f32 = lambda v: v.detach().numpy().astype(np.float32)
    return {"widths": list(widths), "W": [f32(v) for v in t["W"]], "b": [f32(v) for v in t["b"]],
            "bn": [None if t["gamma"][l] is None else (f32(t["gamma"][l]), f32(t["beta"][l]), f32(t["mean"][l]), f32(t["var"][l]))
                   for l in range(L)]}


def certified_accuracy(m, x, y, eps, clip=(-2.5, 2.5)):
    """(clean accuracy, IBP-certified accuracy at eps) of a bounds_ref model in float64."""
    right = R.forward(m, x).argmax(-1) == y
    mm = R.bound_margins(m, x, np.full(len(x), eps), R.INF, clip, y, method="ibp").min(-1)
    return float(right.mean()), float(((mm > 0) & right).mean())
