"""The oracle of CROWN-IBP certified training: the interval forward pass and the backward relaxation of DESIGN.md ("Bound
propagation") restated in torch on the CPU and differentiated by autograd, so that nothing here shares a line with the
hand-derived sweep of csrc/bounds_crown_grad.hip.

    crown_loss_rows  per row logsumexp of u (u_k = -((1 - beta) margin_ibp_k + beta margin_crown_k), u_y = 0)
    loss_and_grads   that loss and d(sum_b loss_b) / d(W, b, gamma, beta), in float64 (the oracle) or float32 (the same graph)
    kinks            how far the float64 oracle is from every point where the loss is not differentiable, in the units the tests ask for
    tolerances       per parameter segment 8 times what the same graph loses in float32, floor 2^-22
    train            the float64 trainer of the functional test: plain, IBP or CROWN-IBP training of a model with BatchNorm

The widening bounds_ref.widen(K, S) of every pre-activation box is a detached constant, as in bounds_grad_ref.  torch's own
conventions are the ones the kernels follow: torch.where takes the first branch where its condition holds (p < 0: the upper line;
Lambda_0 > 0: lo), a comparison carries no gradient.
"""
from __future__ import annotations

import numpy as np
import torch

import bounds_grad_ref as G
import bounds_ref as R


def margins(t, x, eps, y, clip, dtype, keep=None, slack=None):
    """(margin_ibp, margin_crown) [B, C] from the leaves ``t``; the own class's entries are meaningless.  keep (a dict) receives the
    boxes, the widenings and every level's p, for the kink conditions."""
    L = len(t["W"])
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    et = torch.tensor(np.asarray(eps), dtype=dtype)[:, None]
    lo0 = torch.clamp(xt - et, min=clip[0])
    hi0 = torch.clamp(xt + et, max=clip[1])
    lo, hi = lo0, hi0
    boxes, aff = [], []
    for l in range(L - 1):
        W, b = t["W"][l], t["b"][l]
        c, r = (lo + hi) / 2, (hi - lo) / 2
        zc, rad = c @ W + b, r @ W.abs()
        with torch.no_grad():
            w = R.widen(W.shape[0], (c.abs() + r) @ W.abs() + b.abs())
        zlo, zhi = zc - rad - w, zc + rad + w
        boxes.append((zlo, zhi, w))
        if t["gamma"][l] is None:
            s, tt = torch.ones(W.shape[1], dtype=dtype), torch.zeros(W.shape[1], dtype=dtype)
        else:
            s = t["gamma"][l] / torch.sqrt(t["var"][l] + R.BN_EPS)
            tt = t["beta"][l] - s * t["mean"][l]
        aff.append((s, tt))
        a, bb = torch.relu(zlo), torch.relu(zhi)
        lo = torch.where(s >= 0, s * a + tt, s * bb + tt)
        hi = torch.where(s >= 0, s * bb + tt, s * a + tt)
    WL, bL = t["W"][-1], t["b"][-1]
    yt = torch.as_tensor(np.asarray(y), dtype=torch.long)
    lam = WL[:, yt].T[:, None, :] - WL.T[None, :, :]                    # [B, C, n_{L-1}]
    const = bL[yt][:, None] - bL[None, :]
    m_ibp = (torch.where(lam > 0, lo[:, None, :], hi[:, None, :]) * lam).sum(-1) + const
    ps = []
    for l in range(L - 2, -1, -1):
        zlo, zhi, _ = boxes[l]
        zlo, zhi = zlo[:, None, :], zhi[:, None, :]
        s, tt = aff[l]
        const = const + lam @ tt
        p = lam * s
        unstable = (zlo < 0) & (zhi > 0)
        upper = unstable & (p < 0)
        sig = zhi / torch.where(unstable, zhi - zlo, torch.ones_like(zhi))
        lower = (zhi >= -zlo).to(dtype)
        slope = torch.where(zhi <= 0, torch.zeros_like(sig), torch.where(zlo >= 0, torch.ones_like(sig), torch.where(p < 0, sig, lower)))
        slope = slope.expand_as(p)
        const = const + torch.where(upper, -p * sig * zlo, torch.zeros_like(p)).sum(-1)
        nu = p * slope
        const = const + nu @ t["b"][l]
        ps.append((l, p.detach(), unstable.expand_as(p)))
        lam = nu @ t["W"][l].T
    m_crown = (torch.where(lam > 0, lo0[:, None, :], hi0[:, None, :]) * lam).sum(-1) + const
    if slack is not None:
        m_crown = m_crown - torch.tensor(np.asarray(slack), dtype=dtype)
    if keep is not None:
        keep.update(boxes=[(a.detach(), b.detach(), w) for a, b, w in boxes], p=ps, lam0=lam.detach(), lo0=lo0, hi0=hi0)
    return m_ibp, m_crown


def crown_loss_rows(t, x, eps, y, beta, clip, dtype, keep=None, slack=None):
    m_ibp, m_crown = margins(t, x, eps, y, clip, dtype, keep, slack)
    mixed = (1 - beta) * m_ibp + beta * m_crown
    yt = torch.as_tensor(np.asarray(y), dtype=torch.long)
    own = torch.nn.functional.one_hot(yt, mixed.shape[1]).bool()
    return torch.logsumexp(torch.where(own, torch.zeros_like(mixed), -mixed), dim=1)


def loss_and_grads(m, x, eps, y, beta, clip=R.CLIP, dtype=torch.float64, slack=None):
    """(loss_rows [B], grads dict(dW, db, dgamma, dbeta: per layer, None where there is none)) as float64 NumPy."""
    t = G._tensors(m, dtype)
    rows = crown_loss_rows(t, x, eps, y, beta, clip, dtype, slack=slack)
    rows.sum().backward()
    g = lambda v: None if v is None else v.grad.detach().double().numpy()
    grads = {"dW": [g(v) for v in t["W"]], "db": [g(v) for v in t["b"]], "dgamma": [g(v) for v in t["gamma"]],
             "dbeta": [g(v) for v in t["beta"]]}
    return rows.detach().double().numpy(), grads


def tolerances(m, x, eps, y, beta, layout, clip=R.CLIP, factor=8.0, floor=2.0 ** -22, slack=None):
    """(float64 loss_rows, float64 flat gradient, {segment: bound}, {segment: float32 error})."""
    rows, g64 = loss_and_grads(m, x, eps, y, beta, clip, torch.float64, slack)
    _, g32 = loss_and_grads(m, x, eps, y, beta, clip, torch.float32, slack)
    want = G.flat(g64, m, layout)
    err32, _ = G.segment_errors(G.flat(g32, m, layout), want, m, layout)
    return rows, want, {k: max(factor * v, floor) for k, v in err32.items()}, err32


def kinks(m, x, eps, y, clip=R.CLIP):
    """dict of the smallest distances of the float64 oracle from a kink, each in the unit its condition names:
        gate    |z bound| / widening, over every pre-activation bound
        flip    |z_hi + z_lo| / widening, over every unstable neuron (the lower line's slope changes where z_hi = -z_lo)
        p       |p| / (8-free) fp32 drift of p, over every non-zero p of an unstable neuron
        lam0    |Lambda_0| / fp32 drift, over every non-zero Lambda_0[i] whose input box has lo < hi
    and ``drift`` [B, C], bounds_ref.crown's bound on what an fp32 run of the chain moves margin_crown by.  An exact zero is
    structural (the own class's row; a BatchNorm scale of 0) and follows the stated convention in any arithmetic."""
    keep = {}
    with torch.no_grad():
        margins(G._tensors(m, torch.float64), x, eps, y, clip, torch.float64, keep)
    out = {"gate": float("inf"), "flip": float("inf"), "p": float("inf"), "lam0": float("inf")}
    for zlo, zhi, w in keep["boxes"]:
        out["gate"] = min(out["gate"], float((torch.minimum(zlo.abs(), zhi.abs()) / w).min()))
        un = (zlo < 0) & (zhi > 0)
        if un.any():
            out["flip"] = min(out["flip"], float(((zhi + zlo).abs() / w)[un].min()))
    # the drifts of the coefficients, by the recursion of bounds_ref.crown restated per level
    B, C = len(y), m["widths"][-1]
    L = len(m["W"])
    drift = np.zeros((B, C))
    bx = R.ibp(m, np.asarray(x, np.float64), np.asarray(eps, np.float64), R.INF, clip)
    boxes64 = {"box": bx["box"], "z": [(a.numpy(), b.numpy()) for a, b, _ in keep["boxes"]]}
    for b in range(B):
        yb = int(y[b])
        drift[b] = R.crown(m, b, yb, boxes64, R.INF, np.asarray(x, np.float64), float(eps[b]))[1]
        WL = m["W"][-1].astype(np.float64)
        lam = (WL[:, [yb]] - WL).T
        dl = R.U * np.abs(lam)
        for l in range(L - 2, -1, -1):
            zlo, zhi = boxes64["z"][l][0][b], boxes64["z"][l][1][b]
            s, _ = R.affine(m, l)
            p = lam * s
            dp = dl * np.abs(s)
            un = np.broadcast_to((zlo < 0) & (zhi > 0), p.shape)
            sel = un & (p != 0)
            if sel.any():
                out["p"] = min(out["p"], float((np.abs(p)[sel] / dp[sel]).min()))
            sig = np.where((zlo < 0) & (zhi > 0), zhi / np.where(zhi - zlo > 0, zhi - zlo, 1.0), 0.0)
            slope = np.where(zhi <= 0, 0.0, np.where(zlo >= 0, 1.0, np.where(p < 0, sig, np.where(zhi >= -zlo, 1.0, 0.0))))
            nu = p * slope
            dnu = dp * np.where(un, 1.0, slope) * (1 + R.U) + 2 * R.U * np.abs(nu) + R.TINY
            W = m["W"][l].astype(np.float64)
            K = W.shape[1]
            lam = nu @ W.T
            dl = dnu @ np.abs(W).T + R.gamma(K + 1) * ((np.abs(nu) + dnu) @ np.abs(W).T) + (K + 1) * R.TINY
        open_box = np.broadcast_to(bx["box"][0][b] < bx["box"][1][b], lam.shape)
        sel = open_box & (lam != 0)
        if sel.any():
            out["lam0"] = min(out["lam0"], float((np.abs(lam)[sel] / dl[sel]).min()))
    out["drift"] = drift
    return out


# -------------------------------------------------------------------------------------------------------- the float64 trainer
def blobs(n, seed, classes=10, dim=20, noise=0.5):
    return G.blobs(n, seed, classes=classes, dim=dim, noise=noise)


def train(method, widths=(20, 64, 32, 10), seed=0, steps=400, batch=64, eps=0.4, kappa=1.0, warmup=50, ramp=200, lr=1e-3,
          beta=(1.0, 1.0), clip=(-2.5, 2.5), momentum=0.99):
    """bounds_grad_ref.train with the robust term of ``method`` in ("plain", "ibp", "crown-ibp") on blobs(); returns the model as a
    bounds_ref dict."""
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
        f = min(max((step - warmup) / ramp, 0.0), 1.0)
        eps_t, kappa_t = (eps * f, kappa * f) if method != "plain" else (0.0, 0.0)
        beta_t = beta[0] + (beta[1] - beta[0]) * f if method == "crown-ibp" else 0.0
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
            loss = loss + kappa_t * crown_loss_rows(t, x, np.full(batch, eps_t), y, beta_t, clip, dt).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    f32 = lambda v: v.detach().numpy().astype(np.float32)
    return {"widths": list(widths), "W": [f32(v) for v in t["W"]], "b": [f32(v) for v in t["b"]],
            "bn": [None if t["gamma"][l] is None else (f32(t["gamma"][l]), f32(t["beta"][l]), f32(t["mean"][l]), f32(t["var"][l]))
                   for l in range(L)]}


def accuracies(m, x, y, eps, clip=(-2.5, 2.5)):
    """(clean accuracy, accuracy certified by max(IBP, CROWN-IBP) at eps) of a bounds_ref model in float64."""
    right = R.forward(m, x).argmax(-1) == y
    mm = R.bound_margins(m, x, np.full(len(x), eps), R.INF, clip, y, method="crown-ibp").min(-1)
    return float(right.mean()), float(((mm > 0) & right).mean())
