"""float64 references of training for randomized smoothing (no test in here; imported by test_smooth_train_cpu / _gpu).

smooth_loss_ref: a NumPy restatement of lipasr_smooth_loss (include/lipasr.h), written from the definitions and not from the
kernel's text: softmaxes by scipy-free NumPy, Phi^-1 by statistics.NormalDist.  It also returns the two terms of dz separately
(the tests' element-wise bound is built from them) and how close every clip is to one of its decisions.

torch_grads: a float64 torch model of the dense classifier (Dense/ReLU -> BatchNorm(train) -> dropout masks) whose smoothed loss is
differentiated by autograd; Adam and the moving statistics are oracle.mlp_ref.train_step's.  train_cpu / acr_numpy: the functional
recipe of DESIGN.md, "Training for smoothing", on the CPU (plain, Gaussian and MACER).
"""
from statistics import NormalDist

import numpy as np

_ND = NormalDist()


def probit(q):
    q = float(q)
    if q <= 0.0:
        return -np.inf
    if q >= 1.0:
        return np.inf
    return _ND.inv_cdf(q)


def _softmax(z):
    d = z - z.max(axis=-1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(axis=-1, keepdims=True), d - np.log(e.sum(axis=-1, keepdims=True))


def _one_minus(p, c):
    """delta_cc - p_c as the sum of the other classes, per row of p [m, C] -> [m]"""
    return np.delete(p, c, axis=1).sum(axis=1)


def smooth_loss_ref(logits, label, draws, sigma, lam, gamma, beta, scale):
    """logits [clips * draws, classes] (float32 values), label [clips] -> dict of float64 arrays:
    dz, dz_c (the classification term), dz_r (the robust term, lam (sigma / 2) dxi/dz, unsigned by the minus) -- all already times
    scale --, loss, correct, radius, active, top_is_y (A == y) and margin: the distance of the clip to its nearest decision (a tie
    for argmax p^, for A or B, xi against gamma)."""
    f32 = lambda v: float(np.float32(v))
    sigma, lam, gamma, beta, scale = f32(sigma), f32(lam), f32(gamma), f32(beta), f32(scale)
    z = np.asarray(logits, dtype=np.float64)
    label = np.asarray(label).reshape(-1)
    clips, m = label.size, int(draws)
    C = z.shape[1]
    z = z.reshape(clips, m, C)
    out = {k: np.zeros((clips, m, C)) for k in ("dz", "dz_c", "dz_r")}
    out.update({k: np.zeros(clips) for k in ("loss", "correct", "radius", "active", "top_is_y")})
    out["margin"] = np.full(clips, np.inf)
    for b in range(clips):
        y = int(label[b])
        if not (0 <= y < C) or not np.isfinite(z[b]).all():
            for k in ("dz", "dz_c", "dz_r"):
                out[k][b] = np.nan
            out["loss"][b] = np.nan
            continue
        p, logp = _softmax(z[b])
        s, _ = _softmax(beta * z[b])
        phat, q = p.mean(axis=0), s.mean(axis=0)
        lp = logp[:, y]
        lw = lp.max() + np.log(np.exp(lp - lp.max()).sum())
        LC = np.log(m) - lw
        w = np.exp(lp - lw)
        delta_p = -p.copy()
        delta_p[:, y] = _one_minus(p, y)
        gc = -w[:, None] * delta_p
        srt = np.sort(phat)[::-1]
        margin = srt[0] - srt[1] if C > 1 else np.inf
        out["correct"][b] = float(int(np.argmax(phat)) == y)
        A = int(np.argmax(q))
        gr = np.zeros((m, C))
        LR = 0.0
        if C > 1:
            others = [c for c in range(C) if c != y]
            B = others[int(np.argmax(q[others]))]
            qs = np.sort(q)[::-1]
            margin = min(margin, qs[0] - qs[1])
            if C > 2:
                qo = np.sort(q[others])[::-1]
                margin = min(margin, qo[0] - qo[1])
            xi = probit(q[y]) - probit(q[B])
            if A == y:
                out["top_is_y"][b] = 1.0
                out["radius"][b] = 0.5 * sigma * xi if sigma > 0 else 0.0
                if np.isfinite(xi):
                    margin = min(margin, abs(xi - gamma))
            if lam > 0 and A == y and q[B] > 0 and q[y] < 1 and xi <= gamma:
                out["active"][b] = 1.0
                LR = 0.5 * sigma * (gamma - xi)
                a_y = np.sqrt(2 * np.pi) * np.exp(probit(q[y]) ** 2 / 2)
                a_B = np.sqrt(2 * np.pi) * np.exp(probit(q[B]) ** 2 / 2)
                dy, dB = -s.copy(), -s.copy()
                dy[:, y] = _one_minus(s, y)
                dB[:, B] = _one_minus(s, B)
                dxi = (beta / m) * (a_y * s[:, [y]] * dy - a_B * s[:, [B]] * dB)
                gr = lam * 0.5 * sigma * dxi
        else:
            out["top_is_y"][b] = 1.0
            out["radius"][b] = np.inf if sigma > 0 else 0.0
        out["loss"][b] = LC + lam * LR
        out["dz_c"][b], out["dz_r"][b], out["dz"][b] = scale * gc, scale * gr, scale * (gc - gr)
        out["margin"][b] = margin
    for k in ("dz", "dz_c", "dz_r"):
        out[k] = out[k].reshape(clips * m, C)
    return out


def loss_only(logits, label, draws, sigma, lam, gamma, beta):
    """sum over the clips of loss[b] in float64 from float64 logits (no float32 rounding of the logits): what central differences
    differentiate."""
    z = np.asarray(logits, dtype=np.float64)
    label = np.asarray(label).reshape(-1)
    clips, m, C = label.size, int(draws), z.shape[1]
    z = z.reshape(clips, m, C)
    total = 0.0
    for b in range(clips):
        y = int(label[b])
        p, logp = _softmax(z[b])
        s, _ = _softmax(beta * z[b])
        q = s.mean(axis=0)
        lp = logp[:, y]
        total += np.log(m) - (lp.max() + np.log(np.exp(lp - lp.max()).sum()))
        if C > 1 and lam > 0:
            others = [c for c in range(C) if c != y]
            B = others[int(np.argmax(q[others]))]
            xi = probit(q[y]) - probit(q[B])
            if int(np.argmax(q)) == y and q[B] > 0 and q[y] < 1 and xi <= gamma:
                total += lam * 0.5 * sigma * (gamma - xi)
    return total


# ------------------------------------------------------------------------------------------------ float64 torch trainer
def torch_logits(spec, tp, x, masks=None, eps=1e-3):
    """Training-mode forward of the dense classifier on torch tensors (tp: dict of lists W, b, gamma, beta): Dense -> ReLU ->
    BatchNorm with batch statistics -> dropout mask, as oracle.mlp_ref.forward_backward."""
    h = x
    for l, s in enumerate(spec):
        h = h @ tp["W"][l] + tp["b"][l]
        if l == len(spec) - 1:
            return h
        h = h.clamp_min(0)
        if s.bn:
            mean = h.mean(dim=0)
            var = ((h - mean) ** 2).mean(dim=0)
            h = (h - mean) / (var + eps).sqrt() * tp["gamma"][l] + tp["beta"][l]
        if masks is not None and masks[l] is not None:
            h = h * masks[l]


def torch_grads(spec, p, x, labels, draws, sigma, lam, gamma, beta, masks=None):
    """float64 autograd gradients of mean_b loss[b] (torch_smooth_loss) over the rows x [clips * draws, n] of oracle Params p ->
    (the dict dW, db, dgamma, dbeta that oracle.mlp_ref.train_step takes as grads_override, the per-clip losses)."""
    import torch

    t = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    tp = {"W": [t(a) for a in p.W], "b": [t(a) for a in p.b], "gamma": [t(a) for a in p.gamma], "beta": [t(a) for a in p.beta]}
    tm = None if masks is None else [None if k is None else torch.tensor(np.asarray(k, dtype=np.float64)) for k in masks]
    z = torch_logits(spec, tp, torch.tensor(np.asarray(x, dtype=np.float64)), tm)
    rows = torch_smooth_loss(z, torch.tensor(np.asarray(labels, dtype=np.int64)), draws, sigma, lam, gamma, beta)
    rows.mean().backward()
    g = lambda a: None if a is None else a.grad.numpy().copy()
    return ({"dW": [g(a) for a in tp["W"]], "db": [g(a) for a in tp["b"]], "dgamma": [g(a) for a in tp["gamma"]],
             "dbeta": [g(a) for a in tp["beta"]]}, rows.detach().numpy())


# ------------------------------------------------------------------------------------------------ the functional recipe
BLOB_SPEC = ((20, 32, True), (32, 16, True), (16, 4, False))  # (n_in, n_out, BatchNorm) per layer
BLOB = dict(sigma=0.5, draws=16, lam=12.0, gamma=8.0, beta=16.0, warmup=50, steps=300, batch=64, n0=100, n=2000, alpha=0.001, rows=256,
            spread=0.4)


def blobs(n, seed, spread=BLOB["spread"], noise=0.5):
    """n rows of 4 Gaussian blobs in 20 dimensions (centres: fixed draws of N(0, spread^2 I), rows: centre + N(0, noise^2 I))."""
    centres = np.random.default_rng(12345).standard_normal((4, 20)) * spread
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 4, n)
    return (centres[y] + noise * rng.standard_normal((n, 20))).astype(np.float32), y


def blob_spec():
    from oracle import mlp_ref as P

    return [P.LayerSpec(a, b, bn, 0.0, False) for a, b, bn in BLOB_SPEC]


def train_cpu(method, seed, spread=BLOB["spread"], cfg=BLOB):
    """The recipe on the CPU in float64: ``method`` plain, gaussian or macer; Adam and the moving statistics through
    oracle.mlp_ref.train_step, NumPy noise.  Returns the trained oracle Params."""
    from oracle import mlp_ref as P

    spec = blob_spec()
    p = P.init_params(spec, seed=seed, dtype=np.float64)
    st = P.AdamState()
    rng = np.random.default_rng(1000 + seed)
    m = 1 if method == "plain" else cfg["draws"]
    sigma = 0.0 if method == "plain" else cfg["sigma"]
    for step in range(cfg["steps"]):
        x, y = blobs(cfg["batch"], 10_000 * (seed + 1) + step, spread)
        xn = np.repeat(x.astype(np.float64), m, axis=0) + sigma * rng.standard_normal((cfg["batch"] * m, 20))
        yn = np.repeat(y, m)
        if method == "macer":
            lam = 0.0 if step < cfg["warmup"] else cfg["lam"]
            grads, _ = torch_grads(spec, p, xn, y, m, sigma, lam, cfg["gamma"], cfg["beta"])
            P.train_step(spec, p, st, xn, P.to_categorical(yn, 4).astype(np.float64), grads_override=grads)
        else:
            P.train_step(spec, p, st, xn, P.to_categorical(yn, 4).astype(np.float64))
    return p


def acr_numpy(p, x, y, seed, cfg=BLOB):
    """The average certified radius of oracle Params p over rows x with NumPy draws: Cohen's CERTIFY per row (lipasr.smoothing's
    host statistics), wrong or abstaining rows counted as 0."""
    from lipasr.smoothing import _PHI_INV, cp_lower
    from oracle import mlp_ref as P

    spec = blob_spec()
    rng = np.random.default_rng(seed)
    total = 0.0
    for xb, yb in zip(np.asarray(x, dtype=np.float64), y):
        sel = P.forward_infer(spec, p, xb + cfg["sigma"] * rng.standard_normal((cfg["n0"], 20)), return_logits=True).argmax(axis=1)
        ca = int(np.bincount(sel, minlength=4).argmax())
        est = P.forward_infer(spec, p, xb + cfg["sigma"] * rng.standard_normal((cfg["n"], 20)), return_logits=True).argmax(axis=1)
        pl = cp_lower(int((est == ca).sum()), cfg["n"], cfg["alpha"])
        if pl > 0.5 and ca == int(yb):
            total += cfg["sigma"] * _PHI_INV(pl)
    return total / len(y)


def torch_smooth_loss(logits, label, draws, sigma, lam, gamma, beta):
    """The per-clip losses of lipasr_smooth_loss as a differentiable torch expression (float64 logits [clips * draws, C], label a
    LongTensor [clips]) -> [clips]."""
    import torch

    clips, m, C = label.numel(), int(draws), logits.shape[1]
    z = logits.reshape(clips, m, C)
    logp = torch.log_softmax(z, dim=2)
    idx = label.view(clips, 1, 1).expand(clips, m, 1)
    lp = logp.gather(2, idx).squeeze(2)
    loss = np.log(m) - torch.logsumexp(lp, dim=1)
    if lam > 0 and C > 1:
        nd = torch.distributions.Normal(torch.zeros((), dtype=z.dtype), torch.ones((), dtype=z.dtype))
        q = torch.softmax(beta * z, dim=2).mean(dim=1)
        qy = q.gather(1, label.view(-1, 1)).squeeze(1)
        qo = q.scatter(1, label.view(-1, 1), -1.0)
        qB, _ = qo.max(dim=1)
        top = q.argmax(dim=1) == label
        ok = top & (qB > 0) & (qy < 1)
        # (rows that are not ok get harmless arguments: the derivative of icdf at 0 or 1 is inf, and inf * 0 would reach the weights)
        xi = nd.icdf(torch.where(ok, qy, torch.full_like(qy, 0.6))) - nd.icdf(torch.where(ok, qB, torch.full_like(qB, 0.4)))
        act = ok & (xi <= gamma)
        loss = loss + torch.where(act, lam * 0.5 * sigma * (gamma - xi), torch.zeros_like(xi))
    return loss
