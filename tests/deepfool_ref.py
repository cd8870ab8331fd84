"""Oracle of DeepFool (lipasr_deepfool_step, lipasr.attacks.DeepFool, get_lipschitz_bound / get_robustness_radius): the conventions
of include/lipasr.h written out in NumPy.  TEST INFRASTRUCTURE for tests/test_deepfool_*: nothing here is used by the library.

    step            one iteration on one batch, float64: the definition the device kernel is held to
    art_step        the same iteration as ART's art.attacks.evasion.DeepFool writes it (its batched array expressions, restated from
                    the published implementation), for overshoot = 0
    step_lane_f64   the kernel's summation restated on the host: the differences and their squares in float64, 256 lane-serial
                    partial sums (lane l takes columns l, l + 256, ...; with 16-byte loads the four columns 4 l .. 4 l + 3), the
                    64 lanes of a wave by a butterfly, the four waves in order
    deepfool        the whole attack on the oracle classifier (oracle.mlp_ref), in the dtype of its parameters
    audio_graph     one row of audio -> (J [C, n], logits [C]) through tests/mfcc_grad_ref.features_22k and the classifier, in one dtype
    lipschitz_bound prod ||W_l||_2 x prod_BN max_j |gamma_j| / sqrt(var_j + 1e-3) on the host, float64
"""
from __future__ import annotations

import numpy as np

from oracle import mlp_ref as P

TOL = 1e-7  # ART's tol = 10e-8


def _lowest_argmax(row):
    return int(np.flatnonzero(row == row.max())[0])


def step(J, out, label, x, norm=2, overshoot=0.02, lo=-np.inf, hi=np.inf, allowed=None, sums=None):
    """J [B, C, n], out [B, C], label [B], x [B, n] -> (x_new float64 [B, n], r [B, n], dist [B], target [B], state [B]).  r is the
    step before the overshoot and the clipping (zeros where no step is taken).  ``sums(w) -> (||w||_1, ||w||_2^2)`` replaces
    the float64 sums (step_lane_f64)."""
    J, out, x = (np.asarray(a, dtype=np.float64) for a in (J, out, x))
    B, C, n = J.shape
    x_new, r = x.copy(), np.zeros_like(x)
    dist, target, state = np.full(B, np.nan), np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)
    for b in range(B):
        c = int(label[b])
        if not np.isfinite(out[b]).all() or not 0 <= c < C:
            continue
        am = _lowest_argmax(out[b])
        if am != c:
            dist[b], target[b], state[b] = 0.0, am, 0
            continue
        best, l, s_l = np.inf, -1, 0.0
        for k in range(C):
            if k == c or (allowed is not None and not (int(allowed[b]) >> k) & 1):
                continue
            w = J[b, k] - J[b, c]
            with np.errstate(all="ignore"):
                s1, s2 = (np.abs(w).sum(), (w * w).sum()) if sums is None else sums(w)
            s = s2 if norm == 2 else s1
            if not np.isfinite(s):
                continue
            rho = abs(out[b, k] - out[b, c]) / ((np.sqrt(s) if norm == 2 else s) + TOL)
            if rho < best:
                best, l, s_l = rho, k, s
        if l < 0:
            continue
        w = J[b, l] - J[b, c]
        f = abs(out[b, l] - out[b, c])
        r[b] = f / (s_l + TOL) * (w if norm == 2 else np.sign(w))
        moved = np.where(r[b] == 0, x[b], x[b] + (1.0 + float(np.float32(overshoot))) * r[b])
        x_new[b] = np.clip(moved, lo, hi)
        dist[b], target[b], state[b] = best, l, 1
    return x_new, r, dist, target, state


def art_step(grd, f_batch, fk_hat, batch):
    """One pass of the while loop of ART's DeepFool._generate (norm 2, every class a candidate, no clip_values): the arrays keep
    ART's names.  -> the new batch and l_var."""
    tol = 10e-8
    rows = np.arange(len(grd))
    grad_diff = grd - grd[rows, fk_hat][:, None]
    f_diff = f_batch - f_batch[rows, fk_hat][:, None]
    norm = np.linalg.norm(grad_diff.reshape(len(grd), grd.shape[1], -1), axis=2) + tol
    value = np.abs(f_diff) / norm
    value[rows, fk_hat] = np.inf
    l_var = np.argmin(value, axis=1)
    absolute1 = abs(f_diff[rows, l_var])
    draddiff = grad_diff[rows, l_var].reshape(len(grd), -1)
    pow1 = pow(np.linalg.norm(draddiff, axis=1), 2) + tol
    r_var = absolute1 / pow1
    r_var = r_var.reshape((-1,) + (1,) * (len(batch.shape) - 1)) * grad_diff[rows, l_var]
    return batch + r_var, l_var


def lane_sums_f64(w, vec=1, lanes=256):
    """(sum |w|, sum w^2) of a float64 vector the way the kernel adds them: lane-serial, a butterfly over the 64 lanes of each
    wave, the waves in order."""
    w = np.asarray(w, dtype=np.float64)
    n = w.shape[0]
    nv = n // vec
    p1, p2 = np.zeros(lanes), np.zeros(lanes)
    for i0 in range(0, nv, lanes):
        for e in range(vec):
            col = w[i0 * vec + e:min(nv, i0 + lanes) * vec:vec]
            p1[:col.shape[0]] += np.abs(col)
            p2[:col.shape[0]] += col * col
    res = []
    for p in (p1, p2):
        t = p.reshape(lanes // 64, 64)
        o = 32
        while o:
            t = t + t[:, np.arange(64) ^ o]
            o >>= 1
        tot = t[0, 0]
        for wv in range(1, lanes // 64):
            tot = tot + t[wv, 0]
        res.append(tot)
    return res[0], res[1]


def step_lane_f64(J, out, label, x, vec=1, **kw):
    return step(J, out, label, x, sums=lambda w: lane_sums_f64(w, vec), **kw)


def jacobian(spec, p, x, on_logits):
    """[B, n] -> (J [B, C, n], out [B, C]) in the dtype of ``x`` and ``p``: every class gradient and the function they differentiate."""
    C = spec[-1].n_out
    J = np.zeros((x.shape[0], C, x.shape[1]), dtype=x.dtype)
    for c in range(C):
        v = np.zeros((x.shape[0], C), dtype=x.dtype)
        v[:, c] = 1
        J[:, c] = P.output_vjp_infer(spec, p, x, v, on_logits=on_logits)[0]
    return J, P.forward_infer(spec, p, x, return_logits=bool(on_logits))


def top_mask(out, nb_grads):
    """bit k set for the nb_grads largest outputs of each row (lowest index first among equals)."""
    order = np.argsort(-np.asarray(out, dtype=np.float64), axis=1, kind="stable")[:, :nb_grads]
    return np.array([sum(1 << int(k) for k in row) for row in order], dtype=np.uint64)


def deepfool(spec, p, x, norm=2, overshoot=0.02, on_logits=True, max_iter=100, epsilon=1e-6, nb_grads=None, dtype=np.float64):
    """lipasr.attacks.DeepFool on the oracle classifier, every array in ``dtype`` -> dict(x_adv, iterations, flipped, target,
    first_dist, label)."""
    p = p.astype(dtype)
    x0 = np.asarray(x, dtype=dtype)
    out0 = P.forward_infer(spec, p, x0, return_logits=bool(on_logits))
    label = np.array([_lowest_argmax(r) for r in out0])
    C = spec[-1].n_out
    allowed = None if nb_grads is None or nb_grads >= C else top_mask(out0, nb_grads)
    xa = x0.copy()
    B = x0.shape[0]
    iters, first, target = np.zeros(B, dtype=np.int64), np.full(B, np.nan), np.full(B, -1, dtype=np.int64)
    for it in range(max_iter):
        J, out = jacobian(spec, p, xa, on_logits)
        x_new, _, dist, tgt, state = step(J, out, label, xa, norm=norm, overshoot=overshoot, allowed=allowed)
        xa = x_new.astype(dtype)
        iters += state == 1
        if it == 0:
            first = dist.copy()
        target = np.where(state == 1, tgt, target)
        if not (state == 1).any():
            break
    adv = xa if epsilon == 0 else np.where(xa == x0, x0, x0 + dtype(1.0 + epsilon) * (xa - x0)).astype(dtype)
    final = P.forward_infer(spec, p, adv, return_logits=True)
    flipped = np.array([_lowest_argmax(r) for r in final]) != label
    return dict(x_adv=adv, iterations=iters, flipped=flipped, target=target, first_dist=first, label=label)


def lipschitz_bound(spec, p):
    """The true product bound of the logits' Lipschitz constant (2-norm), float64."""
    bound = 1.0
    for l, s in enumerate(spec):
        bound *= np.linalg.norm(np.asarray(p.W[l], dtype=np.float64), 2)
        if s.bn and l < len(spec) - 1:
            g, v = np.asarray(p.gamma[l], dtype=np.float64), np.asarray(p.mov_var[l], dtype=np.float64)
            bound *= np.max(np.abs(g) / np.sqrt(v + P.BN_EPS))
    return float(bound)


def margin(logits, label):
    """min over k != c of z_c - z_k, float64 [B]."""
    z = np.asarray(logits, dtype=np.float64)
    out = np.zeros(z.shape[0])
    for b in range(z.shape[0]):
        c = int(label[b])
        out[b] = (z[b, c] - np.delete(z[b], c)).min()
    return out


def distance(d, norm):
    d = np.asarray(d, dtype=np.float64)
    return np.sqrt((d * d).sum(axis=1)) if norm == 2 else np.abs(d).max(axis=1)


def audio_graph(spec, p, x, mean, scale, dtype=None, n_clip=None, **feat_kw):
    """local_lip_ref.audio_jacobian together with the logits it differentiates: one row of audio ``x`` [n] -> (J [C, n], z [C]),
    float64 arrays holding what the graph gives when it is evaluated in ``dtype`` (torch.float64 by default)."""
    import torch

    import local_lip_ref as R
    import mfcc_grad_ref as G

    dtype = torch.float64 if dtype is None else dtype
    x = np.asarray(x, dtype=np.float64)
    n_clip = x.shape[0] if n_clip is None else int(n_clip)
    xt = torch.as_tensor(x[:n_clip]).to(dtype).requires_grad_(True)
    feat_kw = dict(feat_kw)
    sr_in, domain = feat_kw.pop("sr_in", 16000), feat_kw.pop("domain", "input")
    y = xt if domain == "22k" else R.resample(xt, sr_in, dtype)
    f = G.features_22k(y, mean=mean, scale=scale, dtype=dtype, **feat_kw)
    z = R.torch_logits(spec, R.torch_params(p, dtype), f[None, :])[0]
    J = np.zeros((z.shape[0], x.shape[0]))
    for c in range(z.shape[0]):
        (g,) = torch.autograd.grad(z[c], xt, retain_graph=True)
        J[c, :n_clip] = g.detach().to(torch.float64).numpy()
    return J, z.detach().to(torch.float64).numpy()
