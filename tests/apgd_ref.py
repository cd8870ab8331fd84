"""Oracle of Auto-PGD (lipasr_apgd_loss, lipasr_apgd_step, lipasr.attacks.AutoProjectedGradientDescent): a NumPy restatement in
float64.  TEST INFRASTRUCTURE for tests/test_apgd_*: nothing here is used by the library.

    checkpoints  the schedule by the integer rule of the issue, written a second time (a loop over hundredths)
    loss         the objective to maximise, its gradient at the logits, hit, and the indices chosen (include/lipasr.h, lipasr_apgd_loss)
    step         one iteration given explicit state (lipasr_apgd_step): float64 arithmetic on the float32 inputs; the state as the
                 kernel holds it (float32 / int32), and which rows copied into x_best / g_best / x_adv
    attack       the whole attack on an oracle.mlp_ref model, iterates stored as float32 between iterations; every float comparison a
                 row's run makes is recorded as (a, b), so that a test can see how close to a tie a decision was
"""
from __future__ import annotations

import numpy as np

from oracle import mlp_ref as P

TOL = 1e-7
DLR_TOL = 1e-12
AMBIGUITY = 1e-4  # relative: the issue's definition of an ambiguous comparison
STATE = ("eta", "f_best", "f_prev", "f_best_ckpt", "improved", "reduced_last", "fooled", "halvings")


def checkpoints(max_iter):
    p, out = [0, 22], []
    while p[-1] + max(p[-1] - p[-2] - 3, 6) <= 100:
        p.append(p[-1] + max(p[-1] - p[-2] - 3, 6))
    for q in p:
        w = (q * max_iter + 99) // 100
        if 1 <= w <= max_iter - 1 and w not in out:
            out.append(w)
    return sorted(out)


def loss(z, labels, loss_type=0, targeted=False):
    """float32 logits [B, C], labels int [B] -> dict: f float64 [B] (NaN on a bad row), dz float64 [B, C], hit int [B], bad bool [B],
    top int [B, 3] (pi1, pi2, pi3; -1 where there is none), other int [B] (o; -1 for cross-entropy), gaps: per row the list of
    (a, b) pairs whose order decided an index."""
    z32 = np.asarray(z, dtype=np.float32)
    z = z32.astype(np.float64)
    B, C = z.shape
    labels = np.asarray(labels, dtype=np.int64)
    f, dz, hit = np.full(B, np.nan), np.zeros((B, C)), np.zeros(B, dtype=np.int64)
    bad = ~np.isfinite(z).all(axis=1) | (labels < 0) | (labels >= C)
    top, other = np.full((B, 3), -1, dtype=np.int64), np.full(B, -1, dtype=np.int64)
    gaps = [[] for _ in range(B)]
    for b in range(B):
        if bad[b]:
            continue
        r, y = z[b], int(labels[b])
        order = sorted(range(C), key=lambda c: (-r[c], c))  # descending, the lowest index first on ties
        p1 = order[0]
        top[b, :min(3, C)] = order[:3]
        hit[b] = int(p1 == y) if targeted else int(p1 != y)
        if C > 1:
            gaps[b].append((r[order[0]], r[order[1]]))
        if loss_type == 0:
            m = r[p1]
            s1 = sum(np.exp(r[c] - m) for c in range(C) if c != p1)
            fv = (m - r[y]) + np.log1p(s1)
            inv = 1.0 / (1.0 + s1)
            others = sum(np.exp(r[c] - m) * inv for c in range(C) if c != y)
            sg = -1.0 if targeted else 1.0
            for c in range(C):
                dz[b, c] = sg * (-others if c == y else np.exp(r[c] - m) * inv)
            f[b] = sg * fv
            continue
        p2, p3 = order[1], order[2]
        gaps[b].append((r[p2], r[p3]))
        if C > 3:
            gaps[b].append((r[p3], r[order[3]]))
        o = p1 if p1 != y else p2
        other[b] = o
        D, N = (r[p1] - r[p3]) + DLR_TOL, r[y] - r[o]
        iD, q = 1.0 / D, N / (D * D)
        dz[b, y] -= iD
        dz[b, o] += iD
        dz[b, p1] += q
        dz[b, p3] -= q
        f[b] = -N / D
    return dict(f=f, dz=dz, hit=hit, bad=bad, top=top, other=other, gaps=gaps)


def _project(v, c, eps, lo, hi, l2, inside):
    u = np.clip(v, lo, hi)
    dl = u - c
    if not l2:
        return c + np.clip(dl, -eps, eps)
    nrm = np.sqrt((np.where(inside, dl, 0.0) ** 2).sum(axis=1, keepdims=True))
    return c + dl * np.minimum(1.0, eps / (nrm + TOL))


def step(x, x_prev, x0, g, x_best, g_best, x_adv, f, hit, state, norm, eps, eta0, clip=None, momentum=0.75, rho=0.75, first=False,
         last=False, ckpt_len=0, n_valid=None, record=None):
    """One lipasr_apgd_step.  Row arrays float32 [rows, n] (inputs are not modified), f float32 [rows], hit int [rows], state: dict of
    STATE arrays (ignored with first).  -> dict: x, x_prev float64 [rows, n] (None where the kernel writes nothing: last);
    x_best, g_best, x_adv float32 [rows, n] as the kernel leaves them; state (float32 / int32); upd_best, hit, restart, moved bool
    [rows] (moved: the row took step 4).  record: a list per row that receives the (a, b) of every float comparison."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    x, x_prev, x0, g, x_best, g_best, x_adv = (f32(a).copy() for a in (x, x_prev, x0, g, x_best, g_best, x_adv))
    rows, n = x.shape
    fr = f32(f)
    hit = np.asarray(hit) != 0
    nv = np.full(rows, n) if n_valid is None else np.clip(np.asarray(n_valid, dtype=np.int64), 0, n)
    inside = np.arange(n)[None, :] < nv[:, None]
    eps, eta0, momentum, rho = (float(np.float32(v)) for v in (eps, eta0, momentum, rho))
    lo, hi = (-np.inf, np.inf) if clip is None else (float(np.float32(clip[0])), float(np.float32(clip[1])))
    st = {}
    with np.errstate(invalid="ignore"):
        if first:
            f0 = np.where(np.isnan(fr), np.float32(-np.inf), fr).astype(np.float32)
            st["eta"] = np.full(rows, eta0, dtype=np.float32)
            st["f_best"], st["f_prev"], st["f_best_ckpt"] = f0.copy(), f0.copy(), f0.copy()
            for k in ("improved", "reduced_last", "fooled", "halvings"):
                st[k] = np.zeros(rows, dtype=np.int32)
            upd = np.ones(rows, dtype=bool)
        else:
            st = {k: np.array(state[k], dtype=np.float32 if k in STATE[:4] else np.int32) for k in STATE}
            if record is not None:
                for r in range(rows):
                    record[r] += [(float(fr[r]), float(st["f_prev"][r])), (float(fr[r]), float(st["f_best"][r]))]
            st["improved"] += (fr > st["f_prev"]).astype(np.int32)
            st["f_prev"] = fr.copy()
            upd = fr > st["f_best"]
            st["f_best"] = np.where(upd, fr, st["f_best"]).astype(np.float32)
    st["fooled"] = np.where(hit, 1, st["fooled"]).astype(np.int32)
    cur_x, cur_g = np.where(inside, x, x0), np.where(inside, g, x0)
    x_best[upd], g_best_new = cur_x[upd], g_best.copy()
    g_best_new[upd] = cur_g[upd]
    x_adv[hit] = cur_x[hit]
    stop = np.full(rows, bool(last)) | (nv == 0)
    restart = np.zeros(rows, dtype=bool)
    if ckpt_len > 0:
        c1 = st["improved"].astype(np.float64) < rho * ckpt_len
        c2 = (st["reduced_last"] == 0) & (st["f_best_ckpt"] == st["f_best"])
        restart = (c1 | c2) & ~stop
        go = ~stop
        st["eta"] = np.where(restart, st["eta"] * np.float32(0.5), st["eta"]).astype(np.float32)
        st["halvings"] = (st["halvings"] + restart).astype(np.int32)
        st["reduced_last"] = np.where(go, restart.astype(np.int32), st["reduced_last"]).astype(np.int32)
        st["improved"] = np.where(go, 0, st["improved"]).astype(np.int32)
        st["f_best_ckpt"] = np.where(go, st["f_best"], st["f_best_ckpt"]).astype(np.float32)
    out = dict(x_best=x_best, g_best=g_best_new, x_adv=x_adv, state=st, upd_best=upd, hit=hit, restart=restart, moved=~stop)
    if stop.all():
        return dict(out, x=None, x_prev=None)
    # the step from (xc, gc, xp): a restart starts from the best point (as it is AFTER the bookkeeping) without a momentum term
    xc = np.where(restart[:, None], x_best, x).astype(np.float64)
    gc = np.where(restart[:, None], g_best_new, g).astype(np.float64)
    xp = xc if first else np.where(restart[:, None], xc, x_prev.astype(np.float64))
    gc = np.where(np.isnan(gc), 0.0, gc)
    c = x0.astype(np.float64)
    l2 = float(norm) == 2.0
    with np.errstate(invalid="ignore", over="ignore"):
        if l2:
            nrm = np.sqrt((np.where(inside, gc, 0.0) ** 2).sum(axis=1, keepdims=True))
            d = np.where(np.isfinite(nrm) & np.isfinite(gc), gc / (nrm + TOL), 0.0)
        else:
            d = np.sign(gc)
        eta = st["eta"].astype(np.float64)[:, None]
        a = 1.0 if first else momentum
        z = _project(xc + eta * d, c, eps, lo, hi, l2, inside)
        xn = _project(xc + a * (z - xc) + (1.0 - a) * (xc - xp), c, eps, lo, hi, l2, inside)
    keep = stop[:, None]
    new_x = np.where(keep, x.astype(np.float64), np.where(inside, xn, c))
    new_prev = np.where(keep, x_prev.astype(np.float64), np.where(inside, xc, c))
    return dict(out, x=new_x, x_prev=new_prev)


def attack(spec, p, x, labels, eps, norm=np.inf, eps_step=None, max_iter=100, loss_type=0, targeted=False, clip=None, start=None):
    """AutoProjectedGradientDescent's loop for ONE run (no random restarts: ``start`` float32 [B, n] or None for x) on the float64
    model (spec, p) -> dict: adv float32 [B, n], success bool [B], loss float32 [B], halvings int32 [B], f_start float64 [B],
    comparisons: per row the list of (a, b), ambiguous bool [B]."""
    x0 = np.asarray(x, dtype=np.float32)
    B, n = x0.shape
    p64 = p.astype(np.float64)
    eta0 = 2.0 * eps if eps_step is None else eps_step
    cur = x0.copy() if start is None else np.asarray(start, dtype=np.float32).copy()
    x_prev, x_best, g_best, x_adv = x0.copy(), x0.copy(), np.zeros_like(x0), x0.copy()
    state, record = None, [[] for _ in range(B)]
    ck, prev, f_start = {}, 0, None
    for w in checkpoints(max_iter):
        ck[w], prev = w - prev, w
    kw = dict(norm=norm, eps=eps, eta0=eta0, clip=clip)
    g = np.zeros_like(x0)
    for k in range(max_iter + 1):
        z = P.forward_infer(spec, p64, cur.astype(np.float64), return_logits=True).astype(np.float32)
        L = loss(z, labels, loss_type, targeted)
        for r in range(B):
            record[r] += L["gaps"][r]
        if k == 0:
            f_start = L["f"].copy()
        f32 = L["f"].astype(np.float32)
        if k == max_iter:
            s = step(cur, x_prev, x0, g, x_best, g_best, x_adv, f32, L["hit"], state, last=True, record=record, **kw)
            x_best, g_best, x_adv, state = s["x_best"], s["g_best"], s["x_adv"], s["state"]
            break
        g = P.output_vjp_infer(spec, p64, cur.astype(np.float64), L["dz"].astype(np.float32).astype(np.float64), on_logits=True)[0]
        g = g.astype(np.float32)
        s = step(cur, x_prev, x0, g, x_best, g_best, x_adv, f32, L["hit"], state, first=k == 0, ckpt_len=ck.get(k, 0), record=record, **kw)
        x_best, g_best, x_adv, state = s["x_best"], s["g_best"], s["x_adv"], s["state"]
        cur, x_prev = s["x"].astype(np.float32), s["x_prev"].astype(np.float32)
    fooled = state["fooled"] != 0
    amb = np.array([any(abs(a - b) <= AMBIGUITY * max(abs(a), abs(b)) for a, b in rec if np.isfinite(a) and np.isfinite(b)) for rec in record])
    return dict(adv=np.where(fooled[:, None], x_adv, x_best), success=fooled, loss=state["f_best"], halvings=state["halvings"],
                f_start=f_start, comparisons=record, ambiguous=amb)


def objective(spec, p, x, labels, loss_type=0, targeted=False):
    """f at the rows x on the float64 model -> float64 [B]."""
    z = P.forward_infer(spec, p.astype(np.float64), np.asarray(x, dtype=np.float64), return_logits=True).astype(np.float32)
    return loss(z, labels, loss_type, targeted)["f"]


def within_ball(adv, x, eps, norm, valid=None):
    """The perturbation lies in the eps ball (norm inf: per element, with one unit in the last place of room; norm 2: 1e-6 relative)."""
    adv, x = np.asarray(adv, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d = adv - x if valid is None else np.where(valid, adv - x, 0.0)
    if float(norm) == 2.0:
        return bool((np.sqrt((d * d).sum(axis=1)) <= float(np.float32(eps)) * (1 + 1e-6) + 1e-7).all())
    room = float(np.float32(eps)) + np.spacing(np.float32(np.abs(x) + eps)).astype(np.float64)
    return bool((np.abs(d) <= room).all())
