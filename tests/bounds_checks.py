"""The checks that tests/test_bounds_cpu.py makes on the host twin and tests/test_bounds_gpu.py on the device: each takes what one
lipasr_mlp_bounds call returned (dict: margin_ibp, margin_crown, slack [B, C], lo, hi flat) and the case it was made on, and
compares with tests/bounds_ref.py.  Every bound below is computed from the case; none is a chosen number."""
import numpy as np

import bounds_ref as R

import lipasr._native as N


def spacing32(v):
    return np.spacing(np.maximum(np.abs(v), 2.0 ** -126).astype(np.float32)).astype(np.float64)


def boxes_of(out, m, B):
    w = m["widths"]
    lo0, llo = N.bounds_split_layers(out["lo"], w, B)
    hi0, lhi = N.bounds_split_layers(out["hi"], w, B)
    return {"box": (lo0, hi0), "z": [(a[0], b[0]) for a, b in zip(llo, lhi)], "h": [(a[1], b[1]) for a, b in zip(llo, lhi)]}


def check_enclosure_and_tightness(out, m, x, eps, norm, clip):
    """Per layer and element, from the call's OWN previous box: lo <= lo_f64 and hi >= hi_f64, no exceptions; and no further out
    than 3 w, w = widen(K, S) in float64.  The 3: the call's sums are off by at most w (that is what w bounds), it then steps
    out by its own w (of an S that is at most 1 + 4 gamma times the exact one), and rounds outward once more, less than one fp32
    spacing <= 2^-23 S <= 2 w / (K + 1) -- together below 3 w for K >= 3.  The affine map is made in float64 and rounded outward
    once: one spacing plus the 2^-40 margins."""
    B = x.shape[0]
    bx = boxes_of(out, m, B)
    e = np.asarray(eps, np.float64)[:, None]
    x64 = x.astype(np.float64)
    lo0, hi0 = R.input_box(x64, eps, clip)
    assert (bx["box"][0] <= lo0).all() and (bx["box"][1] >= hi0).all()
    tol0 = spacing32(lo0) + 4 * R.D * (np.abs(x64) + e)
    assert (lo0 - bx["box"][0] <= tol0).all() and (bx["box"][1] - hi0 <= spacing32(hi0) + 4 * R.D * (np.abs(x64) + e)).all()
    exact = np.asarray(eps)[:, None] == 0
    assert (np.where(exact, bx["box"][0] == x, True)).all() and (np.where(exact, bx["box"][1] == x, True)).all()
    lo, hi = bx["box"]
    worst = 0.0
    for l in range(len(m["W"]) - 1):
        K = m["widths"][l]
        zlo, zhi, S = R.ibp_layer(m, l, lo, hi, (x64, np.asarray(eps, np.float64)) if (norm == 2 and l == 0) else None)
        hzlo, hzhi = (a.astype(np.float64) for a in bx["z"][l])
        assert (hzlo <= zlo).all() and (hzhi >= zhi).all(), f"layer {l}: the pre-activation box does not enclose"
        w = R.widen(K, S)
        worst = max(worst, ((zlo - hzlo) / w).max(), ((hzhi - zhi) / w).max())
        assert (zlo - hzlo <= 3 * w).all() and (hzhi - zhi <= 3 * w).all(), f"layer {l}: looser than 3 w ({worst:.3f} w)"
        plo, phi = R.post_box(m, l, hzlo, hzhi)
        hlo, hhi = (a.astype(np.float64) for a in bx["h"][l])
        assert (hlo <= plo).all() and (hhi >= phi).all(), f"layer {l}: the activation box does not enclose"
        s, t = R.affine(m, l)
        tm = 0.0 if m["bn"][l] is None else np.abs(m["bn"][l][1].astype(np.float64)) + np.abs(s * m["bn"][l][2].astype(np.float64))
        mag = np.abs(s) * np.maximum(hzhi, 0) + tm
        assert (plo - hlo <= spacing32(hlo) + 8 * R.D * mag).all() and (hhi - phi <= spacing32(hhi) + 8 * R.D * mag).all()
        lo, hi = bx["h"][l]
    return worst


def check_sampling(out, m, x, eps, norm, clip, y, seed):
    """200 points of every row's input set: the float64 network's margins are >= both reported margins, no exceptions."""
    rng = np.random.default_rng(seed)
    for b in range(x.shape[0]):
        pts = R.sample_points(m, x[b], float(eps[b]), norm, clip, int(y[b]), rng)
        tm = R.true_margins(m, pts, int(y[b])).min(0)
        for name in ("margin_ibp", "margin_crown"):
            got = out[name][b].astype(np.float64)
            k = np.arange(tm.size) != y[b]
            assert (tm[k] >= got[k]).all(), f"row {b}: {name} {got[k]} above the sampled margins {tm[k]}"
            assert np.isposinf(got[y[b]])


def check_agreement(out, m, x, eps, norm, clip, y):
    """The reported margins against the float64 restatement run on the call's OWN boxes (so that no forward widening has to be
    propagated): margin_ibp within the fp32 spacing of its value plus the 2^-40 margins; margin_crown within the slack the call
    reports plus the drift the restatement computes for an fp32 run of the same chain."""
    B = x.shape[0]
    bx = boxes_of(out, m, B)
    lo, hi = bx["h"][-1] if bx["h"] else bx["box"]
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    WL, bL = m["W"][-1].astype(np.float64), m["b"][-1].astype(np.float64)
    x64 = x.astype(np.float64)
    bx64 = {"box": tuple(a.astype(np.float64) for a in bx["box"]), "z": bx["z"]}
    worst = 0.0
    for b in range(B):
        yb, e = int(y[b]), float(eps[b])
        k = np.arange(WL.shape[1]) != yb
        ref = R.margins_ibp(m, b, yb, lo, hi, norm, x64, e)
        H = np.maximum(np.abs(lo[b]), np.abs(hi[b]))
        if not bx["h"]:
            H = np.maximum(H, np.abs(x64[b]))
        mag = np.abs(WL[:, [yb]] - WL).T @ H + np.abs(bL[yb]) + np.abs(bL)
        got = out["margin_ibp"][b].astype(np.float64)
        assert (np.abs(got[k] - ref[k]) <= (spacing32(got) + 8 * R.D * mag)[k]).all(), f"row {b}: margin_ibp {got} vs {ref}"
        ref, drift, _ = R.crown(m, b, yb, bx64, norm, x64, e)
        got, sl = out["margin_crown"][b].astype(np.float64), out["slack"][b].astype(np.float64)
        tol = sl + drift + spacing32(got) + spacing32(sl)
        worst = max(worst, (np.abs(got[k] - ref[k]) / tol[k]).max())
        assert (np.abs(got[k] - ref[k]) <= tol[k]).all(), f"row {b}: margin_crown {got} vs {ref}, slack {sl}, drift {drift}"
        assert (sl[k] > 0).all() and sl[yb] == 0
    return worst
