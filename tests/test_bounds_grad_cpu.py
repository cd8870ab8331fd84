"""IBP certified training without a GPU: the host twin lipasr_mlp_bounds_grad_host (the same inline functions as the kernels, in
the same orders) against the autograd oracle of tests/bounds_grad_ref.py on every case of tests/bounds_ref.py, the loss rows, the
scale_old mix, NaN rows, every refusal of the native entry points and of lipasr.bounds.IBPCrossentropy, its schedule, the driver
flags and the ABI bookkeeping.

Tolerance: per parameter segment, in units of the segment's largest |float64 gradient|, 8 times what the oracle's own graph
loses when it is evaluated in float32, and not below 2^-22 ("Certified training", records the measured ratios)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bounds_grad_ref as G
import bounds_ref as R

import lipasr._native as N

INF = float("inf")
CASES = R.cases()
GATE_MARGIN = 8.0


def layout_of(m):
    return N.bounds_layout(m["widths"], R.bn_flags(m))


@functools.lru_cache(maxsize=None)
def forward(case):
    """The host forward pass of a case: what lipasr_mlp_bounds hands to the backward pass."""
    m, B = CASES[case]
    x, eps, y = R.case_inputs(m, B, len(case))
    params, state = R.pack(m, layout_of(m))
    out = N.mlp_bounds_host(m["widths"], R.bn_flags(m), params, state, x, eps, INF, y, clip_lo=R.CLIP[0], clip_hi=R.CLIP[1], crown=False)
    return out, m, x, eps, y, params, state


@functools.lru_cache(maxsize=None)
def oracle(case):
    _, m, x, eps, y, _, _ = forward(case)
    return G.tolerances(m, x, eps, y, layout_of(m))


def host_grad(case, **kw):
    out, m, x, eps, y, params, state = forward(case)
    return N.mlp_bounds_grad_host(m["widths"], R.bn_flags(m), params, state, out["margin_ibp"], out["lo"], out["hi"], y, **kw)


def check_against_oracle(case, got, what):
    """Asserts the gate distance, then the gradient per segment and the loss rows; returns the largest error / bound."""
    _, m, x, eps, y, _, _ = forward(case)
    dist = G.gate_distance(m, x, eps, y)
    assert dist >= GATE_MARGIN, f"{case}: a pre-activation bound {dist:.1f} widenings from 0"
    rows, want, tol, err32 = oracle(case)
    err, pads = G.segment_errors(got["grads"], want, m, layout_of(m))
    worst = 0.0
    for k in err:
        print(f"{what} {case} {k}: error {err[k]:.3e} of the segment's largest gradient, float32 oracle {err32[k]:.3e}, "
              f"ratio {err[k] / max(err32[k], 2.0 ** -25):.2f}, bound {tol[k]:.3e}")
        worst = max(worst, err[k] / tol[k])
    for k in err:
        assert err[k] <= tol[k], (case, k, err[k], tol[k])
    assert pads == 0.0
    lr = np.abs(got["loss_rows"].astype(np.float64) - rows)
    lt = loss_tolerance(m, x, eps, y, rows)
    print(f"{what} {case} loss_rows: largest |difference| / bound {(lr / lt).max():.3f} (largest bound {lt.max():.3e}), gate distance {dist:.1f} w")
    assert (lr <= lt).all()
    return worst


def loss_tolerance(m, x, eps, y, rows):
    """logsumexp moves by at most the largest change of a margin.  A margin of the device is the oracle's (which carries the
    widening) plus the fp32 roundings of what the forward pass stores, each at most u = 2^-23 of the stored magnitude, pushed
    through the layers above it: with H = max(|lo|, |hi|) of a box,
        dh_0 = u H_0;   dz_l = (dh_{l-1} + u H_{l-1}) |W_l| + u max|z_l|  (the centre of the box is rounded once more);
        dh_l = |s_l| dz_l + u H_l;   d margin_k = sum_j |d_kj| dh_{L-1,j} + u (sum_j |d_kj| H_j + |b_y| + |b_k|),
    and the loss itself is rounded to fp32 once."""
    u = 2.0 ** -23
    bx = R.ibp(m, x, eps, INF, R.CLIP)
    mag = lambda box: np.maximum(np.abs(box[0]), np.abs(box[1]))
    H = mag(bx["box"])
    dh = u * H
    for l in range(len(m["W"]) - 1):
        dz = (dh + u * H) @ np.abs(m["W"][l].astype(np.float64)) + u * mag(bx["z"][l])
        H = mag(bx["h"][l])
        dh = np.abs(R.affine(m, l)[0]) * dz + u * H
    WL, bL = m["W"][-1].astype(np.float64), m["b"][-1].astype(np.float64)
    dm = np.array([((dh[b] + u * H[b]) @ np.abs(WL[:, [y[b]]] - WL) + u * (np.abs(bL[y[b]]) + np.abs(bL))).max() for b in range(len(y))])
    return dm + u * np.abs(rows)


def test_abi_750():
    names = ["lipasr_mlp_bounds_grad_workspace", "lipasr_mlp_bounds_grad", "lipasr_mlp_bounds_grad_workspace_host",
             "lipasr_mlp_bounds_grad_host", "lipasr_debug_bounds_grad_launches"]
    assert N.lib.lipasr_version() >= 750
    assert all(N.has(n) and hasattr(N.lib, n) and N.SINCE[n] == 750 and n in N.PROTOTYPES for n in names)
    assert N.lib.lipasr_debug_bounds_grad_launches(len(N.BOUNDS_GRAD_KERNELS)) == -1 and N.lib.lipasr_debug_bounds_grad_launches(0) >= 0
    assert sum(N.bounds_grad_launches(7).values()) == 3 * 6 + 1 and sum(N.bounds_grad_launches(1).values()) == 2
    assert all(sum(N.bounds_grad_launches(L).values()) <= 3 * (L - 1) + 2 for L in range(1, 17))


@pytest.mark.parametrize("case", list(CASES))
def test_host_twin_against_autograd(case):
    check_against_oracle(case, host_grad(case), "host")


def test_scale_old_mixes_into_what_is_there():
    _, m, *_ = forward("signed70")
    lay = layout_of(m)
    pre = np.zeros(lay[1], np.float32)
    rng = np.random.default_rng(3)
    for _, o, n in G.segments(m, lay):
        pre[o:o + n] = rng.standard_normal(n)
    plain = host_grad("signed70")["grads"]
    mixed = host_grad("signed70", scale_old=0.75, scale_new=0.5 / 70, grads=pre)["grads"]
    want = np.float32(0.75) * pre + np.float32(0.5 / 70) * plain
    assert np.abs(mixed - want).max() <= 2.0 ** -22 * np.abs(want).max()
    used = np.zeros(lay[1], bool)
    for _, o, n in G.segments(m, lay):
        used[o:o + n] = True
    assert (mixed[~used] == 0).all() and np.array_equal(host_grad("signed70", scale_old=0.0, grads=np.full(lay[1], np.nan, np.float32))["grads"][used], plain[used])


def test_the_workspace_offset_changes_nothing():
    a, b = host_grad("signed"), host_grad("signed", ws_offset=1)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_a_nan_row_makes_the_gradient_nan():
    out, m, x, eps, y, params, state = forward("signed")
    margin = out["margin_ibp"].copy()
    margin[1] = np.nan
    got = N.mlp_bounds_grad_host(m["widths"], R.bn_flags(m), params, state, margin, out["lo"], out["hi"], y)
    assert np.isnan(got["loss_rows"][1]) and np.isfinite(got["loss_rows"][[0, 2]]).all()
    for _, o, n in G.segments(m, layout_of(m)):
        assert np.isnan(got["grads"][o:o + n]).any()
    bad_y = y.copy()
    bad_y[2] = 5
    got = N.mlp_bounds_grad_host(m["widths"], R.bn_flags(m), params, state, out["margin_ibp"], out["lo"], out["hi"], bad_y)
    assert np.isnan(got["loss_rows"][2]) and np.isfinite(got["loss_rows"][:2]).all()


def test_known_answer_one_layer():
    """7 -> 3 at eps 0 is plain softmax regression: dW = x^T (p - onehot), db = sum (p - onehot)."""
    m, B = CASES["linear"]
    x, _, y = R.case_inputs(m, B, 0)
    params, state = R.pack(m, layout_of(m))
    out = N.mlp_bounds_host(m["widths"], None, params, None, x, np.zeros(B, np.float32), INF, y, crown=False)
    got = N.mlp_bounds_grad_host(m["widths"], None, params, None, out["margin_ibp"], out["lo"], out["hi"], y)
    z = R.forward(m, x)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    g = p - np.eye(3)[y]
    lay = layout_of(m)[0][0]
    assert np.abs(got["grads"][lay["W"]:lay["W"] + 21].reshape(7, 3) - x.astype(np.float64).T @ g).max() < 1e-5
    assert np.abs(got["grads"][lay["b"]:lay["b"] + 3] - g.sum(0)).max() < 1e-5
    assert np.abs(got["loss_rows"] + np.log(p[np.arange(B), y])).max() < 1e-5


# ------------------------------------------------------------------------------------------------------------------ refusals
def _raw_host_call(case="signed", **over):
    out, m, x, eps, y, params, state = forward(case)
    w, b = m["widths"], x.shape[0]
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_grad_workspace_host(len(w) - 1, N.int_array(w), b, C.byref(need)))
    a = {"n_layers": len(w) - 1, "widths": N.int_array(w), "bn": N.int_array(R.bn_flags(m)), "params": params, "bnstate": state,
         "margin": out["margin_ibp"], "lo": out["lo"], "hi": out["hi"], "y": np.ascontiguousarray(y, np.int32), "batch": b,
         "ws": np.zeros(need.value + 8, np.float32), "ws_floats": need.value, "grads": np.zeros(params.size, np.float32),
         "loss_rows": np.zeros(b, np.float32)}
    a.update(over)
    vp = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    return N.lib.lipasr_mlp_bounds_grad_host(a["n_layers"], a["widths"], a["bn"], vp(a["params"]), vp(a["bnstate"]), vp(a["margin"]), vp(a["lo"]),
                                             vp(a["hi"]), vp(a["y"]), a["batch"], vp(a["ws"]), a["ws_floats"], 0.0, 1.0, vp(a["grads"]),
                                             vp(a["loss_rows"]))


def test_native_refusals():
    assert _raw_host_call() == N.OK
    for name in ("params", "bnstate", "margin", "lo", "hi", "y", "ws", "grads", "loss_rows"):
        assert _raw_host_call(**{name: None}) == N.EINVAL, name
    assert "null" in N.last_error()
    assert _raw_host_call(ws_floats=16) == N.EINVAL and "workspace" in N.last_error()
    out, m, x, eps, y, params, state = forward("signed")
    assert _raw_host_call(grads=params) == N.EINVAL and "overlaps" in N.last_error()
    ws = np.zeros(1 << 16, np.float32)
    assert _raw_host_call(ws=ws, loss_rows=ws[100:103]) == N.EINVAL
    assert _raw_host_call(ws=ws, lo=ws[:out["lo"].size]) == N.EINVAL
    assert _raw_host_call(batch=0) == N.EINVAL
    need = C.c_size_t()
    ws_host = N.lib.lipasr_mlp_bounds_grad_workspace_host
    assert ws_host(2, N.int_array([8, 4097, 3]), 2, C.byref(need)) == N.EINVAL
    assert ws_host(2, N.int_array([8, 16, 33]), 2, C.byref(need)) == N.EINVAL and "classes" in N.last_error()
    assert ws_host(2, N.int_array([8, 16, 32]), (1 << 19) + 1, C.byref(need)) == N.EINVAL
    assert ws_host(2, N.int_array([8, 16, 32]), 1 << 19, C.byref(need)) == N.OK
    assert ws_host(2, N.int_array([8, 16, 32]), 4, None) == N.EINVAL


def test_schedule_and_refusals_of_the_loss():
    from lipasr.bounds import IBPCrossentropy
    from lipasr.keras import CategoricalCrossentropy

    loss = IBPCrossentropy(0.2, kappa=0.5, warmup_steps=50, ramp_steps=150)
    assert isinstance(loss, CategoricalCrossentropy)
    assert loss.schedule(0) == (0.0, 0.0) and loss.schedule(50) == (0.0, 0.0)
    assert loss.schedule(125) == pytest.approx((0.1, 0.25)) and loss.schedule(200) == (0.2, 0.5) and loss.schedule(10 ** 6) == (0.2, 0.5)
    e, k = loss.schedule(51)
    assert 0 < e < 0.2 and 0 < k < 0.5
    assert IBPCrossentropy(0.1).schedule(0) == (0.0, 0.0) and IBPCrossentropy(0.1).schedule(1) == (0.1, 0.5)
    assert loss.step == 0 and loss.clip == (-INF, INF) and IBPCrossentropy(0.1, clip_values=(-1, 2)).clip == (-1.0, 2.0)
    for bad in (dict(eps=-0.1), dict(eps=float("nan")), dict(eps=0.1, kappa=1.5), dict(eps=0.1, kappa=-0.1), dict(eps=0.1, ramp_steps=0),
                dict(eps=0.1, warmup_steps=-1), dict(eps=0.1, clip_values=(1, 0))):
        with pytest.raises(ValueError):
            IBPCrossentropy(**bad)
    with pytest.raises(ValueError, match="norm 2 .*not built"):
        IBPCrossentropy(0.1, norm=2)
    assert IBPCrossentropy(0.1, norm="inf").eps == 0.1 and IBPCrossentropy(0.1, norm=np.inf).kappa == 0.5


def test_the_driver_flags_parse_and_default_to_off():
    import lipasr.train_constraints as TC
    import lipasr.train_google_dataset as TG

    for mod in (TC, TG):
        off = mod.certified_loss(mod.certified_arguments([]))
        assert off is None
        on = mod.certified_loss(mod.certified_arguments(["--certified-eps", "0.1", "--certified-kappa", "0.25", "--certified-warmup", "3",
                                                         "--certified-ramp", "7"]))
        assert (on.eps, on.kappa, on.warmup_steps, on.ramp_steps) == (0.1, 0.25, 3, 7)
        dflt = mod.certified_loss(mod.certified_arguments(["--certified-eps", "0.2"]))
        assert (dflt.kappa, dflt.warmup_steps, dflt.ramp_steps) == (0.5, 0, 1)
