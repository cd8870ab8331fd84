"""Bound propagation without a GPU: the host twin lipasr_mlp_bounds_host (the same inline functions as the kernels, in the same
orders) against the float64 restatement of tests/bounds_ref.py -- enclosure and tightness layer by layer, soundness on sampled
points, agreement of both margins, known answers, every refusal, NaN containment and the ABI bookkeeping."""
import ctypes as C
import functools

import numpy as np
import pytest

import bounds_checks as K
import bounds_ref as R

import lipasr._native as N

INF = float("inf")
CASES = R.cases()
NORMS = [INF, 2]
GRID = [(c, n) for c in CASES for n in NORMS]
IDS = [f"{c}-{'inf' if n == INF else 2}" for c, n in GRID]


def packed(m):
    return R.pack(m, N.bounds_layout(m["widths"], R.bn_flags(m)))


@functools.lru_cache(maxsize=None)
def run(case, norm, ws_offset=0):
    m, B = CASES[case]
    x, eps, y = R.case_inputs(m, B, len(case))
    params, state = packed(m)
    out = N.mlp_bounds_host(m["widths"], R.bn_flags(m), params, state, x, eps, norm, y, clip_lo=R.CLIP[0], clip_hi=R.CLIP[1],
                            ws_offset=ws_offset)
    return out, m, x, eps, y


def test_the_cases_cover_what_they_should():
    m, B = CASES["signed70"]
    x, eps, y = R.case_inputs(m, B, len("signed70"))
    bx = R.ibp(m, x, eps, INF, R.CLIP)
    unstable = np.mean([((lo < 0) & (hi > 0)).mean(1) for lo, hi in bx["z"]], axis=0)
    assert (eps == 0).any() and (unstable[eps == np.float32(1e-4)] < 0.1).all() and (unstable[eps == np.float32(0.3)] > 0.5).all()
    lo0, hi0 = bx["box"]
    cut = (lo0 == R.CLIP[0]).any(1) & (hi0 == R.CLIP[1]).any(1)
    assert cut[eps == 4.0].all()
    g = m["bn"][0][0]
    assert (g < 0).any() and (g == 0).any() and (m["W"][0] < 0).any() and (CASES["nonneg"][0]["W"][0] >= 0).all()


@pytest.mark.parametrize("case,norm", GRID, ids=IDS)
def test_boxes_enclose_and_are_tight(case, norm):
    out, m, x, eps, y = run(case, norm)
    worst = K.check_enclosure_and_tightness(out, m, x, eps, norm, R.CLIP)
    print(f"{case} norm {norm}: loosest side {worst:.3f} w")


@pytest.mark.parametrize("case,norm", GRID, ids=IDS)
def test_margins_hold_on_sampled_points(case, norm):
    out, m, x, eps, y = run(case, norm)
    K.check_sampling(out, m, x, eps, norm, R.CLIP, y, seed=7)


@pytest.mark.parametrize("case,norm", GRID, ids=IDS)
def test_margins_agree_with_float64(case, norm):
    out, m, x, eps, y = run(case, norm)
    worst = K.check_agreement(out, m, x, eps, norm, R.CLIP, y)
    print(f"{case} norm {norm}: largest |difference| / bound {worst:.3f}")


@pytest.mark.parametrize("norm", NORMS)
def test_the_workspace_offset_changes_nothing(norm):
    a, b = run("signed", norm)[0], run("signed", norm, 1)[0]
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_crown_is_what_tightens_the_signed_model():
    out = run("signed70", INF)[0]
    fin = np.isfinite(out["margin_ibp"])
    assert (out["margin_crown"][fin] > out["margin_ibp"][fin]).mean() > 0.5


# ------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("norm", NORMS)
def test_linear_model_gives_the_dual_norm(norm):
    m, B = CASES["linear"]
    x, _, y = R.case_inputs(m, B, 0)
    eps = np.array([0.0, 0.05, 0.5], np.float32)
    params, state = packed(m)
    out = N.mlp_bounds_host(m["widths"], None, params, None, x, eps, norm, y)
    W, b = m["W"][0].astype(np.float64), m["b"][0].astype(np.float64)
    for r in range(B):
        d = W[:, [y[r]]] - W
        true = x[r].astype(np.float64) @ d + b[y[r]] - b
        want = true - float(eps[r]) * (np.abs(d).sum(0) if norm == INF else np.sqrt((d * d).sum(0)))
        k = np.arange(3) != y[r]
        # the call's own slack, once for each margin: the box is one fp32 spacing wider than eps on either side
        tol = out["slack"][r] + np.abs(d).sum(0) * K.spacing32(np.abs(x[r]).max() + eps[r]) + K.spacing32(want)
        for name in ("margin_ibp", "margin_crown"):
            assert (np.abs(out[name][r] - want)[k] <= tol[k]).all() and (out[name][r][k] <= want[k]).all()


@pytest.mark.parametrize("case", ["signed", "nonneg", "signed70"])
def test_eps_zero_gives_the_true_margin(case):
    """At eps = 0 the input box is the point x, so the margin is the true one up to what the call took off (its slack), what fp32
    moved (the drift) and what the few neurons whose widened box straddles 0 lose (the gap): all three computed."""
    out, m, x, eps, y = run(case, INF)
    rows = np.flatnonzero(eps == 0)
    assert rows.size
    bx = K.boxes_of(out, m, x.shape[0])
    for r in rows:
        true = R.true_margins(m, x[r].astype(np.float64), int(y[r]))
        k = np.arange(true.size) != y[r]
        got, sl = out["margin_crown"][r].astype(np.float64), out["slack"][r].astype(np.float64)
        _, drift, gap = R.crown(m, r, int(y[r]), {"box": bx["box"], "z": bx["z"]}, INF, x.astype(np.float64), 0.0)
        assert (got[k] <= true[k]).all() and (true[k] - got[k] <= (sl + drift + gap + K.spacing32(got))[k]).all()


def test_two_neurons_by_hand():
    """x in [-1, 1]; z = (x + 0.5, x + 2): the first ReLU is unstable on [-0.5, 1.5], the second stable.  The margin of class 1 over
    class 0 is a_2 - a_1.  CROWN: -a_1 >= -0.75 (z_1 + 0.5), so the margin >= 0.25 x + 1.25 >= 1.0 (the true minimum, at x = -1);
    IBP: 1 - 1.5 = -0.5."""
    widths = [1, 2, 2]
    m = {"widths": widths, "W": [np.array([[1.0, 1.0]], np.float32), np.eye(2, dtype=np.float32)],
         "b": [np.array([0.5, 2.0], np.float32), np.zeros(2, np.float32)], "bn": [None, None]}
    params, state = packed(m)
    out = N.mlp_bounds_host(widths, None, params, None, np.zeros((1, 1), np.float32), np.ones(1, np.float32), INF,
                            np.array([1], np.int32))
    sl = float(out["slack"][0, 0])
    assert 0 < sl < 1e-5
    assert 1.0 - 2 * sl - 1e-6 <= out["margin_crown"][0, 0] <= 1.0
    assert -0.5 - 1e-5 <= out["margin_ibp"][0, 0] <= -0.5
    assert np.isposinf(out["margin_crown"][0, 1]) and np.isposinf(out["margin_ibp"][0, 1])


# ------------------------------------------------------------------------------------------------------ refusals and the ABI
def _raw_call(m, B, **over):
    """lipasr_mlp_bounds_host with one argument replaced; returns the return code."""
    x, eps, y = R.case_inputs(m, B, 0)
    params, state = packed(m)
    w = m["widths"]
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_workspace_host(len(w) - 1, N.int_array(w), B, C.byref(need)))
    ws = np.zeros(need.value + 8, np.float32)
    c = w[-1]
    a = {"n_layers": len(w) - 1, "widths": N.int_array(w), "bn": N.int_array(R.bn_flags(m)), "params": params, "bnstate": state, "x": x,
         "eps": eps, "norm": INF, "clip_lo": -INF, "clip_hi": INF, "y": y, "batch": B, "ws": ws, "ws_floats": need.value,
         "ibp": np.zeros((B, c), np.float32), "crown": np.zeros((B, c), np.float32), "slack": np.zeros((B, c), np.float32),
         "lo": None, "hi": None}
    a.update(over)
    keep = list(a.values())
    v = lambda k: a[k] if not isinstance(a[k], np.ndarray) else C.c_void_p(a[k].ctypes.data)
    rc = N.lib.lipasr_mlp_bounds_host(a["n_layers"], a["widths"], a["bn"], v("params"), v("bnstate"), v("x"), v("eps"), a["norm"],
                                      a["clip_lo"], a["clip_hi"], v("y"), a["batch"], v("ws"), a["ws_floats"], v("ibp"), v("crown"),
                                      v("slack"), v("lo"), v("hi"))
    del keep
    return rc


def test_refusals():
    m, B = CASES["signed"]
    assert _raw_call(m, B) == N.OK
    for name in ("params", "bnstate", "x", "eps", "y", "ws", "ibp", "widths"):
        assert _raw_call(m, B, **{name: None}) == N.EINVAL, name
    assert "null" in N.last_error()
    assert _raw_call(m, B, crown=None) == N.EINVAL  # the slack without the margin it belongs to
    assert _raw_call(m, B, crown=None, slack=None) == N.OK
    for norm in (1.0, 0.0, float("nan"), -INF):
        assert _raw_call(m, B, norm=norm) == N.EINVAL
    assert "norm" in N.last_error()
    x, eps, y = R.case_inputs(m, B, 0)
    for bad in (-1e-3, float("nan")):
        e = eps.copy()
        e[1] = bad
        assert _raw_call(m, B, eps=e) == N.EINVAL and "eps[1]" in N.last_error()
    yy = y.copy()
    yy[2] = 5
    assert _raw_call(m, B, y=yy) == N.EINVAL
    assert _raw_call(m, B, ws_floats=10) == N.EINVAL and "workspace" in N.last_error()
    assert _raw_call(m, B, clip_lo=1.0, clip_hi=0.0) == N.EINVAL
    assert _raw_call(m, B, batch=0) == N.EINVAL
    assert _raw_call(m, B, n_layers=0) == N.EINVAL and _raw_call(m, B, n_layers=N.MAX_LAYERS + 1) == N.EINVAL
    # classes > 32, a width the constants do not cover
    need = C.c_size_t()
    assert N.lib.lipasr_mlp_bounds_workspace_host(1, N.int_array([4, 33]), 1, C.byref(need)) == N.EINVAL and "classes" in N.last_error()
    assert N.lib.lipasr_mlp_bounds_workspace_host(2, N.int_array([4, 4097, 3]), 1, C.byref(need)) == N.EINVAL
    assert N.lib.lipasr_mlp_bounds_workspace_host(1, N.int_array([4, 3]), 1, None) == N.EINVAL
    # overlapping spans: an output inside the workspace, two outputs on each other, an output on an input
    c = m["widths"][-1]
    ws = np.zeros(1 << 16, np.float32)
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_workspace_host(3, N.int_array(m["widths"]), B, C.byref(need)))
    assert _raw_call(m, B, ws=ws, ibp=ws[100:100 + B * c].reshape(B, c)) == N.EINVAL and "overlaps" in N.last_error()
    both = np.zeros((B, c), np.float32)
    assert _raw_call(m, B, ibp=both, crown=both) == N.EINVAL
    xx = np.zeros((B, m["widths"][0]), np.float32)
    assert _raw_call(m, B, x=xx, ibp=xx[:, :c]) == N.EINVAL


@pytest.mark.parametrize("norm", NORMS)
def test_a_nan_stays_in_its_row(norm):
    m, B = CASES["signed"]
    x, eps, y = R.case_inputs(m, B, len("signed"))
    params, state = packed(m)
    kw = dict(clip_lo=R.CLIP[0], clip_hi=R.CLIP[1])
    good = N.mlp_bounds_host(m["widths"], R.bn_flags(m), params, state, x, eps, norm, y, **kw)
    xb = x.copy()
    xb[1, 5] = np.nan
    bad = N.mlp_bounds_host(m["widths"], R.bn_flags(m), params, state, xb, eps, norm, y, **kw)
    for name in ("margin_ibp", "margin_crown", "slack"):
        assert np.isnan(bad[name][1]).all()
        assert np.array_equal(bad[name][[0, 2]], good[name][[0, 2]])


def test_abi_bookkeeping():
    names = ("lipasr_mlp_bounds", "lipasr_mlp_bounds_workspace", "lipasr_mlp_bounds_host", "lipasr_mlp_bounds_workspace_host",
             "lipasr_debug_bounds_launches")
    assert N.lib.lipasr_version() >= 710
    assert all(N.has(n) and N.SINCE[n] == 710 and n in N.PROTOTYPES for n in names)
    assert [N.lib.lipasr_debug_bounds_launches(i) >= 0 for i in range(5)] == [True] * 5 and N.lib.lipasr_debug_bounds_launches(5) == -1
    assert len(N.BOUNDS_KERNELS) == 5


def test_widening_constants():
    assert R.gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24)
    assert R.widen(880, 1.0) == R.gamma(881) + 2 * 881 * 2.0 ** -149
