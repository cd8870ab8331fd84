"""CROWN-IBP certified training without a GPU: the host twin lipasr_mlp_bounds_crown_grad_host (the same inline functions as the
kernels, in the same orders) against the autograd oracle of tests/bounds_crown_grad_ref.py on the six cases of tests/bounds_ref.py
and one at the class limit, at beta 1 and 0.5; the loss rows, beta = 0 against lipasr_mlp_bounds_grad_host, the scale_old mix, NaN
rows, every refusal of the native entry points and of lipasr.bounds.CrownIBPCrossentropy, its schedules, the driver flags, the ABI
bookkeeping and the float64 trainer of the functional recipe.

Tolerance: per parameter segment, in units of the segment's largest |float64 gradient|, 8 times what the oracle's own graph
loses when it is evaluated in float32, and not below 2^-22 ("CROWN-IBP certified training", records the measured
ratios).  The oracle takes the slack that lipasr_mlp_bounds subtracted from margin_crown as one more detached constant, next to
the widening: the slack is a constant of the derivative but not of the loss, it moves the softmax weights by its own size (1e-5
to 1e-4 of a margin here), and without it the host twin is 11 to 50 bounds away from the oracle on the cases with hidden layers.

Kink conditions, asserted on the float64 oracle before anything is compared: every pre-activation bound and every |z_hi + z_lo| of
an unstable neuron at least 8 widenings from 0, every non-zero p of an unstable neuron and every non-zero Lambda_0 over an open
input interval at least 8 times its fp32 drift.  The input seeds are len(case) as in tests/test_bounds_grad_cpu.py, except where
SEEDS says otherwise: at len(case) `wide` has |z_hi + z_lo| 3.2 widenings and a Lambda_0 7.3 drifts from 0."""
import ctypes as C
import functools

import numpy as np
import pytest

import bounds_crown_grad_ref as CR
import bounds_grad_ref as G
import bounds_ref as R
from test_bounds_grad_cpu import loss_tolerance

import lipasr._native as N

INF = float("inf")
CASES = dict(R.cases())
CASES["classes32"] = (R.make_model([19, 40, 32], 6, bn=(0,)), 3)
SEEDS = {"wide": 8, "classes32": 13}
BETAS = (1.0, 0.5)
KINK_MARGIN = 8.0


def layout_of(m):
    return N.bounds_layout(m["widths"], R.bn_flags(m))


def inputs_of(case):
    m, B = CASES[case]
    return R.case_inputs(m, B, SEEDS.get(case, len(case)))


@functools.lru_cache(maxsize=None)
def forward(case):
    """The host forward pass of a case with margin_crown: what lipasr_mlp_bounds hands to the backward pass."""
    m, B = CASES[case]
    x, eps, y = inputs_of(case)
    params, state = R.pack(m, layout_of(m))
    out = N.mlp_bounds_host(m["widths"], R.bn_flags(m), params, state, x, eps, INF, y, clip_lo=R.CLIP[0], clip_hi=R.CLIP[1], crown=True)
    return out, m, x, eps, y, params, state


@functools.lru_cache(maxsize=None)
def oracle(case, beta):
    out, m, x, eps, y, _, _ = forward(case)
    return CR.tolerances(m, x, eps, y, beta, layout_of(m), slack=out["slack"])


@functools.lru_cache(maxsize=None)
def kinks(case):
    _, m, x, eps, y, _, _ = forward(case)
    return CR.kinks(m, x, eps, y)


def host_grad(case, beta, **kw):
    out, m, x, eps, y, params, state = forward(case)
    return N.mlp_bounds_crown_grad_host(m["widths"], R.bn_flags(m), params, state, out["margin_ibp"], out["margin_crown"], out["lo"],
                                        out["hi"], y, beta, **kw)


def check_against_oracle(case, beta, got, what):
    """Asserts the kink conditions, then the gradient per segment and the loss rows; returns the largest error / bound."""
    out, m, x, eps, y, _, _ = forward(case)
    k = kinks(case)
    print(f"{case}: kink distances gate {k['gate']:.1f} w, flip {k['flip']:.1f} w, p {k['p']:.1f} drifts, Lambda_0 {k['lam0']:.1f} drifts")
    for name in ("gate", "flip", "p", "lam0"):
        assert k[name] >= KINK_MARGIN, f"{case}: {name} {k[name]:.2f} from a kink"
    rows, want, tol, err32 = oracle(case, beta)
    err, pads = G.segment_errors(got["grads"], want, m, layout_of(m))
    worst = 0.0
    for s in err:
        print(f"{what} {case} beta {beta} {s}: error {err[s]:.3e} of the segment's largest gradient, float32 oracle {err32[s]:.3e}, "
              f"ratio {err[s] / max(err32[s], 2.0 ** -25):.2f}, bound {tol[s]:.3e}")
        worst = max(worst, err[s] / tol[s])
    for s in err:
        assert err[s] <= tol[s], (case, beta, s, err[s], tol[s])
    assert pads == 0.0
    lr = np.abs(got["loss_rows"].astype(np.float64) - rows)
    lt = crown_loss_tolerance(case, beta, rows)
    print(f"{what} {case} beta {beta} loss_rows: largest |difference| / bound {(lr / lt).max():.3f} (largest bound {lt.max():.3e})")
    assert (lr <= lt).all()
    return worst


def crown_loss_tolerance(case, beta, rows):
    """test_bounds_grad_cpu.loss_tolerance (what the stored boxes' roundings move a margin by) extended by the CROWN chain's drift:
    bounds_ref.crown's bound on what an fp32 run of the chain moves margin_crown by, and the two roundings of the stored margin and
    slack, 2^-23 of their magnitude each."""
    out, m, x, eps, y, _, _ = forward(case)
    u = 2.0 ** -23
    own = np.eye(m["widths"][-1], dtype=bool)[y]
    mag = np.where(own, 0.0, np.abs(out["margin_crown"].astype(np.float64)) + np.abs(out["slack"].astype(np.float64)))
    return loss_tolerance(m, x, eps, y, rows) + beta * (kinks(case)["drift"] + u * mag).max(-1)


NAMES = ["lipasr_mlp_bounds_crown_grad_workspace", "lipasr_mlp_bounds_crown_grad", "lipasr_mlp_bounds_crown_grad_workspace_host",
         "lipasr_mlp_bounds_crown_grad_host", "lipasr_debug_bounds_crown_grad_launches"]


def test_abi_760():
    assert N.lib.lipasr_version() >= 760
    assert all(N.has(n) and hasattr(N.lib, n) and N.SINCE[n] == 760 and n in N.PROTOTYPES for n in NAMES)
    hook = N.lib.lipasr_debug_bounds_crown_grad_launches
    assert hook(len(N.BOUNDS_CROWN_GRAD_KERNELS)) == -1 and hook(-1) == -1 and hook(0) >= 0
    total = lambda L: sum(N.bounds_crown_grad_launches(L).values()) + sum(N.bounds_grad_launches(L).values())
    assert total(1) == 5 and all(total(L) == 10 * (L - 1) + 3 for L in range(2, 17))
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "lipasr.h")).read()
    assert all(n in header for n in NAMES) and "lipasr_version(): 760" in header and "10 (L - 1) + 3" in header


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", list(CASES))
def test_host_twin_against_autograd(case, beta):
    check_against_oracle(case, beta, host_grad(case, beta), "host")


@pytest.mark.parametrize("case", list(CASES))
def test_beta_zero_is_the_interval_backward_pass(case):
    out, m, x, eps, y, params, state = forward(case)
    want = N.mlp_bounds_grad_host(m["widths"], R.bn_flags(m), params, state, out["margin_ibp"], out["lo"], out["hi"], y)
    got = host_grad(case, 0.0)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    pre = np.random.default_rng(1).standard_normal(params.size).astype(np.float32)
    want = N.mlp_bounds_grad_host(m["widths"], R.bn_flags(m), params, state, out["margin_ibp"], out["lo"], out["hi"], y, scale_old=0.5,
                                  scale_new=0.25, grads=pre)
    got = host_grad(case, 0.0, scale_old=0.5, scale_new=0.25, grads=pre)
    assert all(np.array_equal(got[k], want[k]) for k in want)


def test_scale_old_mixes_into_what_is_there():
    _, m, *_ = forward("signed70")
    lay = layout_of(m)
    pre = np.zeros(lay[1], np.float32)
    rng = np.random.default_rng(3)
    used = np.zeros(lay[1], bool)
    for _, o, n in G.segments(m, lay):
        pre[o:o + n] = rng.standard_normal(n)
        used[o:o + n] = True
    plain = host_grad("signed70", 0.5)["grads"]
    mixed = host_grad("signed70", 0.5, scale_old=0.75, scale_new=0.5 / 70, grads=pre)["grads"]
    want = np.float32(0.75) * pre + np.float32(0.5 / 70) * plain
    assert np.abs(mixed - want).max() <= 2.0 ** -21 * np.abs(want).max()
    assert (mixed[~used] == 0).all()
    fresh = host_grad("signed70", 0.5, scale_old=0.0, grads=np.full(lay[1], np.nan, np.float32))["grads"]
    assert np.array_equal(fresh[used], plain[used])


def test_the_workspace_offset_changes_nothing_and_two_calls_agree():
    a, b, c = host_grad("signed", 1.0), host_grad("signed", 1.0, ws_offset=1), host_grad("signed", 1.0)
    assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in a)


@pytest.mark.parametrize("beta", BETAS)
def test_a_nan_row_makes_the_gradient_nan(beta):
    out, m, x, eps, y, params, state = forward("signed")
    call = lambda mi, mc, yy: N.mlp_bounds_crown_grad_host(m["widths"], R.bn_flags(m), params, state, mi, mc, out["lo"], out["hi"], yy, beta)
    for which in ("margin_ibp", "margin_crown"):
        mi, mc = out["margin_ibp"].copy(), out["margin_crown"].copy()
        (mi if which == "margin_ibp" else mc)[1] = np.nan
        got = call(mi, mc, y)
        assert np.isnan(got["loss_rows"][1]) and np.isfinite(got["loss_rows"][[0, 2]]).all(), which
        for _, o, n in G.segments(m, layout_of(m)):
            assert np.isnan(got["grads"][o:o + n]).any(), which
    bad_y = y.copy()
    bad_y[2] = 5
    got = call(out["margin_ibp"], out["margin_crown"], bad_y)
    assert np.isnan(got["loss_rows"][2]) and np.isfinite(got["loss_rows"][:2]).all()
    for _, o, n in G.segments(m, layout_of(m)):
        assert np.isnan(got["grads"][o:o + n]).any()


def test_known_answer_one_layer():
    """7 -> 3 at eps 0 is plain softmax regression at every beta: dW = x^T (p - onehot), db = sum (p - onehot)."""
    m, B = CASES["linear"]
    x, _, y = R.case_inputs(m, B, 0)
    params, _ = R.pack(m, layout_of(m))
    out = N.mlp_bounds_host(m["widths"], None, params, None, x, np.zeros(B, np.float32), INF, y, crown=True)
    z = R.forward(m, x)
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    g = p - np.eye(3)[y]
    lay = layout_of(m)[0][0]
    for beta in (1.0, 0.5, 0.25):
        got = N.mlp_bounds_crown_grad_host(m["widths"], None, params, None, out["margin_ibp"], out["margin_crown"], out["lo"], out["hi"], y, beta)
        assert np.abs(got["grads"][lay["W"]:lay["W"] + 21].reshape(7, 3) - x.astype(np.float64).T @ g).max() < 1e-5
        assert np.abs(got["grads"][lay["b"]:lay["b"] + 3] - g.sum(0)).max() < 1e-5
        assert np.abs(got["loss_rows"] + np.log(p[np.arange(B), y])).max() < 1e-5


# ------------------------------------------------------------------------------------------------------------------ refusals
def _raw_host_call(case="signed", beta=0.5, **over):
    out, m, x, eps, y, params, state = forward(case)
    w, b = m["widths"], x.shape[0]
    need = C.c_size_t()
    N.check(N.lib.lipasr_mlp_bounds_crown_grad_workspace_host(len(w) - 1, N.int_array(w), b, C.byref(need)))
    a = {"n_layers": len(w) - 1, "widths": N.int_array(w), "bn": N.int_array(R.bn_flags(m)), "params": params, "bnstate": state,
         "margin": out["margin_ibp"], "crown": out["margin_crown"], "lo": out["lo"], "hi": out["hi"],
         "y": np.ascontiguousarray(y, np.int32), "batch": b, "ws": np.zeros(need.value + 8, np.float32), "ws_floats": need.value,
         "grads": np.zeros(params.size, np.float32), "loss_rows": np.zeros(b, np.float32)}
    a.update(over)
    vp = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    return N.lib.lipasr_mlp_bounds_crown_grad_host(a["n_layers"], a["widths"], a["bn"], vp(a["params"]), vp(a["bnstate"]), vp(a["margin"]),
                                                   vp(a["crown"]), vp(a["lo"]), vp(a["hi"]), vp(a["y"]), a["batch"], beta, vp(a["ws"]),
                                                   a["ws_floats"], 0.0, 1.0, vp(a["grads"]), vp(a["loss_rows"]))


def test_native_refusals():
    assert _raw_host_call() == N.OK and _raw_host_call(beta=0.0) == N.OK and _raw_host_call(beta=1.0) == N.OK
    for name in ("params", "bnstate", "margin", "crown", "lo", "hi", "y", "ws", "grads", "loss_rows"):
        assert _raw_host_call(**{name: None}) == N.EINVAL, name
        assert _raw_host_call(beta=0.0, **{name: None}) == N.EINVAL, name
    assert "null" in N.last_error()
    for beta in (-0.01, 1.01, float("nan"), INF):
        assert _raw_host_call(beta=beta) == N.EINVAL and "beta" in N.last_error()
    assert _raw_host_call(ws_floats=16) == N.EINVAL and "workspace" in N.last_error()
    out, m, x, eps, y, params, state = forward("signed")
    assert _raw_host_call(grads=params) == N.EINVAL and "overlaps" in N.last_error()
    ws = np.zeros(1 << 18, np.float32)
    assert _raw_host_call(ws=ws) == N.OK
    assert _raw_host_call(ws=ws, loss_rows=ws[100:103]) == N.EINVAL
    assert _raw_host_call(ws=ws, lo=ws[:out["lo"].size]) == N.EINVAL
    assert _raw_host_call(ws=ws, crown=ws[:out["margin_crown"].size].reshape(3, 5)) == N.EINVAL
    assert _raw_host_call(batch=0) == N.EINVAL
    need = C.c_size_t()
    ws_host = N.lib.lipasr_mlp_bounds_crown_grad_workspace_host
    assert ws_host(2, N.int_array([8, 4097, 3]), 2, C.byref(need)) == N.EINVAL
    assert ws_host(2, N.int_array([8, 16, 33]), 2, C.byref(need)) == N.EINVAL and "classes" in N.last_error()
    assert ws_host(2, N.int_array([8, 16, 32]), (1 << 19) + 1, C.byref(need)) == N.EINVAL
    assert ws_host(2, N.int_array([8, 16, 32]), 1 << 19, C.byref(need)) == N.OK
    assert ws_host(2, N.int_array([8, 16, 32]), 4, None) == N.EINVAL
    assert ws_host(0, N.int_array([8]), 4, C.byref(need)) == N.EINVAL


def test_schedules_and_refusals_of_the_loss():
    from lipasr.bounds import CrownIBPCrossentropy, IBPCrossentropy

    loss = CrownIBPCrossentropy(0.2, kappa=0.5, warmup_steps=50, ramp_steps=150)
    assert isinstance(loss, IBPCrossentropy) and loss.certified and (loss.beta_start, loss.beta_end) == (1.0, 0.0)
    assert loss.schedule(0) == (0.0, 0.0) and loss.schedule(125) == pytest.approx((0.1, 0.25)) and loss.schedule(200) == (0.2, 0.5)
    assert loss.beta_schedule(0) == 1.0 and loss.beta_schedule(50) == 1.0 and loss.beta_schedule(125) == pytest.approx(0.5)
    assert loss.beta_schedule(200) == 0.0 and loss.beta_schedule(10 ** 6) == 0.0
    up = CrownIBPCrossentropy(0.1, warmup_steps=2, ramp_steps=4, beta_start=0.25, beta_end=0.75)
    assert [up.beta_schedule(s) for s in (0, 2, 4, 6, 9)] == pytest.approx([0.25, 0.25, 0.5, 0.75, 0.75])
    one = CrownIBPCrossentropy(0.1, beta_start=1.0, beta_end=1.0)
    assert all(one.beta_schedule(s) == 1.0 for s in (0, 1, 7)) and one.step == 0 and one.clip == (-INF, INF)
    for bad in (dict(eps=-0.1), dict(eps=0.1, kappa=1.5), dict(eps=0.1, ramp_steps=0), dict(eps=0.1, beta_start=1.5),
                dict(eps=0.1, beta_end=-0.1), dict(eps=0.1, beta_start=float("nan")), dict(eps=0.1, clip_values=(1, 0))):
        with pytest.raises(ValueError):
            CrownIBPCrossentropy(**bad)
    with pytest.raises(ValueError, match="norm 2 .*not built"):
        CrownIBPCrossentropy(0.1, norm=2)


def test_the_driver_flags_parse_and_default_to_ibp():
    import lipasr.train_constraints as TC
    import lipasr.train_google_dataset as TG
    from lipasr.bounds import CrownIBPCrossentropy, IBPCrossentropy

    for mod in (TC, TG):
        assert mod.certified_loss(mod.certified_arguments(["--certified-method", "crown-ibp"])) is None
        dflt = mod.certified_loss(mod.certified_arguments(["--certified-eps", "0.2"]))
        assert type(dflt) is IBPCrossentropy
        on = mod.certified_loss(mod.certified_arguments(["--certified-eps", "0.1", "--certified-kappa", "0.25", "--certified-warmup", "3",
                                                         "--certified-ramp", "7", "--certified-method", "crown-ibp"]))
        assert type(on) is CrownIBPCrossentropy and (on.eps, on.kappa, on.warmup_steps, on.ramp_steps) == (0.1, 0.25, 3, 7)
        assert (on.beta_start, on.beta_end) == (1.0, 0.0)
        flat = mod.certified_loss(mod.certified_arguments(["--certified-eps", "0.1", "--certified-method", "crown-ibp", "--certified-beta",
                                                           "1", "0.5"]))
        assert (flat.beta_start, flat.beta_end) == (1.0, 0.5)
        with pytest.raises(SystemExit):
            mod.certified_arguments(["--certified-method", "crown"])


def test_the_float64_trainer_on_the_harder_recipe():
    """The recipe of DESIGN.md, "CROWN-IBP certified training", seed 0, in float64: 10 blobs in 20 dimensions at noise 0.5,
    20 -> 64 -> 32 -> 10 with BatchNorm, Adam 1e-3, batch 64, 400 steps (50 warm-up, 200 ramp), kappa 1, eps 0.4, clip +-2.5;
    512 fresh rows certified by max(IBP, CROWN-IBP) at eps 0.4.  The thresholds are those of the device's functional test."""
    xt, yt = CR.blobs(512, 999)
    got = {}
    for method in ("ibp", "crown-ibp"):
        got[method] = CR.accuracies(CR.train(method, seed=0), xt, yt, 0.4)
        print(f"float64 {method}: clean accuracy {got[method][0]:.3f}, certified accuracy at eps 0.4 {got[method][1]:.3f}")
    assert got["crown-ibp"][0] >= 0.95 and got["crown-ibp"][1] >= 0.70 and got["crown-ibp"][1] >= got["ibp"][1] + 0.30
