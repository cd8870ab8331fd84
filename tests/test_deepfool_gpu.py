"""DeepFool on the MI355X: lipasr_deepfool_step against the float64 definition of tests/deepfool_ref.py on the same arrays, its edge
conventions (include/lipasr.h), lipasr.attacks.DeepFool over features against the float64 attack on the oracle classifier and over
audio against the float64 graph of tests/mfcc_grad_ref.py, and the read-outs built on it (get_robustness_radius, radius_report).

Bounds.  Kernel: 1e-5, the bound of test_sigma_kernel_matches_svd -- the sums are fp64, so what is left is the fp32 rounding of
dist and of each x (6e-8), and a dropped or doubled column would move ||w||^2 by order 1 / n >= 4.5e-5.  The step is compared on
x = 0, where x + r is r rounded once; on a random x the rounding of the sum to fp32 (half a unit in the last place of the result)
is added to the bound, because it does not shrink with r.  Attack over features: the issue's -- iteration counts equal to the
float64 attack's (the float32 attack on the CPU has the same counts on these rows), ``found`` within 1e-3.  Audio: 8 x the error
of the same oracle graph evaluated in float32 on the CPU, the factor of the backward-pass tests."""
import wave

import numpy as np
import pytest
import torch

import deepfool_ref as D
import local_lip_ref as R
import mfcc_grad_ref as G
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

OVERSHOOT = 0.02


# =================================================================================================
# 1. the kernel against the float64 definition on the same arrays
# =================================================================================================
def _place(J, layout, offset=0):
    """float32 [B, C, n] -> a device view [B, C, n] over [B][C][n] ("bcn") or class-major [C][B][n] ("cbn") storage that starts
    ``offset`` floats into its allocation."""
    B, C, n = J.shape
    buf = torch.zeros(B * C * n + offset, device="cuda")
    if layout == "bcn":
        view = buf[offset:].view(B, C, n)
    else:
        view = buf[offset:].view(C, B, n).permute(1, 0, 2)
    view.copy_(torch.as_tensor(J))
    return view


def _place_x(x, offset=0):
    buf = torch.zeros(x.size + offset, device="cuda")
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _random_jac(B, C, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, C, n)) * rng.uniform(0.2, 2.0, (B, C, 1))).astype(np.float32)


def _random_case(B, C, n, seed):
    """-> (J float32 [B, C, n], out float32 [B, C], label int32 [B] = argmax out, x float32 [B, n])"""
    J = _random_jac(B, C, n, seed)
    rng = np.random.default_rng(seed + 1000)
    out = rng.standard_normal((B, C)).astype(np.float32)
    return J, out, out.argmax(axis=1).astype(np.int32), rng.standard_normal((B, n)).astype(np.float32)


def _rho_gap(J, out, label, norm):
    """The smallest relative gap between the two smallest rho_k of any row (inf with a single candidate), float64."""
    gap = np.inf
    J, out = J.astype(np.float64), out.astype(np.float64)
    for b in range(J.shape[0]):
        c = int(label[b])
        w = J[b] - J[b, c]
        nrm = np.sqrt((w * w).sum(axis=1)) if norm == 2 else np.abs(w).sum(axis=1)
        rho = np.sort(np.delete(np.abs(out[b] - out[b, c]) / (nrm + D.TOL), c))
        if rho.shape[0] > 1:
            gap = min(gap, (rho[1] - rho[0]) / rho[0])
    return gap


def _step(J, out, label, x, norm=2, overshoot=OVERSHOOT, clip=None, allowed=None, layout="bcn", offset=0, x_offset=0):
    """-> (x_new, dist, target, state) as NumPy, from one lipasr_deepfool_step."""
    from lipasr.attacks import deepfool_step

    jt = _place(np.asarray(J, dtype=np.float32), layout, offset)
    xt = _place_x(np.asarray(x, dtype=np.float32), x_offset)
    ot = torch.as_tensor(np.asarray(out, dtype=np.float32)).cuda().contiguous()
    lt = torch.as_tensor(np.asarray(label, dtype=np.int32)).cuda()
    at = None if allowed is None else torch.as_tensor(np.asarray(allowed, dtype=np.uint32).view(np.int32)).cuda()
    dist, target, state = deepfool_step(jt, ot, lt, xt, norm, overshoot, clip, at)
    torch.cuda.synchronize()
    return xt.cpu().numpy(), dist.cpu().numpy(), target.cpu().numpy(), state.cpu().numpy()


def _check_step(J, out, label, x, got, norm, what, **kw):
    """One device step against deepfool_ref.step on the same float32 arrays."""
    x_new, dist, target, state = got
    want_x, r, want_d, want_t, want_s = D.step(J, out, label, x, norm=norm, overshoot=OVERSHOOT, **kw)
    np.testing.assert_array_equal(state, want_s)
    np.testing.assert_array_equal(target, want_t)
    moved = want_x - x.astype(np.float64)
    scale = np.abs(moved).max(axis=1)
    e_d = np.abs(dist - want_d) / want_d
    e_x = np.abs((x_new.astype(np.float64) - x) - moved).max(axis=1)
    half_ulp = 0.5 * np.spacing(np.abs(want_x).astype(np.float32)).astype(np.float64).max(axis=1) if np.any(x) else 0.0
    print(f"{what}: dist relative error {e_d.max():.2e}; step error / max |step| {(e_x / scale).max():.2e} (bound 1e-5"
          f"{' + half a unit in the last place of x' if np.any(x) else ''})")
    assert (e_d <= 1e-5).all()
    assert (e_x <= 1e-5 * scale + half_ulp).all()


SHAPES = [(1, 10, 880), (3, 20, 2020), (2, 10, 22050), (5, 2, 1), (4, 32, 67), (2, 10, 881), (2, 15, 260)]


def _seed(shape):
    """sum(shape), the seeds of test_sigma_kernel_matches_svd: at every one of them the two smallest rho_k of every row differ by
    more than 0.1 relative in both norms (asserted below at 1e-3), so none had to be moved."""
    return sum(shape)


@pytest.mark.parametrize("layout", ["bcn", "cbn"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_kernel_matches_float64(cuda, shape, layout):
    J, out, label, x = _random_case(*shape, seed=_seed(shape))
    zero = np.zeros_like(x)
    for norm in (2, np.inf):
        assert _rho_gap(J, out, label, norm) > 1e-3  # the choice of l does not hang on rounding
        _check_step(J, out, label, zero, _step(J, out, label, zero, norm, layout=layout), norm, f"{shape} {layout} norm {norm} x = 0")
        _check_step(J, out, label, x, _step(J, out, label, x, norm, layout=layout), norm, f"{shape} {layout} norm {norm} random x")
        # once more with the Jacobian, then x, one float off 16-byte alignment: the 4-byte loads, the same result
        a = _step(J, out, label, zero, norm, layout=layout)
        for off in (dict(offset=1), dict(x_offset=1)):
            b = _step(J, out, label, zero, norm, layout=layout, **off)
            _check_step(J, out, label, zero, b, norm, f"{shape} {layout} norm {norm} {off}")
            np.testing.assert_array_equal(b[2], a[2])
            np.testing.assert_allclose(b[0], a[0], rtol=2e-6, atol=0)


# =================================================================================================
# 2. edges (the conventions of include/lipasr.h)
# =================================================================================================
def test_flipped_rows_keep_their_bits_and_ties_take_the_lowest_index(cuda):
    J, out, label, x = _random_case(4, 10, 881, seed=5)
    x[1, 7] = -0.0
    label[1] = (label[1] + 1) % 10  # row 1 has already left its class
    out[2, :] = -1.0
    out[2, [3, 6]] = 2.0  # an argmax tie: the lowest index, 3, is the class
    label[2] = 6          # ... so a row labelled 6 has left it
    out[3, :] = -1.0
    out[3, [3, 6]] = 2.0
    label[3] = 3          # and a row labelled 3 is still there (and sits on the boundary with 6: rho = 0)
    x_new, dist, target, state = _step(J, out, label, x, clip=(-0.5, 0.5))
    assert state.tolist() == [1, 0, 0, 1]
    assert target[1] == out[1].argmax() and target[2] == 3 and target[3] == 6
    assert dist[1] == 0 and dist[2] == 0 and dist[3] == 0
    for b in (1, 2):  # not even clipped
        assert x_new[b].tobytes() == x[b].tobytes()
    # two identical candidate rows of J with the same f: a rho tie, the lowest index
    J, out, label, x = _random_case(1, 10, 880, seed=6)
    c = int(label[0])
    a, b = [k for k in range(10) if k != c][2:4]
    J[0, b] = J[0, a]
    out[0, [a, b]] = out[0, c] - 1e-3  # by far the nearest two
    got = _step(J, out, label, x)
    assert got[3][0] == 1 and got[2][0] == a
    _check_step(J, out, label, x, got, 2, "rho tie")


def test_zero_jacobian_and_zero_columns(cuda):
    J, out, label, x = _random_case(2, 10, 22050, seed=7)
    for norm in (2, np.inf):
        x_new, dist, target, state = _step(np.zeros_like(J), out, label, x, norm)
        assert state.tolist() == [1, 1] and x_new.tobytes() == x.tobytes()
        f = np.sort(np.abs(out.astype(np.float64) - out[np.arange(2), label][:, None]), axis=1)[:, 1]
        assert np.isfinite(dist).all() and (np.abs(dist - f / D.TOL) <= 1e-6 * f / D.TOL).all()
    # all-zero columns (a ragged clip's padding) keep the bits of x, -0 included
    J[:, :, -1000:] = 0.0
    J[1, :, 300:340] = 0.0
    x[:, -1000:-500] = -0.0
    for norm in (2, np.inf):
        for layout in ("bcn", "cbn"):
            got = _step(J, out, label, x, norm, layout=layout)
            _check_step(J, out, label, x, got, norm, f"zero columns {layout} norm {norm}")
            assert got[0][:, -1000:].tobytes() == x[:, -1000:].tobytes() and got[0][1, 300:340].tobytes() == x[1, 300:340].tobytes()
            # the rest of the row does move (an entry whose step is under half a unit in its last place keeps its value)
            assert (got[0][0, :-1000] != x[0, :-1000]).mean() > 0.9


def test_non_finite_input_stays_in_its_row(cuda):
    J, out, label, x = _random_case(3, 10, 880, seed=8)
    clean = _step(J, out, label, x)
    again = _step(J, out, label, x)
    for a, b in zip(clean, again):  # two runs give the same bits
        assert a.tobytes() == b.tobytes()
    for bad in (np.nan, np.inf):
        # in the row of the class itself: every w_k carries it, no candidate is left
        Jn = J.copy()
        Jn[1, label[1], 501] = bad
        x_new, dist, target, state = _step(Jn, out, label, x)
        assert state.tolist() == [1, -1, 1] and target[1] == -1 and np.isnan(dist[1]) and x_new[1].tobytes() == x[1].tobytes()
        for r in (0, 2):
            assert x_new[r].tobytes() == clean[0][r].tobytes() and dist[r] == clean[1][r] and target[r] == clean[2][r]
        # in the nearest candidate's row: that class is never chosen, the next one is
        Jn = J.copy()
        Jn[1, clean[2][1], 3] = bad
        got = _step(Jn, out, label, x)
        mask = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        mask[1] &= ~np.uint32(1 << int(clean[2][1]))
        want = _step(J, out, label, x, allowed=mask)
        assert got[3].tolist() == [1, 1, 1] and got[2][1] != clean[2][1]
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        # in the outputs
        on = out.copy()
        on[1, (label[1] + 1) % 10] = bad
        x_new, dist, target, state = _step(J, on, label, x)
        assert state.tolist() == [1, -1, 1] and target[1] == -1 and np.isnan(dist[1]) and x_new[1].tobytes() == x[1].tobytes()
        assert x_new[0].tobytes() == clean[0][0].tobytes() and x_new[2].tobytes() == clean[0][2].tobytes()


def test_mask_and_clipping(cuda):
    J, out, label, x = _random_case(3, 10, 881, seed=9)
    for norm in (2, np.inf):
        free = _step(J, out, label, x, norm)
        mask = np.array([0xFFFFFFFF & ~(1 << int(t)) for t in free[2]], dtype=np.uint32)
        got = _step(J, out, label, x, norm, allowed=mask)
        assert (got[2] != free[2]).all() and (got[1] > free[1]).all()
        _check_step(J, out, label, x, got, norm, f"masked norm {norm}", allowed=mask)
        # a mask that leaves nothing but the class itself
        only = (np.uint32(1) << label.astype(np.uint32)).astype(np.uint32)
        x_new, dist, target, state = _step(J, out, label, x, norm, allowed=only)
        assert state.tolist() == [-1] * 3 and x_new.tobytes() == x.tobytes() and np.isnan(dist).all() and (target == -1).all()
        # clipping: the result lies in [lo, hi] and lands exactly on both
        lo, hi = -0.25, 0.5
        got = _step(J, out, label, x, norm, clip=(lo, hi))
        want = D.step(J, out, label, x, norm=norm, overshoot=OVERSHOOT, lo=np.float32(lo), hi=np.float32(hi))[0]
        assert got[0].min() == np.float32(lo) and got[0].max() == np.float32(hi)
        np.testing.assert_array_equal(got[0] == np.float32(lo), want == np.float32(lo))
        np.testing.assert_array_equal(got[0] == np.float32(hi), want == np.float32(hi))


def test_degenerate_and_invalid_shapes(cuda):
    from lipasr import _native as N
    from lipasr.attacks import deepfool_step

    # one class: nothing to move towards
    x_new, dist, target, state = _step(_random_jac(2, 1, 130, 1), np.zeros((2, 1)), [0, 0], np.ones((2, 130)))
    assert state.tolist() == [-1, -1] and (x_new == 1).all() and np.isnan(dist).all() and (target == -1).all()
    # batch == 0 and n == 0
    d, t, s = deepfool_step(torch.zeros(0, 10, 880, device="cuda"), torch.zeros(0, 10, device="cuda"),
                            torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, 880, device="cuda"))
    assert d.shape == t.shape == s.shape == (0,)
    out = np.array([[0.5, 2.0, 0.25], [3.0, 1.0, 2.5]], dtype=np.float32)
    d, t, s = deepfool_step(torch.zeros(2, 3, 0, device="cuda"), torch.as_tensor(out).cuda(),
                            torch.as_tensor(np.array([1, 0], dtype=np.int32)).cuda(), torch.zeros(2, 0, device="cuda"))
    torch.cuda.synchronize()
    assert s.tolist() == [1, 1] and t.tolist() == [0, 2]
    np.testing.assert_allclose(d.cpu().numpy(), np.array([1.5, 0.5]) / D.TOL, rtol=1e-6)
    h = N.get_handle(0)
    assert N.lib.lipasr_deepfool_step(h.h, None, 0, 0, None, None, None, 0, 10, 880, 2.0, 0.0, -np.inf, np.inf, None, None, None, None,
                                      N.stream_ptr()) == N.OK
    # 33 classes, a norm that is neither 2 nor inf, a label outside the classes
    with pytest.raises(ValueError, match="33 classes"):
        deepfool_step(torch.zeros(2, 33, 8, device="cuda"), torch.zeros(2, 33, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                      torch.zeros(2, 8, device="cuda"))
    with pytest.raises(ValueError):
        deepfool_step(torch.zeros(2, 3, 8, device="cuda"), torch.zeros(2, 3, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"),
                      torch.zeros(2, 8, device="cuda"), norm=1)
    J, out, label, x = _random_case(2, 10, 36, seed=3)
    label[0] = 10
    x_new, dist, target, state = _step(J, out, label, x)
    assert state.tolist() == [-1, 1] and x_new[0].tobytes() == x[0].tobytes()


def test_power_of_two_scaling(cuda):
    """J 2^-60 with f 2^-60: the squares (2^-120) are not fp32 numbers and tol is most of every denominator."""
    J, out, label, x = _random_case(2, 10, 880, seed=21)
    Js, outs = np.ldexp(J, -60), np.ldexp(out, -60)
    zero = np.zeros_like(x)
    for norm in (2, np.inf):
        assert _rho_gap(Js, outs, label, norm) > 1e-3
        _check_step(Js, outs, label, zero, _step(Js, outs, label, zero, norm), norm, f"2^-60 norm {norm}")
    # the ~1e-30 Jacobian of a saturated softmax next to outputs of order one
    Jt = (J.astype(np.float64) * 1e-30).astype(np.float32)
    for norm in (2, np.inf):
        _check_step(Jt, out, label, zero, _step(Jt, out, label, zero, norm), norm, f"1e-30 norm {norm}")


# =================================================================================================
# 3. the attack over features
# =================================================================================================
FEATURE_CASES = {"vd": P.vd_constrained_spec, "sr": P.sr_constrained_spec}


@pytest.fixture(scope="module", params=sorted(FEATURE_CASES))
def feat(request, cuda):
    """The oracle models with setup_params(spec, 7) and 16 rows of np.random.default_rng(3).standard_normal, rounded to float32:
    the inputs of tests/test_deepfool_cpu.py.  On them the float64 attack and the float32 attack on the CPU take the same number of
    steps on all 16 rows, in both norms (checked in ``ref``), so no other seed was needed."""
    from lipasr.attacks import TensorFlowV2Classifier

    spec = FEATURE_CASES[request.param]()
    p = R.setup_params(spec, 7)
    m = build_model(spec)
    load_params(m, p)
    n, C = spec[0].n_in, spec[-1].n_out
    x = np.random.default_rng(3).standard_normal((16, n)).astype(np.float32)
    return dict(name=request.param, spec=spec, p=p, p64=p.astype(np.float64), model=m, x=x, n=n, C=C, runs={},
                clf=TensorFlowV2Classifier(model=m, nb_classes=C, input_shape=(n,)))


def _ref(feat, norm, **kw):
    key = (norm,) + tuple(sorted(kw.items()))
    if key not in feat["runs"]:
        kw = dict(dict(overshoot=OVERSHOOT, max_iter=10), **kw)
        r64 = D.deepfool(feat["spec"], feat["p"], feat["x"], norm=norm, **kw)
        r32 = D.deepfool(feat["spec"], feat["p"], feat["x"], norm=norm, dtype=np.float32, **kw)
        np.testing.assert_array_equal(r32["iterations"], r64["iterations"])  # the precondition of comparing counts on the device
        feat["runs"][key] = r64
    return feat["runs"][key]


@pytest.mark.parametrize("norm", [2, np.inf])
def test_deepfool_over_features(feat, norm):
    from lipasr.attacks import DeepFool

    x = feat["x"]
    want = _ref(feat, norm)
    attack = DeepFool(feat["clf"], max_iter=10, norm=norm, overshoot=OVERSHOOT)
    keep = x.copy()
    adv = attack.generate(x)
    assert adv is not x and adv.dtype == np.float32 and adv.shape == x.shape and np.array_equal(x, keep)
    last = attack.last
    found, want_found = D.distance(adv.astype(np.float64) - x, norm), D.distance(want["x_adv"] - x, norm)
    rel = np.abs(found - want_found) / want_found
    print(f"{feat['name']} norm {norm}: iterations {last['iterations'].tolist()} (float64 {want['iterations'].tolist()}); found "
          f"{found.min():.4e} .. {found.max():.4e}, worst relative deviation from the float64 attack {rel.max():.2e}; "
          f"found / linear {(found / last['first_dist']).min():.3f} .. {(found / last['first_dist']).max():.3f}")
    assert last["flipped"].all() and last["flipped"].dtype == bool
    fresh = feat["clf"].predict(adv).argmax(axis=1) != feat["clf"].predict(x).argmax(axis=1)
    np.testing.assert_array_equal(last["flipped"], fresh)
    np.testing.assert_array_equal(last["iterations"], want["iterations"])
    np.testing.assert_array_equal(last["target"], want["target"])
    assert (rel <= 1e-3).all()
    assert (np.abs(last["first_dist"] - want["first_dist"]) <= 1e-3 * want["first_dist"]).all()
    # the device entry point: a new tensor, the same bits
    xt = dev(x)
    at = attack.generate_device(xt)
    assert at.data_ptr() != xt.data_ptr() and np.array_equal(xt.cpu().numpy(), x) and np.array_equal(at.cpu().numpy(), adv)


def test_certified_radius_is_below_what_deepfool_found(feat):
    from lipasr.extract_features_construct_dataset import get_lipschitz_bound, get_robustness_radius

    r = get_robustness_radius(feat["clf"], feat["x"], norm=2, max_iter=10)
    L, want_L = get_lipschitz_bound(feat["model"]), D.lipschitz_bound(feat["spec"], feat["p64"])
    z = P.forward_infer(feat["spec"], feat["p64"], feat["x"].astype(np.float64), return_logits=True)
    want_margin = D.margin(z, z.argmax(axis=1))
    print(f"{feat['name']}: bound {L:.6e} (host float64 {want_L:.6e}); certified {r['certified'].min():.3e} .. {r['certified'].max():.3e} "
          f"linear {r['linear'].min():.3e} .. {r['linear'].max():.3e} found {r['found'].min():.3e} .. {r['found'].max():.3e}")
    assert want_L * (1 - 1e-4) <= L <= want_L * (1 + 1e-5)  # power iteration: from below, in fp32
    for k in ("margin", "certified", "linear", "found"):
        assert r[k].dtype == np.float64 and r[k].shape == (16,)
    assert (np.abs(r["margin"] - want_margin) <= 1e-4 * np.abs(z).max()).all()
    np.testing.assert_allclose(r["certified"], r["margin"] / (np.sqrt(2.0) * L), rtol=1e-12)
    assert r["flipped"].all()
    assert (r["certified"] > 0).all() and (r["certified"] <= r["found"]).all() and (r["certified"] <= r["linear"]).all()
    assert get_robustness_radius(feat["clf"], feat["x"][:2], norm=np.inf, max_iter=10)["certified"] is None


def test_nb_grads_restricts_the_targets(feat):
    from lipasr.attacks import DeepFool

    if feat["C"] != 20:  # ART's default nb_grads on ten classes: every class is a candidate, no mask
        a, b = (DeepFool(feat["clf"], max_iter=2, nb_grads=k).generate(feat["x"][:2]) for k in (10, 32))
        np.testing.assert_array_equal(a, b)
        return
    want = _ref(feat, 2, nb_grads=5)
    attack = DeepFool(feat["clf"], max_iter=10, nb_grads=5)
    adv = attack.generate(feat["x"])
    z = P.forward_infer(feat["spec"], feat["p64"], feat["x"].astype(np.float64), return_logits=True)
    top5 = np.argsort(-z, axis=1, kind="stable")[:, :5]
    assert all(t in row for t, row in zip(attack.last["target"], top5))
    np.testing.assert_array_equal(attack.last["target"], want["target"])
    np.testing.assert_array_equal(attack.last["iterations"], want["iterations"])
    # a row attacked alone gives the same bits: the candidates are the row's own
    alone = attack.generate(feat["x"][3:4])
    np.testing.assert_array_equal(alone[0], adv[3])


def test_overshoot_zero_is_arts_first_iteration(feat):
    """max_iter = 1 only: ART's step lands on the boundary, and what later iterations do there is decided by rounding.  Bound: the
    project's convention where the device is compared with a float64 graph -- 8 x the error of the same formula evaluated in
    float32 on the CPU (its worst row), plus the rounding of x_adv to fp32."""
    from lipasr.attacks import DeepFool

    x = feat["x"]
    for on_logits in (True, False):
        J, out = D.jacobian(feat["spec"], feat["p64"], x.astype(np.float64), on_logits)
        want, l_var = D.art_step(J, out, out.argmax(axis=1), x.astype(np.float64))
        J32, out32 = D.jacobian(feat["spec"], feat["p"], x, on_logits)
        want32, l32 = D.art_step(J32.astype(np.float64), out32.astype(np.float64), out32.argmax(axis=1), x.astype(np.float64))
        np.testing.assert_array_equal(l32, l_var)
        step = np.abs(want - x).max(axis=1)
        yard = (np.abs(want32 - want).max(axis=1) / step).max()
        want = x + (1.0 + 1e-6) * (want - x)
        attack = DeepFool(feat["clf"], max_iter=1, epsilon=1e-6, overshoot=0.0, on_logits=on_logits)
        adv = attack.generate(x)
        np.testing.assert_array_equal(attack.last["target"], l_var)
        np.testing.assert_array_equal(attack.last["iterations"], np.ones(16, dtype=np.int64))
        err = np.abs(adv - want).max(axis=1)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64).max(axis=1)  # x_iter and x_adv: two roundings of half of it
        print(f"{feat['name']} on_logits {on_logits}: worst error / max |step| {(err / step).max():.2e}; float32 oracle {yard:.2e}")
        assert (err <= 8 * yard * step + ulp).all()


def test_chunks_and_argument_checks(cuda, monkeypatch):
    from lipasr import extract_features_construct_dataset as E
    from lipasr.attacks import DeepFool, TensorFlowV2Classifier

    spec = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
    m = build_model(spec, max_batch=4)
    load_params(m, R.setup_params(spec, 2))
    clf = TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,))
    x = np.random.default_rng(4).standard_normal((11, 36)).astype(np.float32)
    attack = DeepFool(clf, max_iter=20, batch_size=64)
    whole = attack.generate(x)  # three chunks of the batch limit
    last = {k: v.copy() for k, v in attack.last.items()}
    assert all(v.shape == (11,) for v in last.values())
    monkeypatch.setattr(E, "JACOBIAN_CHUNK_BYTES", 3 * 4 * 5 * 36)  # three rows per chunk
    np.testing.assert_array_equal(attack.generate(x), whole)
    for k in last:
        np.testing.assert_array_equal(attack.last[k], last[k])
    assert attack.generate(x[:0]).shape == (0, 36) and attack.last["iterations"].shape == (0,)
    with pytest.raises(ValueError):
        attack.generate(x, lengths=[36] * 11)
    with pytest.raises(ValueError):
        DeepFool(clf, norm=1)
    with pytest.raises(ValueError):
        attack.generate(x[:, :35])


# =================================================================================================
# 4. the attack over audio
# =================================================================================================
L = 44
RAGGED = [16000, 9000, 37]


def _mean_features(clips, kw):
    with torch.no_grad():
        return np.stack([G.features(torch.as_tensor(c.astype(np.float64)), **kw).numpy() for c in clips]).mean(axis=0)


def ragged_clips():
    """[3, 16000] float32 at 16 kHz: the chirp, 9000 samples of the voiced clip and 37 of the gated chirp, zero behind each."""
    w = np.zeros((3, 16000), dtype=np.float32)
    w[0] = G.parity_clips(16000)[0]
    w[1, :9000] = G.parity_clips(9000)[2]
    w[2, :37] = G.parity_clips(37)[3]
    return w


FULL_RUN_SEED = 8


def _audio_case(name, cuda):
    """-> dict(clf, rows (device), lt, per_row [(numpy row, n_clip)], kw, spec, p, mean, scale).  "ragged_22k_full" is "ragged_22k"
    with the classifier's parameters from setup_params(spec, FULL_RUN_SEED)."""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(11)
    if name == "short":
        from lipasr.speaker_recognition import waveform_classifier

        spec = P.sr_unconstrained_spec()
        p = R.setup_params(spec, 3)
        m = build_model(spec, max_batch=8)
        load_params(m, p)
        w = G.short_parity_clips(441, 220, 22050)[:2]
        kw = dict(n_fft=441, hop=220, utterance_length=101, domain="22k")
        mean, scale = _mean_features(G.short_parity_clips(441, 220, 22050), kw), rng.uniform(0.5, 2.0, 2020)
        clf = waveform_classifier(m, mean, scale, batch_max=4)
        return dict(clf=clf, rows=torch.as_tensor(w).to(cuda), lt=None, per_row=[(r, None) for r in w], kw=kw, spec=spec, p=p, mean=mean,
                    scale=scale)
    spec = P.vd_unconstrained_spec()
    p = R.setup_params(spec, FULL_RUN_SEED if name == "ragged_22k_full" else 3)
    m = build_model(spec, max_batch=8)
    load_params(m, p)
    ex = MfccExtractor(16000, 16000, batch_max=4)
    clips16 = G.parity_clips(16000)
    if name.startswith("ragged_22k"):
        domain, w, lens = "22k", ragged_clips(), np.array(RAGGED, dtype=np.int32)
    else:
        domain, w, lens = "input", clips16[1:2], None
    wt = torch.as_tensor(w).to(cuda).contiguous()
    lt = None if lens is None else torch.as_tensor(lens).to(cuda)
    rows = ex.resample(wt, n_valid=lt) if domain == "22k" else wt
    rows_np = rows.cpu().numpy()
    clip = lambda n: int(np.ceil(n * 22050.0 / 16000.0)) if domain == "22k" else int(n)
    per_row = [(rows_np[i], None if lens is None else clip(lens[i])) for i in range(len(w))]
    kw = dict(sr_in=16000, utterance_length=L, domain=domain)
    mean, scale = _mean_features(clips16, dict(sr_in=16000, utterance_length=L, domain="input")), rng.uniform(0.5, 2.0, 20 * L)
    clf = WaveformClassifier(m, 10, extractor=ex, utterance_length=L, mean=mean, scale=scale, domain=domain)
    return dict(clf=clf, rows=rows, lt=lt, per_row=per_row, kw=kw, spec=spec, p=p, mean=mean, scale=scale)


@pytest.fixture(scope="module")
def audio(cuda):
    cases = {}
    yield lambda name: cases.setdefault(name, _audio_case(name, cuda))
    for c in cases.values():
        c["clf"].extractor.close()


@pytest.mark.parametrize("name", ["ragged_22k", "input", "short"])
def test_one_iteration_over_audio(audio, cuda, name):
    """One iteration (max_iter = 1, epsilon = 0: the kernel's own result) per row against the float64 graph: the same target, and
    x_adv - x within 8 x the error of the step the same graph gives in float32 on the CPU (both rounded to fp32 as x_adv is)."""
    from lipasr.attacks import DeepFool

    case = audio(name)
    clf, rows, lt = case["clf"], case["rows"], case["lt"]
    lo, hi = clf.clip_values
    attack = DeepFool(clf, max_iter=1, epsilon=0.0, overshoot=OVERSHOOT)
    keep = rows.clone()
    adv = attack.generate_device(rows, lengths=lt)
    assert torch.equal(rows, keep) and adv.shape == rows.shape
    got = adv.cpu().numpy()
    assert got.min() >= lo and got.max() <= hi and np.isfinite(got).all()
    yard, errs = [], []
    for b, (row, n_clip) in enumerate(case["per_row"]):
        steps = {}
        for dtype in (torch.float64, torch.float32):
            J, z = D.audio_graph(case["spec"], case["p"].astype(np.float64) if dtype == torch.float64 else case["p"], row, case["mean"],
                                 case["scale"], dtype=dtype, n_clip=n_clip, **case["kw"])
            x_new, _, dist, target, state = D.step(J[None], z[None], [int(z.argmax())], row[None], norm=2, overshoot=OVERSHOOT, lo=lo, hi=hi)
            steps[dtype] = (x_new[0].astype(np.float32).astype(np.float64) - row, int(target[0]), float(dist[0]))
        want, want_t, want_d = steps[torch.float64]
        assert attack.last["target"][b] == want_t and attack.last["iterations"][b] == 1
        if n_clip is not None:  # the padding is bit-identical
            assert got[b, n_clip:].tobytes() == row[n_clip:].tobytes() and not want[n_clip:].any()
        assert np.abs(want).max() > 0
        yard.append(G.errs(steps[torch.float32][0], want) + (abs(steps[torch.float32][2] - want_d) / want_d,))
        errs.append(G.errs(got[b].astype(np.float64) - row, want) + (abs(attack.last["first_dist"][b] - want_d) / want_d,))
        print(f"audio {name} row {b}: target {want_t} dist {want_d:.4e} max |step| {np.abs(want).max():.3e}; device inf {errs[-1][0]:.3e} two "
              f"{errs[-1][1]:.3e} dist {errs[-1][2]:.3e}; float32 oracle inf {yard[-1][0]:.3e} two {yard[-1][1]:.3e} dist {yard[-1][2]:.3e}")
    y = [max(v[i] for v in yard) for i in range(3)]
    # dist is ONE number per row, and the float32 oracle's error of it can vanish by luck; ||step||_2 = (1 + overshoot) dist, so a
    # step within e of the float64 one in the 2-norm has its dist within e too: the 2-norm yardstick bounds it as well
    for e in errs:
        assert e[0] <= 8 * y[0] and e[1] <= 8 * y[1] and e[2] <= 8 * max(y[1], y[2]), (e, y)
    if name == "short":
        with pytest.raises(ValueError):
            attack.generate_device(rows, lengths=[22050, 22050])


def test_full_run_over_ragged_audio(audio, cuda):
    """max_iter = 10 on the three clips: every clip leaves its class, inside its own samples and inside clip_values.
    The classifier: with the parameters of the other audio cases, setup_params(spec, 3), the float64 attack on the CPU does not
    flip two of the three clips within 10 iterations either (the 16 000-sample chirp: its margin falls 34 -> 0.5, the log of the
    MFCC stage makes each linearisation good for a fraction of its step; the 37-sample clip: margin 17 - 21 throughout, it reaches
    20 of the 880 features and the clip box).  Seeds 0 .. 47 were run through the float64 attack and through the same attack with the
    graph in float32, both on the CPU.  Few classifiers let the 37-sample clip leave its class at all: the float64 attack flips all
    three clips with seeds 2, 4, 8, 11, 15, 27 and 41, and with the same iteration counts in float32 with 2, 8, 15, 27 and 41.
    Seed 8 is the one whose smallest step is largest (rho_l >= 1.2e-3 on every iteration of every clip; 7, 4 and 4 iterations, margins
    crossing zero at -3.4e-3, -1.7e-3 and -0.41 on logits of 65 - 110): with 15, 27 and 41 a clip comes to rest within 1e-4 of the
    boundary and its next step is 3e-6 to 1e-4 long, which the fp32 forward pass of the MFCC stage does not resolve -- measured on the
    MI355X with seed 15: the 37-sample clip took its first step as the float64 attack does and then nine steps that changed nothing
    (|x_adv - x| 4.6e-3, not flipped), the failure the per-step overshoot cures only while 0.02 rho_l is above the noise of f."""
    from lipasr.attacks import DeepFool

    case = audio("ragged_22k_full")
    clf, rows, lt = case["clf"], case["rows"], case["lt"]
    attack = DeepFool(clf, max_iter=10, overshoot=OVERSHOOT)
    adv = attack.generate_device(rows, lengths=lt)
    got, x = adv.cpu().numpy(), rows.cpu().numpy()
    print(f"ragged audio: iterations {attack.last['iterations'].tolist()} flipped {attack.last['flipped'].tolist()} "
          f"|x_adv - x|_2 {np.linalg.norm(got - x, axis=1).tolist()}")
    assert attack.last["flipped"].all()
    before = clf.predict_device(rows, logits=True, lengths=lt).argmax(dim=1)
    after = clf.predict_device(adv, logits=True, lengths=lt).argmax(dim=1)
    assert bool((before != after).all())
    for b, (_, n_clip) in enumerate(case["per_row"]):
        assert got[b, n_clip:].tobytes() == x[b, n_clip:].tobytes()
    assert got.min() >= clf.clip_values[0] and got.max() <= clf.clip_values[1]


# =================================================================================================
# 5. the read-outs
# =================================================================================================
def test_radius_readouts(cuda, tmp_path, capsys):
    from lipasr import attack_eval as V
    from lipasr.extract_features_construct_dataset import compute_mfcc_all_files, get_robustness_radius
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(24, seed=31)
    files = []
    for i in range(24):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(waves[i], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = compute_mfcc_all_files(files)
    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=8)
    load_params(m, R.setup_params(spec, 3))
    models = {"constrained": m, "unconstrained": m}
    train, val, test = feats[:8], feats[8:16], feats[16:24]
    capsys.readouterr()
    rep = V.radius_report(models, train, val, test, over="mfcc", norm=2, max_iter=10)
    out = capsys.readouterr().out
    for name in models:
        r = rep[name]
        for k in ("margin", "certified", "linear", "found"):
            assert r[k].dtype == np.float64 and r[k].shape == (8,)
        assert r["flipped"].shape == (8,) and set(r["quartiles"]) == {"certified", "linear", "found"}
        assert (r["certified"][r["flipped"]] <= r["found"][r["flipped"]]).all()
        assert r["flipped_share"] == r["flipped"].mean()
    assert "Certified radius over 8 test rows: quartiles" in out and "Distance DeepFool found over 8 test rows unconstrained: quartiles" in out
    assert "Share of 8 test rows DeepFool moved to another class" in out
    assert len(V.radius_report(models, train, val, test, over="mfcc", norm=np.inf, limit=3, max_iter=4)["constrained"]["found"]) == 3
    capsys.readouterr()
    rep = V.radius_report(models, train, val, test, over="audio", test_filenames=files[16:24], norm=2, limit=4, max_iter=2)
    out = capsys.readouterr().out
    r = rep["unconstrained"]
    assert r["certified"] is None and "certified" not in r["quartiles"] and "Certified radius over 4 test files: not given" in out
    for k in ("margin", "linear", "found"):
        assert r[k].dtype == np.float64 and r[k].shape == (4,)
    assert (r["linear"] > 0).all() and (r["found"] > 0).all()
    with pytest.raises(ValueError):
        V.radius_report(models, train, val, test, over="audio")
    with pytest.raises(ValueError):
        V.radius_report(models, train, val, test, over="mel")
