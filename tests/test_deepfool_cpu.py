"""DeepFool without a GPU: the float64 oracle of tests/deepfool_ref.py on the oracle classifier (it flips the measured inputs, the
certified radius stays below what it finds, overshoot = 0 is ART's iteration), the device kernel's summation restated on the host
against plain float64 sums, and the ABI / menu plumbing."""
import math

import numpy as np
import pytest

import deepfool_ref as D
import local_lip_ref as R
from oracle import mlp_ref as P

SPECS = {"vd": (P.vd_constrained_spec, 10, 880), "sr": (P.sr_constrained_spec, 20, 2020)}


@pytest.fixture(scope="module", params=sorted(SPECS))
def case(request):
    make, C_, n = SPECS[request.param]
    spec = make()
    p = R.setup_params(spec, 7)
    x = np.random.default_rng(3).standard_normal((16, n))
    return dict(name=request.param, spec=spec, p=p, p64=p.astype(np.float64), x=x, C=C_, n=n, runs={})


def _run(case, norm, on_logits):
    key = (norm, on_logits)
    if key not in case["runs"]:
        case["runs"][key] = D.deepfool(case["spec"], case["p"], case["x"], norm=norm, overshoot=0.02, on_logits=on_logits, max_iter=10)
    return case["runs"][key]


@pytest.mark.parametrize("on_logits", [True, False])
@pytest.mark.parametrize("norm", [2, np.inf])
def test_flips_the_measured_inputs(case, norm, on_logits):
    """16 rows of np.random.default_rng(3).standard_normal on the oracle models with setup_params(spec, 7), overshoot 0.02: every
    row leaves its class within 10 iterations (measured: at most 6 for 880 -> 10, at most 3 for 2020 -> 20), and what was found is
    between 1 and 2.1 times the distance to the first linearised boundary."""
    r = _run(case, norm, on_logits)
    found = D.distance(r["x_adv"] - case["x"], norm)
    ratio = found / r["first_dist"]
    print(f"{case['name']} norm {norm} on_logits {on_logits}: iterations {r['iterations'].tolist()} found / linear "
          f"{ratio.min():.3f} .. {ratio.max():.3f}")
    assert r["flipped"].all()
    assert r["iterations"].max() <= 10 and r["iterations"].min() >= 1
    assert (r["target"] != r["label"]).all() and (r["target"] >= 0).all()


def test_certified_radius_is_below_what_deepfool_found(case):
    """margin / (sqrt(2) L) <= ||x_adv - x||_2 on every row: a theorem when L bounds the Lipschitz constant of the logits."""
    r = _run(case, 2, True)
    z = P.forward_infer(case["spec"], case["p64"], case["x"], return_logits=True)
    L = D.lipschitz_bound(case["spec"], case["p64"])
    certified = D.margin(z, r["label"]) / (math.sqrt(2.0) * L)
    found = D.distance(r["x_adv"] - case["x"], 2)
    print(f"{case['name']}: L {L:.4e}; certified {certified.min():.3e} .. {certified.max():.3e}, linear {r['first_dist'].min():.3e} .. "
          f"{r['first_dist'].max():.3e}, found {found.min():.3e} .. {found.max():.3e}")
    assert (certified > 0).all()
    assert (certified <= found).all()
    assert (certified <= r["first_dist"]).all()  # the linearisation is exact up to the first ReLU boundary: the same theorem


def _random_jac(B, C_, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, C_, n)) * rng.uniform(0.2, 2.0, (B, C_, 1))).astype(np.float32)


def _random_out(B, C_, seed):
    rng = np.random.default_rng(seed + 1000)
    out = rng.standard_normal((B, C_)).astype(np.float32)
    return out, out.argmax(axis=1).astype(np.int32)


@pytest.mark.parametrize("shape", [(10, 880), (20, 2020), (10, 22050)], ids=lambda s: "x".join(map(str, s)))
def test_lane_serial_sums_reproduce_float64(shape):
    """The kernel's summation before it runs on a device: fp64 differences and squares, 256 lane-serial partial sums, a butterfly
    per wave and the waves in order, with 4-byte and with 16-byte loads -- against NumPy's pairwise float64 sums.  Also for J and
    f scaled by 2^-60, where the squares (2^-120) are not fp32 numbers and tol dominates the denominators.  Same l; r within 1e-6
    relative (measured: ~1e-15, the sums are fp64 on both sides; the bound is the issue's)."""
    C_, n = shape
    J = _random_jac(2, C_, n, seed=C_ + n)
    out, label = _random_out(2, C_, seed=n)
    x = np.zeros((2, n))
    worst = 0.0
    for k in (0, -60):
        Jk, ok = np.ldexp(J, k), np.ldexp(out, k)
        for norm in (2, np.inf):
            _, r, dist, target, state = D.step(Jk, ok, label, x, norm=norm)
            assert (state == 1).all()
            for vec in (1, 4):
                if n % vec:
                    continue
                _, r2, dist2, target2, state2 = D.step_lane_f64(Jk, ok, label, x, vec=vec, norm=norm)
                np.testing.assert_array_equal(target2, target)
                np.testing.assert_array_equal(state2, state)
                err = max(np.abs(r2 - r).max() / np.abs(r).max(), (np.abs(dist2 - dist) / dist).max())
                worst = max(worst, err)
    print(f"{shape}: worst relative deviation of the lane-serial step from the float64 one {worst:.2e}")
    assert worst <= 1e-6


def test_overshoot_zero_is_arts_iteration(case):
    """One iteration with overshoot = 0 is the update of ART's loop (deepfool_ref.art_step: its array expressions), and the
    attack's result after max_iter = 1 is x + (1 + epsilon) (x_iter - x)."""
    spec, p64, x = case["spec"], case["p64"], case["x"][:4]
    for on_logits in (True, False):
        J, out = D.jacobian(spec, p64, x, on_logits)
        label = out.argmax(axis=1)
        x_new, r, dist, target, state = D.step(J, out, label, x, norm=2, overshoot=0.0)
        want, l_var = D.art_step(J, out, label, x.copy())
        np.testing.assert_array_equal(target, l_var)
        assert np.abs(x_new - want).max() <= 1e-13 * np.abs(want).max()
        res = D.deepfool(spec, p64, x, norm=2, overshoot=0.0, on_logits=on_logits, max_iter=1, epsilon=1e-6)
        np.testing.assert_allclose(res["x_adv"], x + (1.0 + 1e-6) * (want - x), rtol=0, atol=1e-13 * np.abs(want).max())
        np.testing.assert_array_equal(res["iterations"], np.ones(4, dtype=np.int64))


def test_step_conventions_of_the_oracle():
    """The edges include/lipasr.h fixes, on the float64 definition the device tests compare against."""
    J = _random_jac(1, 5, 12, seed=1).astype(np.float64)
    out = np.array([[0.1, 2.0, 0.3, 2.0, -1.0]])
    x = np.ones((1, 12))
    # an argmax tie takes the lowest index: label 3 has left its class (argmax is 1), label 1 steps
    _, _, dist, target, state = D.step(J, out, [3], x)
    assert (state[0], target[0], dist[0]) == (0, 1, 0.0)
    _, _, dist, target, state = D.step(J, out, [1], x)
    assert state[0] == 1 and target[0] == 3 and dist[0] == 0.0  # f = 0 against class 3: already on that boundary
    # a mask without any other class, one class, a NaN output: state -1
    assert D.step(J, out, [1], x, allowed=[0b00010])[4][0] == -1
    assert D.step(J[:, :1], out[:, :1], [0], x)[4][0] == -1
    bad = out.copy()
    bad[0, 4] = np.nan
    assert D.step(J, bad, [1], x)[4][0] == -1
    # zero Jacobian: dist = |f| / tol, x unchanged
    out = np.array([[0.5, 2.0, 0.25, 1.0, -1.0]])
    x_new, r, dist, target, state = D.step(np.zeros_like(J), out, [1], x)
    assert state[0] == 1 and target[0] == 3 and dist[0] == 1.0 / D.TOL and np.array_equal(x_new, x)
    # clipping lands on the limits
    x_new = D.step(J * 1e-3, out, [1], x, lo=0.999, hi=1.001)[0]
    assert x_new.min() == 0.999 and x_new.max() == 1.001


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _call(norm=2.0, classes=10, stride_b=8800, stride_c=880, overshoot=0.02, lo=-math.inf, hi=math.inf, batch=0):
    from lipasr import _native as N

    return N.lib.lipasr_deepfool_step(None, None, stride_b, stride_c, None, None, None, batch, classes, 880, norm, overshoot, lo, hi,
                                      None, None, None, None, None)


def test_abi_argument_checks_without_a_device():
    """Every argument check of lipasr_deepfool_step comes before the handle is looked at, so each is reached with a null handle:
    the message says which one refused."""
    from lipasr import _native as N

    assert N.lib.lipasr_version() >= 600 and N.has("lipasr_deepfool_step")
    assert len(N.lib.lipasr_deepfool_step.argtypes) == 19
    for kw, msg in ((dict(norm=1.5), "norm 1.5"), (dict(norm=1.0), "norm 1"), (dict(norm=-math.inf), "norm -inf"),
                    (dict(classes=33), "33 classes"), (dict(classes=0), "0 classes"), (dict(stride_b=-1), "negative stride"),
                    (dict(stride_c=-880), "negative stride"), (dict(batch=-1), "bad shape"), (dict(overshoot=-0.1), "overshoot"),
                    (dict(lo=1.0, hi=-1.0), "clip range"), (dict(lo=math.nan), "clip range"), (dict(), "null handle")):
        assert _call(**kw) == N.EINVAL, kw
        assert msg in N.last_error(), (kw, N.last_error())
    with pytest.raises(ValueError):
        N.check(_call(norm=math.inf))  # valid arguments: the null handle


def test_attack_and_readouts_are_exported():
    import inspect

    from lipasr import attack_eval as V, attacks as A
    from lipasr.extract_features_construct_dataset import get_lipschitz_bound, get_robustness_radius

    sig = inspect.signature(A.DeepFool.__init__)
    assert list(sig.parameters)[1:7] == ["classifier", "max_iter", "epsilon", "nb_grads", "batch_size", "verbose"]
    assert [sig.parameters[k].default for k in ("max_iter", "epsilon", "nb_grads", "batch_size", "verbose")] == [100, 1e-6, 10, 1, True]
    for k, d in (("norm", 2), ("overshoot", 0.02), ("on_logits", True)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d
    with pytest.raises(TypeError):
        A.DeepFool(object())
    assert callable(get_lipschitz_bound) and callable(get_robustness_radius) and callable(V.radius_report)


def test_menu_accepts_radius(tmp_path):
    """attack_eval.main takes --attack radius (argparse would exit with status 2) and goes on to load the dataset; --norm 1 is
    refused for it before anything is loaded."""
    from lipasr import attack_eval as V

    missing = str(tmp_path) + "/missing/"
    for over in ("mfcc", "audio"):
        for norm in ("2", "inf"):
            with pytest.raises(FileNotFoundError):
                V.main(["--attack", "radius", "--over", over, "--norm", norm, "--points", "8", "--standardize", "after", "--path", missing])
    with pytest.raises(FileNotFoundError):
        V.main(["--attack", "radius", "--path", missing])
    with pytest.raises(ValueError, match="radius"):
        V.main(["--attack", "radius", "--norm", "1", "--path", missing])
    with pytest.raises(SystemExit):
        V.main(["--attack", "radius", "--norm", "3", "--path", missing])
