"""The local Lipschitz read-out without a GPU: the oracle of tests/local_lip_ref.py against a finite difference, the device
kernel's summation scheme restated on the host against float64, and the ABI / menu plumbing."""
import numpy as np
import pytest

import local_lip_ref as R
from oracle import mlp_ref as P

SPECS = {"vd": (P.vd_constrained_spec, 10, 880), "sr": (P.sr_constrained_spec, 20, 2020)}


@pytest.fixture(scope="module", params=sorted(SPECS))
def case(request):
    make, C, n = SPECS[request.param]
    spec = make()
    p64 = R.setup_params(spec, 7).astype(np.float64)
    x = np.random.default_rng(3).standard_normal((4, n))
    return dict(name=request.param, spec=spec, p64=p64, x=x, C=C, n=n, J={ol: R.jacobian(spec, p64, x, ol) for ol in (True, False)})


@pytest.mark.parametrize("on_logits", [True, False])
def test_sigma_is_the_finite_difference_along_v(case, on_logits):
    """||f(x + h v) - f(x)|| / h at h = 1e-6 in float64 reproduces sigma (measured agreement 1e-8; asserted 1e-6)."""
    spec, p64, x = case["spec"], case["p64"], case["x"]
    h = 1e-6
    f0 = R.outputs(spec, p64, x, on_logits)
    for b in range(x.shape[0]):
        J = case["J"][on_logits][b]
        assert J.shape == (case["C"], case["n"])
        sigma, u, v = R.sigma_uv(J)
        assert abs(np.linalg.norm(u) - 1) < 1e-12 and abs(np.linalg.norm(v) - 1) < 1e-12 and u[np.argmax(np.abs(u))] > 0
        np.testing.assert_allclose(J @ v, sigma * u, atol=1e-12 * sigma)
        fd = np.linalg.norm(R.outputs(spec, p64, (x[b] + h * v)[None], on_logits)[0] - f0[b]) / h
        print(f"{case['name']} on_logits {on_logits} row {b}: sigma {sigma:.9e} finite difference {fd:.9e} rel {abs(fd - sigma) / sigma:.2e}")
        assert abs(fd - sigma) <= 1e-6 * sigma
    if not on_logits:  # probabilities sum to one: their gradients cancel
        assert np.abs(case["J"][False].sum(axis=1)).max() <= 1e-14 * np.abs(case["J"][False]).max() * case["C"]


def test_float32_lane_serial_gram_reproduces_float64_sigma(case):
    """The kernel's algorithm before it runs on a device: a float32 Gram matrix from 256 lane-serial partial sums plus a tree gives
    the float64 sigma (measured <= 4.4e-8 on (10, 880) and (20, 2020); asserted 1e-6), also for a Jacobian near fp32's floor."""
    worst = 0.0
    for ol in (True, False):
        for J in case["J"][ol]:
            j32 = J.astype(np.float32)
            want = R.sigma_uv(j32)[0]
            for k in (0, -100):
                got = R.gram_sigma_f32(np.ldexp(j32, k))
                worst = max(worst, abs(got - np.ldexp(want, k)) / np.ldexp(want, k))
    print(f"{case['name']}: worst relative error of the float32 lane-serial Gram sigma {worst:.2e}")
    assert worst <= 1e-6


def test_gather_resampler_is_the_oracle_resampler():
    """local_lip_ref.resample (one gather) against mfcc_grad_ref.resample (one indexing per phase): forward and adjoint."""
    import torch

    import mfcc_grad_ref as G

    for sr, n in ((16000, 3001), (8000, 1500), (22050, 100)):
        x = torch.as_tensor(np.random.default_rng(n).standard_normal(n) * 0.3).requires_grad_(True)
        a, b = R.resample(x, sr), G.resample(x, sr)
        assert a.shape == b.shape
        assert float((a - b).detach().abs().max()) <= 1e-14
        g = torch.as_tensor(np.random.default_rng(1).standard_normal(a.shape[0]))
        (ga,), (gb,) = torch.autograd.grad(a, x, grad_outputs=g), torch.autograd.grad(b, x, grad_outputs=g)
        assert float((ga - gb).abs().max()) <= 1e-13 * float(gb.abs().max())


def test_audio_jacobian_is_the_features_vjp():
    """A class row of audio_jacobian against mfcc_grad_ref.vjp with the classifier's feature gradient as cotangent."""
    import mfcc_grad_ref as G

    spec = P.vd_unconstrained_spec()
    p = R.setup_params(spec, 3)
    p64 = p.astype(np.float64)
    x = G.parity_clips(12000)[0][:4000].astype(np.float64)
    rng = np.random.default_rng(2)
    kw = dict(sr_in=16000, utterance_length=44, domain="input")
    mean, scale = rng.standard_normal(880), rng.uniform(0.5, 2.0, 880)
    J = R.audio_jacobian(spec, p64, x, mean, scale, **kw)
    import torch

    with torch.no_grad():
        f = G.features(torch.as_tensor(x), mean=mean, scale=scale, **kw).numpy()
    Jf = R.jacobian(spec, p64, f[None], True)[0]
    for c in (0, 7):
        want = G.vjp(x, Jf[c], scale=scale, **kw)
        assert np.abs(J[c] - want).max() <= 1e-10 * np.abs(want).max()
    Jr = R.audio_jacobian(spec, p64, np.concatenate([x, np.ones(100)]), mean, scale, n_clip=4000, **kw)
    assert not Jr[:, 4000:].any() and np.array_equal(Jr[:, :4000], J)


def test_sigma_uv_conventions():
    assert R.sigma_uv(np.zeros((3, 5)))[0] == 0.0 and not R.sigma_uv(np.zeros((3, 5)))[1].any()
    J = np.zeros((4, 9))
    J[2, 8] = -3.0
    s, u, v = R.sigma_uv(J)
    assert s == 3.0 and u[2] == 1.0 and v[8] == -1.0 and np.count_nonzero(u) == 1 and np.count_nonzero(v) == 1


def test_abi_has_the_entry_points():
    from lipasr import _native as N

    assert N.lib.lipasr_version() >= 580
    assert N.has("lipasr_mlp_jacobian") and N.has("lipasr_jacobian_sigma")
    assert N.lib.lipasr_mlp_jacobian.argtypes is not None and len(N.lib.lipasr_mlp_jacobian.argtypes) == 11
    assert N.lib.lipasr_jacobian_sigma.argtypes is not None and len(N.lib.lipasr_jacobian_sigma.argtypes) == 11


def test_menu_accepts_lipschitz(tmp_path):
    """attack_eval.main takes --attack lipschitz (argparse would exit with status 2) and goes on to load the dataset."""
    from lipasr import attack_eval as V

    for over in ("mfcc", "audio"):
        with pytest.raises(FileNotFoundError):
            V.main(["--attack", "lipschitz", "--over", over, "--path", str(tmp_path) + "/missing/"])
    assert callable(V.lipschitz_report)


def test_lip_stats_callback_keeps_its_default():
    from lipasr.train_constraints import lip_stats_callback

    assert lip_stats_callback().probe is None
    assert lip_stats_callback(probe=np.zeros((2, 880))).probe.dtype == np.float32
