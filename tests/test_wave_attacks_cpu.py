"""The float64 oracle of the MFCC backward pass (tests/mfcc_grad_ref.py) checked against the forward oracle and against finite
differences, the guard on the parity inputs, and the ABI of the new entry points.  No GPU."""
import numpy as np
import pytest
import torch

import mfcc_grad_ref as G
from lipasr import _native as N
from oracle import mfcc_ref as M

CASES = [(n, i) for n in G.LENGTHS for i in range(len(G.CLIP_NAMES))]
IDS = [f"{G.CLIP_NAMES[i]}-{n}" for n, i in CASES]


@pytest.fixture(scope="module")
def clips():
    return {n: G.parity_clips(n) for n in G.LENGTHS}


@pytest.mark.parametrize("n,i", CASES, ids=IDS)
def test_restatement_forward_matches_the_oracle(clips, n, i):
    """The gap is the oracle's own float32 rounding (measured 6e-6 .. 9e-5 on features of magnitude up to a few hundred)."""
    x = clips[n][i]
    ours = G.features(torch.as_tensor(x.astype(np.float64))).numpy()
    ref = M.extract_features_wave(x, 16000).reshape(-1).astype(np.float64)
    err = float(np.abs(ours - ref).max())
    print(f"{G.CLIP_NAMES[i]} n={n}: max |restatement - oracle| = {err:.3e} (max |feature| {np.abs(ref).max():.1f})")
    assert err <= 5e-4


@pytest.mark.parametrize("n,i", CASES, ids=IDS)
def test_parity_inputs_keep_clear_of_the_floor_and_of_ties(clips, n, i):
    """max(db, thr) and max over the clip are not differentiable at ties: every parity clip must stay 1e-2 dB away from both."""
    y = M.librosa_load_resample(clips[n][i], 16000)
    to_floor, top_gap = G.guard_margins(y)[:2]
    print(f"{G.CLIP_NAMES[i]} n={n}: closest element to the floor {to_floor:.3e} dB, top gap {top_gap:.3e} dB")
    assert to_floor >= 1e-2
    assert top_gap >= 1e-2


def test_stationary_clips_fail_the_guard():
    """Why tests/golden/inputs.py's tone and clipped square are no parity inputs."""
    from golden.inputs import test_clips as golden_clips

    w = golden_clips()
    for i in (0, 3):
        assert G.guard_margins(M.librosa_load_resample(w[i], 16000))[1] < 1e-2


@pytest.mark.parametrize("domain", ["input", "22k"])
@pytest.mark.parametrize("n,i", CASES, ids=IDS)
def test_autograd_gradient_matches_central_differences(clips, n, i, domain):
    rng = np.random.default_rng(1000 * n + i)
    x = clips[n][i].astype(np.float64)
    if domain == "22k":
        x = M.librosa_load_resample(x.astype(np.float32), 16000).astype(np.float64)
    g_feat = rng.standard_normal(20 * 44)
    d = rng.standard_normal(x.shape[0])
    d /= np.linalg.norm(d)  # unit direction: `step` below is the Euclidean length of the perturbation
    grad = G.vjp(x, g_feat, domain=domain)
    an = float(grad @ d)
    gt = torch.as_tensor(g_feat)

    def loss(v):
        with torch.no_grad():
            return float((G.features(torch.as_tensor(v), domain=domain) * gt).sum())

    for step in (1e-6, 1e-7):
        fd = (loss(x + step * d) - loss(x - step * d)) / (2 * step)
        rel = abs(fd - an) / abs(an)
        print(f"{G.CLIP_NAMES[i]} n={n} {domain} step {step:g}: autograd {an:.10e} central difference {fd:.10e} rel {rel:.2e}")
        assert rel <= 1e-5


def test_library_exports_and_binds_the_backward_entry_points():
    assert N.lib.lipasr_version() >= 520
    for name in ("lipasr_mfcc_plan_vjp", "lipasr_mfcc_plan_resample_vjp"):
        assert hasattr(N.lib, name) and name in N.PROTOTYPES
    # argument validation needs no GPU: a null plan is rejected before anything touches the device
    assert N.lib.lipasr_mfcc_plan_vjp(None, None, 0, 1, 44, None, None, None, 0, None) == N.EINVAL
    assert "lipasr_mfcc_plan_vjp" in N.last_error()
    assert N.lib.lipasr_mfcc_plan_resample_vjp(None, None, 1, None, None) == N.EINVAL


def test_keyword_validation():
    from lipasr import attack_eval as E, attacks as AT

    with pytest.raises(TypeError):
        AT.WaveformClassifier(model=object(), nb_classes=10)
    with pytest.raises(TypeError):
        AT.FastGradientMethod(estimator=object(), eps=0.01)
    for kind in ("jsma", "l2", "linf"):
        with pytest.raises(ValueError):
            E.white_box_sweep({}, None, None, None, None, kind=kind, over="audio", test_filenames=["a.wav"])
    with pytest.raises(ValueError):
        E.white_box_sweep({}, None, None, None, None, kind="fgsm", over="audio")  # no file names
    with pytest.raises(ValueError):
        E.white_box_sweep({}, None, None, None, None, kind="fgsm", over="video")


def test_sweeps_and_reports_refuse_bad_arguments_in_one_order():
    """The preparation the sweeps and read-outs share: over="audio" without file names, then ``domain``, then ``over`` -- each
    refused before anything touches a device or the data (there is no device here and the data are None).  white_box_sweep looks
    at ``kind`` before all of them."""
    from lipasr import attack_eval as E

    calls = {"lipschitz_report": lambda **kw: E.lipschitz_report({}, None, None, None, **kw),
             "radius_report": lambda **kw: E.radius_report({}, None, None, None, **kw),
             "smooth_report": lambda **kw: E.smooth_report({}, None, None, None, None, 0.1, **kw),
             "genetic_sweep": lambda **kw: E.genetic_sweep({}, None, None, None, None, **kw),
             "white_box_sweep": lambda **kw: E.white_box_sweep({}, None, None, None, None, kind="fgsm", **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="test_filenames"):
            call(over="audio", domain="44k")  # no file names AND a bad domain: the file names come first
        with pytest.raises(ValueError, match="domain="):
            call(over="audio", test_filenames=["a.wav"], domain="44k")
        with pytest.raises(ValueError, match="over must be"):
            call(over="video", domain="44k")
        with pytest.raises(ValueError, match="over must be"):
            call(over="video", test_filenames=["a.wav"])
    with pytest.raises(ValueError, match="kind"):
        E.white_box_sweep({}, None, None, None, None, kind="jsma", over="audio", domain="44k")  # kind before file names and domain
    with pytest.raises(ValueError, match="unknown white-box attack"):
        E.white_box_sweep({}, None, None, None, None, kind="deepfool", over="video")  # and before over
    with pytest.raises(ValueError, match="sigma"):
        E.smooth_report({}, None, None, None, None, -1.0, over="video")  # smooth_report's own argument first
