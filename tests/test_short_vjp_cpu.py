"""The float64 oracle of the short-window MFCC backward pass (tests/mfcc_grad_ref.py, n_fft= / hop=) checked against the forward oracle and
against finite differences, the guard on the parity inputs, and the ABI of the new entry point.  No GPU."""
import numpy as np
import pytest
import torch

import mfcc_grad_ref as H
from lipasr import _native as N
from oracle import mfcc_ref as M

CASES = [(s, i) for s in H.SHORT_SHAPES for i in range(len(H.SHORT_CLIP_NAMES))]
IDS = [f"{s[0]}-{s[1]}-{s[2]}-{H.SHORT_CLIP_NAMES[i]}" for s, i in CASES]


@pytest.fixture(scope="module")
def clips():
    return {s: H.short_parity_clips(*s) for s in H.SHORT_SHAPES}


@pytest.mark.parametrize("shape,i", CASES, ids=IDS)
def test_restatement_forward_matches_the_oracle(clips, shape, i):
    """Both sides are float64: the gap is summation order (measured <= 2.1e-12 on features of magnitude up to a few hundred)."""
    n_fft, hop, n = shape
    y = clips[shape][i].astype(np.float64)
    ref = M.mfcc_22k(y, np.float64, n_fft, hop)
    T = ref.shape[1]
    assert T == 1 + n // hop
    ours = H.features(torch.as_tensor(y), utterance_length=T, domain="22k", n_fft=n_fft, hop=hop).numpy().reshape(20, T)
    err = float(np.abs(ours - ref).max())
    print(f"{shape} {H.SHORT_CLIP_NAMES[i]}: max |restatement - oracle| = {err:.3e} (max |feature| {np.abs(ref).max():.1f})")
    assert err <= 1e-9
    # fix_frames: a shorter and a longer utterance_length
    for L in (T - 3, T + 2):
        got = H.features(torch.as_tensor(y), utterance_length=L, domain="22k", n_fft=n_fft, hop=hop).numpy().reshape(20, L)
        assert np.abs(got - M.fix_frames(ref, L)).max() <= 1e-9


@pytest.mark.parametrize("shape,i", CASES, ids=IDS)
def test_parity_inputs_keep_clear_of_the_floor_and_of_ties(clips, shape, i):
    """max(db, thr) and max over the clip are not differentiable at ties: every parity clip, at every gain a batch uses it at, must
    stay 1e-2 dB away from both -- over all dB elements, the empty mel bands pinned at -100 dB among them."""
    n_fft, hop, _ = shape
    for g in H.SHORT_GAINS:
        to_floor, top_gap, floored = H.guard_margins((np.float32(g) * clips[shape][i]).astype(np.float32), n_fft, hop)
        print(f"{shape} {H.SHORT_CLIP_NAMES[i]} gain {g}: closest element to the floor {to_floor:.3e} dB, top gap {top_gap:.3e} dB, {floored} floored")
        assert to_floor >= 1e-2
        assert top_gap >= 1e-2


def test_the_441_clips_cover_both_branches_of_the_floor(clips):
    """At least one 441/220 clip has floored elements (their sum is handed to the clip maximum), at least one has none."""
    floored = [H.guard_margins(c, 441, 220)[2] for c in clips[(441, 220, 22050)]]
    assert max(floored) > 0 and min(floored) == 0, floored
    y = M.librosa_load_resample(H.input_rate_clips()[0], H.INPUT_RATE)
    assert len(y) == 22050
    for c in H.input_rate_clips():
        to_floor, top_gap, _ = H.guard_margins(M.librosa_load_resample(c, H.INPUT_RATE), 441, 220)
        assert to_floor >= 1e-2 and top_gap >= 1e-2


@pytest.mark.parametrize("shape,i", CASES, ids=IDS)
def test_autograd_gradient_matches_central_differences(clips, shape, i):
    n_fft, hop, n = shape
    L = 1 + n // hop
    rng = np.random.default_rng(1000 * n_fft + i)
    x = clips[shape][i].astype(np.float64)
    g_feat = rng.standard_normal(20 * L)
    d = rng.standard_normal(n)
    d /= np.linalg.norm(d)  # unit direction: `step` below is the Euclidean length of the perturbation
    an = float(H.vjp(x, g_feat, utterance_length=L, domain="22k", n_fft=n_fft, hop=hop) @ d)
    gt = torch.as_tensor(g_feat)

    def loss(v):
        with torch.no_grad():
            return float((H.features(torch.as_tensor(v), utterance_length=L, domain="22k", n_fft=n_fft, hop=hop) * gt).sum())

    for step in (1e-6, 1e-7):
        fd = (loss(x + step * d) - loss(x - step * d)) / (2 * step)
        rel = abs(fd - an) / abs(an)
        print(f"{shape} {H.SHORT_CLIP_NAMES[i]} step {step:g}: autograd {an:.10e} central difference {fd:.10e} rel {rel:.2e}")
        assert rel <= 1e-5


def test_library_exports_and_binds_the_short_window_backward_entry_point():
    assert N.lib.lipasr_version() >= 550
    name = "lipasr_mfcc_plan_vjp_short"
    assert hasattr(N.lib, name) and name in N.PROTOTYPES
    # argument validation needs no GPU: a null plan is rejected before anything touches the device
    assert N.lib.lipasr_mfcc_plan_vjp_short(None, None, 0, 1, 101, None, None, None, 0, None) == N.EINVAL
    assert name in N.last_error()


def test_keyword_validation():
    from lipasr import speaker_recognition as S

    for kind in ("jsma", "l2", "linf"):
        with pytest.raises(ValueError):
            S.white_box_audio_sweep({}, None, None, ["a.wav"], [0], kind=kind)
    with pytest.raises(TypeError):
        S.waveform_classifier(object())
