"""Per-clip lengths in the MFCC backward pass, the parts that need no GPU: the ABI of the new entry points, the oracle for
clips shorter than the reflect padding (tests/mfcc_grad_ref.py) against the forward oracle, the guard on the parity
inputs, and keyword validation."""
import numpy as np
import pytest
import torch

import mfcc_grad_ref as G
from lipasr import _native as N
from oracle import mfcc_ref as M

SHORT = tuple(n for n in G.RAGGED_LENGTHS if n < 12000)  # tests/test_wave_attacks_cpu.py covers 12 000 .. 20 000
CASES = [(n, i) for n in SHORT for i in range(len(G.CLIP_NAMES))]
IDS = [f"{G.CLIP_NAMES[i]}-{n}" for n, i in CASES]


@pytest.fixture(scope="module")
def clips():
    return {n: G.parity_clips(n) for n in SHORT}


def test_library_exports_and_binds_the_ragged_entry_points():
    assert N.lib.lipasr_version() >= 530
    for name in ("lipasr_mfcc_plan_vjp_ragged", "lipasr_mfcc_plan_resample_ragged", "lipasr_mfcc_plan_from_22k_ragged"):
        assert hasattr(N.lib, name) and name in N.PROTOTYPES
    # argument validation needs no GPU: a null plan is rejected before anything touches the device
    assert N.lib.lipasr_mfcc_plan_vjp_ragged(None, None, 0, None, 0, 1, 44, None, None, None, 0, None) == N.EINVAL
    assert "lipasr_mfcc_plan_vjp_ragged" in N.last_error()
    assert N.lib.lipasr_mfcc_plan_resample_ragged(None, None, 0, None, 1, None, None) == N.EINVAL
    assert N.lib.lipasr_mfcc_plan_from_22k_ragged(None, None, None, 1, 44, None, None, None, None) == N.EINVAL


@pytest.mark.parametrize("n,i", CASES, ids=IDS)
def test_restatement_forward_matches_the_oracle_on_short_clips(clips, n, i):
    """The tolerance of tests/test_wave_attacks_cpu.py for the long clips (the oracle's own float32 rounding)."""
    x = clips[n][i]
    ours = G.features(torch.as_tensor(x.astype(np.float64))).numpy()
    ref = M.compute_mfcc_batch(x[None, :])[0].reshape(-1).astype(np.float64)
    err = float(np.abs(ours - ref).max())
    print(f"{G.CLIP_NAMES[i]} n={n}: max |restatement - oracle| = {err:.3e} (max |feature| {np.abs(ref).max():.1f})")
    assert err <= 5e-4


def test_gather_padding_is_the_reflect_pad_where_torch_has_one():
    """For a clip longer than the padding the gather is torch's reflect pad, bit for bit: the padded signal, and the dB tile through
    either (the oracle's steps after the padding, restated on torch's padded signal)."""
    x = G.parity_clips(3000)[1].astype(np.float64)
    y = torch.as_tensor(M.librosa_load_resample(x.astype(np.float32), 16000).astype(np.float64))
    yp = torch.nn.functional.pad(y[None, None, :], (M.N_FFT // 2, M.N_FFT // 2), mode="reflect")[0, 0]
    assert torch.equal(y[torch.as_tensor(np.pad(np.arange(y.shape[0]), M.N_FFT // 2, mode="reflect"))], yp)
    X = torch.fft.rfft(yp.unfold(0, M.N_FFT, M.HOP) * torch.as_tensor(M.hann_periodic()), dim=1)
    mel = (X.real ** 2 + X.imag ** 2) @ torch.as_tensor(M.mel_filterbank().astype(np.float64)).T
    assert torch.equal(G.db_22k(y), 10.0 * torch.log10(torch.clamp(mel, min=1e-10)))


@pytest.mark.parametrize("n,i", CASES, ids=IDS)
def test_parity_inputs_keep_clear_of_the_floor_and_of_ties(clips, n, i):
    """max(db, thr) and max over the clip are not differentiable at ties: every parity clip must stay 1e-2 dB away from both."""
    y = M.librosa_load_resample(clips[n][i], 16000)
    to_floor, top_gap = G.guard_margins(y)[:2]
    print(f"{G.CLIP_NAMES[i]} n={n}: closest element to the floor {to_floor:.3e} dB, top gap {top_gap:.3e} dB")
    assert to_floor >= 1e-2
    assert top_gap >= 1e-2


def test_lengths_keyword_needs_a_waveform_classifier():
    from lipasr import attacks as AT

    clf = object.__new__(AT.TensorFlowV2Classifier)  # (a real one needs a model on the device; the check comes before any use)
    x = np.zeros((2, 880), dtype=np.float32)
    for attack in (AT.FastGradientMethod(estimator=clf, eps=0.1), AT.ProjectedGradientDescent(estimator=clf, eps=0.1, max_iter=1)):
        with pytest.raises(ValueError):
            attack.generate(x, lengths=[400, 880])
        with pytest.raises(ValueError):
            attack.generate_device(x, None, lengths=[400, 880])
