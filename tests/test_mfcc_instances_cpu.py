"""CPU companion of test_mfcc_instances_gpu.py: the bounds of the per-stage MFCC tests are decisive.

Stage B: on every clip set of the GPU cases the float32 yardstick is finite and positive on every non-silent frame, and each of three
wrong restatements of the float64 reference (a symmetric instead of the periodic Hann window, the mel bank shifted by one bin, every
frame one sample late) exceeds STAGE_B_MAX_FACTOR x the yardstick of the set's worst frame on at least one frame.  Stage C: a floor taken
over the first L frames only exceeds the derived DCT bound on the loud-last-frame clip.

One exemption, by reasoning: a clip of n_y = 2 samples [a, b] is reflected into the period-2 signal a b a b ...; a frame one sample
late is b a b a ..., whose DC term is the same sum (the periodic Hann window has equal sums over its even and its odd samples) and
whose other terms only change sign.  No clip of two samples can tell the two apart, so the 'offset' restatement is not asked of it.
"""
import numpy as np
import pytest

import mfcc_stage_ref as S
from oracle import mfcc_ref as M

# (n_fft, hop, n_y) of the stage-B cases of test_mfcc_instances_gpu.py
FFT_SETS = [(2048, 512, 2), (2048, 512, 700), (2048, 512, 2205), (2048, 512, 22528)]
DFT_SETS = [(32, 32, 200), (33, 16, 200), (64, 1, 100), (441, 220, 2205), (510, 510, 2205)]


def test_wrong_restatement_helper_restates_the_oracle():
    y = S.stage_b_clips(2205)[0]
    assert np.allclose(S.mel_power_wrong(y, "none"), S.mel_power(y, np.float64), rtol=1e-12, atol=0.0)
    assert np.allclose(S.mel_power_wrong(y[:200], "none", 33, 16), S.mel_power(y[:200], np.float64, 33, 16), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("n_fft,hop,n_y", FFT_SETS + DFT_SETS)
def test_stage_b_bound_is_decisive(n_fft, hop, n_y):
    clips = S.stage_b_clips(n_y)
    refs = [S.stage_b_reference(y, n_fft, hop) for y in clips]
    yard = np.concatenate([r[1] for r in refs])
    silent = np.concatenate([S.silent_frames(r[0]) for r in refs])
    assert np.isfinite(yard).all()
    assert (yard[~silent] > 0.0).all(), "a non-silent frame on which the float32 oracle is exact: the bound would be zero there"
    assert silent.any() and not silent.all()  # the all-zero clip; on silent frames the device is held to exactly -100 dB instead
    bound = S.STAGE_B_MAX_FACTOR * yard[~silent].max()
    assert bound < 1e-4, bound  # the yardstick is float32 rounding, nothing coarser
    for which in ("hann", "mel", "offset"):
        if which == "offset" and n_y == 2:
            continue  # see the module docstring
        worst = max(S.frame_metric(S.mel_power_wrong(y, which, n_fft, hop), r[0]).max() for y, r in zip(clips, refs))
        print(f"n_fft {n_fft} hop {hop} n_y {n_y}: bound {bound:.2e}, wrong '{which}' {worst:.2e}")
        assert worst > bound, (which, worst, bound)


def test_fused_chain_yardstick_is_positive():
    """the fused kernel's reference chain starts at the waveform: float64 resampling, float32-rounded for the yardstick"""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, 1600).astype(np.float32)
    y64 = M.librosa_load_resample(x, 16000, dtype=np.float64)
    y32 = M.librosa_load_resample(x, 16000)
    assert y64.dtype == np.float64 and y32.dtype == np.float32 and np.array_equal(y64.astype(np.float32), y32)
    P64, yard, _ = S.stage_b_reference(y32, y64=y64)
    assert P64.shape == (5, 128) and np.isfinite(yard).all() and (yard > 0.0).all()


@pytest.mark.parametrize("L", [1, 3])
def test_stage_c_bound_is_decisive(L):
    """dct_kernel's floor comes from the maximum over ALL frames of the clip.  On the loud-last-frame clip a floor taken over the L
    output frames only is far outside the derived bound."""
    y = S.loud_last_clip()
    db = (10.0 * np.log10(S.mel_power(y, np.float32))).astype(np.float32)
    fmax = db.max(axis=1)
    assert fmax.argmax() == 4 and fmax[4] - fmax[:3].max() > 60.0
    val, bound = S.dct_reference(db, fmax, 5, L)
    wrong, _ = S.dct_reference(db, fmax, 5, L, floor_frames=L)
    assert (bound > 0.0).all() and bound.max() < 1e-2
    assert np.abs(wrong - val).max() > 1000.0 * bound.max(), (np.abs(wrong - val).max(), bound.max())
