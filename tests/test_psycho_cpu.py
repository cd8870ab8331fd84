"""The psychoacoustic masker without a GPU: the host tables behind lipasr_psy_table against the NumPy restatement, the error
convention of the lipasr_psy_* entry points, the restatement's own gradient against central differences, the merge rule on
hand-made lists, and the suitability of the seeded inputs the GPU tests use (tests/psycho_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import psycho_ref as R
import lipasr._native as N


def test_version_and_symbols():
    assert N.lib.lipasr_version() >= 590
    for name in ("create", "destroy", "psd", "threshold", "prepare", "loss_grad", "step", "table"):
        assert N.has(f"lipasr_psy_{name}") and hasattr(N.lib, f"lipasr_psy_{name}")


@pytest.mark.parametrize("sr", R.RATES + (48000,))
def test_tables_against_the_restatement(sr):
    ref = R.tables(sr)
    for which in range(4):
        got = N.psy_table(which, sr)
        assert got.shape == (R.K,)
        inf = np.isinf(ref[which])
        assert np.array_equal(np.isinf(got), inf) and np.all(got[inf] == ref[which][inf])
        assert np.abs(got[~inf] - ref[which][~inf]).max() <= 1e-12
    ath = N.psy_table(2, sr)
    assert np.isneginf(ath[0]) and np.isneginf(ath[1]) == (sr / 2048 < 20)  # below 20 Hz
    assert np.isneginf(ath[-1]) == (sr / 2 > 20000)


def test_error_convention_without_gpu():
    plan = N.c_h()
    assert N.lib.lipasr_psy_destroy(None) == N.EINVAL
    assert "null plan" in N.last_error()
    assert N.lib.lipasr_psy_create(None, 16000, 4096, 2, 0, None) == N.EINVAL
    assert N.lib.lipasr_psy_create(None, 0, 4096, 2, 0, C.byref(plan)) == N.EINVAL
    assert "sample_rate" in N.last_error()
    assert N.lib.lipasr_psy_create(None, 16000, 2047, 2, 0, C.byref(plan)) == N.EINVAL  # n < 2048: not one window
    assert "2048" in N.last_error()
    assert N.lib.lipasr_psy_create(None, 16000, 4096, 0, 0, C.byref(plan)) == N.EINVAL
    assert N.lib.lipasr_psy_create(None, 16000, 4096, 2, 2, C.byref(plan)) == N.EINVAL
    assert "flags" in N.last_error()
    assert N.lib.lipasr_psy_create(None, 16000, 1 << 30, 64, 0, C.byref(plan)) == N.EUNSUPPORTED
    assert N.lib.lipasr_psy_create(None, 16000, 4096, 2, 0, C.byref(plan)) == N.EINVAL  # null handle
    assert not plan.value
    assert N.lib.lipasr_psy_psd(None, None, 4096, 1, None, None, None) == N.EINVAL
    assert N.lib.lipasr_psy_threshold(None, None, 5, 1, None, None, None) == N.EINVAL
    assert N.lib.lipasr_psy_prepare(None, None, 4096, 1, None, None, None) == N.EINVAL
    assert N.lib.lipasr_psy_loss_grad(None, None, 4096, 1, None, None, None, None, None) == N.EINVAL
    assert N.lib.lipasr_psy_step(None, None, None, None, None, None, None, None, 4096, 1, 0.1, 1, -1.0, 1.0, None) == N.EINVAL
    assert N.lib.lipasr_psy_table(4, 16000, None, 0) == N.EINVAL
    assert N.lib.lipasr_psy_table(0, 0, None, 0) == N.EINVAL
    small = (C.c_double * 4)()
    assert N.lib.lipasr_psy_table(1, 16000, small, 4) == N.EINVAL
    assert N.lib.lipasr_psy_table(1, 16000, None, 0) == R.K
    with pytest.raises(ValueError):
        N.check(N.lib.lipasr_psy_destroy(None))


def test_python_surface_rejects_other_framings_and_short_clips():
    from lipasr.psychoacoustic import PsychoacousticMasker

    for kw in (dict(window_size=1024), dict(hop_size=256), dict(window_size=441, hop_size=220), dict(bark_by="hz"), dict(sample_rate=0)):
        with pytest.raises(ValueError):
            PsychoacousticMasker(**kw)
    m = PsychoacousticMasker(sample_rate=22050)
    assert (m.window_size, m.hop_size, m.sample_rate, m.bark_by) == (2048, 512, 22050, "bin")
    np.testing.assert_array_equal(m.fft_frequencies, N.psy_table(0, 22050))
    np.testing.assert_array_equal(m.bark, N.psy_table(1, 22050))
    np.testing.assert_array_equal(m.absolute_threshold_hearing, N.psy_table(2, 22050))
    with pytest.raises(ValueError):
        m.n_frames(2047)
    with pytest.raises(ValueError):
        R.n_frames(2047)
    assert [m.n_frames(n) for n in R.SIZES] == [1, 2, 3, 9, 40] == [R.n_frames(n) for n in R.SIZES]


def _clip_theta(n, sr, seed=0):
    x = R.clips(n, sr, 1, seed)[0].astype(np.float64)
    p, mx = R.psd(x)
    return R.threshold(p, sr)[0], mx


@pytest.mark.parametrize("n", R.SIZES)
def test_reference_gradient_against_central_differences(n):
    theta, mx = _clip_theta(n, 22050)
    rng = np.random.default_rng(n)
    delta = 1e-2 * rng.standard_normal(n)
    v = rng.standard_normal(n)
    loss, g = R.loss_grad(delta, theta, mx)
    assert loss > 0
    h = 1e-7
    quot = (R.loss_grad(delta + h * v, theta, mx)[0] - R.loss_grad(delta - h * v, theta, mx)[0]) / (2 * h)
    print(f"n={n}: <g, v> {g @ v:.10e} difference quotient {quot:.10e}")
    assert abs(g @ v - quot) <= 1e-6 * abs(quot)
    # samples past the last frame: exactly zero
    last = R.HOP * (R.n_frames(n) - 1) + R.N
    assert np.all(g[last:] == 0) and (last == n or n == 6244 or n == 22050)
    assert np.abs(g[:last]).max() > 0


def test_merge_rule_on_hand_made_lists():
    _, bark, _, _ = R.tables(16000)
    near = [100, 101, 102, 103]                      # within half a Bark of each other (bark by bin)
    assert bark[103] - bark[100] < 0.5
    far = [100, 200, 300, 400]
    assert np.all(np.diff(bark[far]) >= 0.5)
    # ascending levels: each i beats i_prev, which moves on by one
    keep, _ = R.merge(np.array([50.0, 60.0, 70.0, 80.0]), near, bark)
    assert keep.tolist() == [False, False, False, True]
    # a tie drops i, not i_prev
    keep, margin = R.merge(np.array([60.0, 60.0, 50.0, 60.0]), near, bark)
    assert keep.tolist() == [True, False, False, False] and margin == 0.0
    # far apart: nothing merges, whatever the levels
    keep, margin = R.merge(np.array([80.0, 50.0, 70.0, 60.0]), far, bark)
    assert keep.all() and margin == np.inf
    # the i_prev + 1 step: entry 0 loses to entry 2 and i_prev becomes 1 -- an entry that was ALREADY dropped (by entry 0) -- so the
    # far-away entry 3 is then compared with entry 1's bin, and a literal restatement keeps ART's order of events
    bins = [100, 101, 102, 400]
    keep, _ = R.merge(np.array([60.0, 50.0, 70.0, 40.0]), bins, bark)
    assert keep.tolist() == [False, False, True, True]
    # ... and where i_prev + 1 lands on a dropped entry that is weaker than a later neighbour, it is "dropped" again and i_prev
    # moves on to the entry it should have been all along
    bins = [100, 101, 102, 103]
    keep, _ = R.merge(np.array([60.0, 50.0, 70.0, 65.0]), bins, bark)
    #   i=1: 60 vs 50 -> drop 1.  i=2: 60 < 70 -> drop 0, i_prev = 1.  i=3: level[1] = 50 < 65 -> drop 1 (again), i_prev = 2:
    #   entries 2 (70) and 3 (65) are never compared and BOTH survive within half a Bark
    assert keep.tolist() == [False, False, True, True]
    # bark by position: the table is read at the list position, 0 .. 3, all within half a Bark whatever the bins
    assert bark[3] - bark[0] < 0.5
    keep, _ = R.merge(np.array([80.0, 50.0, 70.0, 60.0]), far, bark, "position")
    assert keep.tolist() == [True, False, False, False]
    keep, _ = R.merge(np.array([80.0, 50.0, 70.0, 60.0]), far, bark, "bin")
    assert keep.all()
    with pytest.raises(ValueError):
        R.merge(np.array([1.0]), [1], bark, "hz")


def test_threshold_properties_of_the_restatement():
    # a flat PSD has no strict local maximum: theta is the absolute threshold alone, zero where that is undefined
    for sr in R.RATES:
        ath = R.tables(sr)[2]
        theta, count, margin = R.threshold(np.full((1, R.K), 30.0), sr)
        assert count[0] == 0 and margin[0] == np.inf
        fin = np.isfinite(ath)
        np.testing.assert_allclose(theta[0][fin], 10.0 ** (ath[fin] / 10.0), rtol=1e-15)
        assert np.all(theta[0][~fin] == 0) and (~fin).sum() >= 2
        assert np.isneginf(R.threshold_db(theta)[0][~fin]).all()
    # a silent clip: psd == 96 everywhere, finite
    p, mx = R.psd(np.zeros(4096))
    assert mx == -200.0 and np.all(p == 96.0)


def test_gpu_inputs_are_suitable():
    """What tests/test_psycho_gpu.py relies on, asserted for the committed seeds on the reference alone."""
    # 1. few frames whose discrete decisions are closer than the float32 levels can resolve
    total = low = low3 = 0
    for sr in R.RATES:
        for n in R.SIZES:
            for batch in (1, 3):
                for x in R.clips(n, sr, batch):
                    p, _ = R.psd(x.astype(np.float64))
                    for by in ("bin", "position"):
                        margin = R.threshold(p, sr, by)[2]
                        total += len(margin)
                        low += int((margin < R.MARGIN_DB).sum())
                        low3 += int((margin < 1e-3).sum())
    print(f"frames with a decision margin under 1e-4 dB: {low} of {total}; under 1e-3 dB: {low3}")
    assert low <= R.MAX_LEFT_OUT * total
    # 2. the sawtooth has 511 candidates, all over the ATH, and a margin of 1e-3 dB at least in both modes
    for by in ("bin", "position"):
        for sr in R.RATES:
            v = R.sawtooth(R.SAW_SEED[by])
            k = np.arange(1, R.K - 1)
            assert int(((v[k] > v[k - 1]) & (v[k] > v[k + 1])).sum()) == 511
            theta, count, margin = R.threshold(v[None, :], sr, by)
            print(f"sawtooth {by} sr {sr}: {count[0]} maskers survive, margin {margin[0]:.3e} dB")
            assert margin[0] >= 1e-3 and count[0] >= 1 and np.isfinite(theta).all()
    # 3. no bin of the loss tests sits on the hinge
    shares = {}
    for sr in R.RATES:
        for n in R.SIZES:
            for batch in (1, 3):
                xs, ds = R.clips(n, sr, batch), R.noise(n, batch)
                for x, d in zip(xs, ds):
                    p, mx = R.psd(x.astype(np.float64))
                    theta = R.threshold(p, sr)[0].astype(np.float32).astype(np.float64)
                    mx = float(np.float32(mx))
                    for amp in R.AMPLITUDES:
                        pw = R.loss_grad((np.float32(amp) * d).astype(np.float64), theta, mx, detail=True)[2]
                        assert not (np.abs(pw - theta) <= 1e-5 * theta).any(), (sr, n, batch, amp)
                        if np.any(x):
                            shares.setdefault(amp, []).append((pw > theta).mean())
    for amp, s in shares.items():
        print(f"share of bins over theta at amplitude {amp}: mean {100 * np.mean(s):.2f}% (min {100 * np.min(s):.2f}%, max {100 * np.max(s):.2f}%)")
    assert np.mean(shares[1e-3]) < np.mean(shares[1e-2]) < np.mean(shares[5e-2])
