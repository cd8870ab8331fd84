"""DolphinAttack without a GPU: the host tables of csrc/dolphin_tables.h (fetched through lipasr_dolphin_table) against SciPy, the
centred interpolator / decimator against MATLAB's resample rule, the two recorded quirks of the reference script, and the
error convention of the new entry points."""
import ctypes as C

import numpy as np
import pytest
from scipy import signal

import dolphin_ref as D
import lipasr._native as N


def test_bandpass_table_against_scipy():
    sos = N.dolphin_table(0).reshape(10, 6)
    # every section: numerator g (1, 0, -1), monic denominator
    assert np.all(sos[:, 1] == 0) and np.all(sos[:, 2] == -sos[:, 0]) and np.all(sos[:, 3] == 1)
    imp = np.zeros(16000)
    imp[0] = 1.0
    ref = signal.sosfilt(D.sos(), imp)
    got = signal.sosfilt(sos, imp)
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
    poles = np.concatenate([np.roots(s[3:]) for s in sos])
    assert len(poles) == 20 and np.abs(poles).max() <= 0.99393 and np.abs(poles).max() > 0.99
    assert np.all(np.abs(np.imag(poles)) > 0)  # ten conjugate pairs
    # the chunked scan's carry: each section's zero-input state map to the power of 64
    mp = N.dolphin_table(3).reshape(10, 2, 2)
    for s, m in zip(sos, mp):
        step = np.array([[-s[4], 1.0], [-s[5], 0.0]])
        np.testing.assert_allclose(m, np.linalg.matrix_power(step, 64), rtol=1e-10, atol=0)  # six squarings in fp64, either way


def test_resampling_filters_against_restatement():
    h_up, h_dn = N.dolphin_table(1), N.dolphin_table(2)
    assert h_up.shape == (241,) and h_dn.shape == (241,)
    assert np.abs(h_up - D.resample_filter(12, 1)).max() <= 1e-12
    assert np.abs(h_dn - D.resample_filter(1, 12)).max() <= 1e-12
    assert abs(h_up.sum() - 12) <= 1e-12 and abs(h_dn.sum() - 1) <= 1e-12


def test_centred_forms_equal_matlab_rule():
    x = np.random.default_rng(7).standard_normal(500)
    u = D.up_centred(x, D.resample_filter(12, 1))
    ref = D.matlab_resample(x, 12, 1)
    assert u.shape == ref.shape == (6000,)
    np.testing.assert_array_equal(u, ref)
    w = np.random.default_rng(8).standard_normal(6000)
    r = D.down_centred(w, D.resample_filter(1, 12))
    ref = D.matlab_resample(w, 1, 12)
    assert r.shape == ref.shape == (500,)
    np.testing.assert_array_equal(r, ref)


def test_quirk_transfer_function_form_is_unstable():
    """filter(b, a, x) with [b, a] = butter(10, [100 7000]/8000) cannot be reproduced literally: in double precision the
    20th-order denominator has roots outside the unit circle, which the section form does not."""
    b, a = D.ba()
    assert len(a) == 21 and np.abs(np.roots(a)).max() > 1
    assert max(np.abs(np.roots(s[3:])).max() for s in D.sos()) < 1


def test_quirk_carrier_level_decides_what_is_demodulated():
    """With the script's 0.001 the recorded clip is essentially v^2; with the paper's carrier level 1 it is v."""
    x = D.chirp(4100, seed=1)
    v, _, _, r = D.chain(x, np.float64, carrier_level=1.0)
    hi = D.demod_correlation(r, v)
    v, _, _, r = D.chain(x, np.float64, carrier_level=0.001)
    lo = D.demod_correlation(r, v)
    print(f"correlation of the recorded clip with the voice: {hi:.4f} at carrier level 1, {lo:.4f} at 0.001")
    assert hi >= 0.9 and lo <= 0.2


def test_float32_oracle_runs_in_float32():
    x = D.chirp(1000)
    v, s, pk, r = D.chain(x, np.float32)
    v64, s64, pk64, r64 = D.chain(x, np.float64)
    assert v.dtype == s.dtype == pk.dtype == r.dtype == np.float32
    assert 0 < np.abs(v - v64).max() / np.abs(v64).max() < 1e-3 and np.abs(s - s64).max() < 1e-3


def test_error_convention_without_gpu():
    plan = N.c_h()
    assert N.lib.lipasr_dolphin_destroy(None) == N.EINVAL
    assert "null plan" in N.last_error()
    assert N.lib.lipasr_dolphin_create(None, 16000, 4100, 5, 30000.0, 0.001, None) == N.EINVAL
    assert N.lib.lipasr_dolphin_create(None, 8000, 4100, 5, 30000.0, 0.001, C.byref(plan)) == N.EUNSUPPORTED
    assert "16000" in N.last_error()
    for hz in (7000.0, 89000.0, 30000.5):
        assert N.lib.lipasr_dolphin_create(None, 16000, 4100, 5, hz, 0.001, C.byref(plan)) == N.EINVAL
        assert "carrier_hz" in N.last_error()
    assert N.lib.lipasr_dolphin_create(None, 16000, 4100, 5, 30000.0, -1.0, C.byref(plan)) == N.EINVAL
    assert "carrier_level" in N.last_error()
    assert N.lib.lipasr_dolphin_create(None, 16000, 4100, 5, 30000.0, 0.001, C.byref(plan)) == N.EINVAL  # null handle
    assert not plan.value
    assert N.lib.lipasr_dolphin_bandpass(None, None, None, 1, None, None) == N.EINVAL
    assert N.lib.lipasr_dolphin_generate(None, None, None, 1, None, None, None) == N.EINVAL
    assert N.lib.lipasr_dolphin_record(None, None, None, 1, 1.0, 0.5, None, None) == N.EINVAL
    assert N.lib.lipasr_dolphin_generate_recorded(None, None, None, 1, 1.0, 0.5, None, None) == N.EINVAL
    assert N.lib.lipasr_dolphin_table(99, 16000, None, 0) == N.EINVAL
    assert N.lib.lipasr_dolphin_table(0, 8000, None, 0) == N.EUNSUPPORTED
    small = (C.c_double * 4)()
    assert N.lib.lipasr_dolphin_table(1, 16000, small, 4) == N.EINVAL
    with pytest.raises(ValueError):
        N.check(N.lib.lipasr_dolphin_destroy(None))
    assert N.lib.lipasr_version() >= 570 and N.has("lipasr_dolphin_generate_recorded")


def test_chunked_scan_on_the_library_tables_equals_sosfilt():
    """The band-pass kernel's algorithm restated in NumPy on the tables the kernel reads: per section a zero-state run of every
    64-sample chunk, the carry of the (z0, z1) state of the transposed direct form II across chunks with M^64, and the re-run from
    the carried state.  In float64 it equals sosfilt to 1e-9 of the peak; so do the polyphase forms of the interpolator and decimator."""
    sos, mp = N.dolphin_table(0).reshape(10, 6), N.dolphin_table(3).reshape(10, 2, 2)
    x = D.chirp(1000, seed=5)
    n_chunks = -(-len(x) // 64)
    y = np.concatenate([x, np.zeros(64 * n_chunks - len(x))]).reshape(n_chunks, 64)

    def run(sec, rows, z):
        g, a1, a2 = sec[0], sec[4], sec[5]
        out = np.empty_like(rows)
        z0, z1 = z[:, 0].copy(), z[:, 1].copy()
        for k in range(64):
            xk = rows[:, k]
            out[:, k] = g * xk + z0
            z0, z1 = z1 - a1 * out[:, k], -g * xk - a2 * out[:, k]
        return out, np.stack([z0, z1], axis=1)

    for sec, m in zip(sos, mp):
        _, zend = run(sec, y, np.zeros((n_chunks, 2)))
        init, st = np.zeros((n_chunks, 2)), np.zeros(2)
        for c in range(n_chunks):
            init[c] = st
            st = m @ st + zend[c]
        y, _ = run(sec, y, init)
    ref = signal.sosfilt(D.sos(), x)
    # (1e-9 of the peak, the bound the tabulated cascade itself is held to above: the scan re-associates each section's recurrence
    # once per chunk and superposes two responses, a few thousand float64 roundings away from sosfilt's order)
    assert np.abs(y.reshape(-1)[:len(x)] - ref).max() <= 1e-9 * np.abs(ref).max()
    # polyphase fragments as csrc/dolphin_tables.h cuts them: [p][t + 10] = h_up[120 + 12 t + p] and h_dn[120 - 12 t - p]
    h_up, h_dn = N.dolphin_table(1), N.dolphin_table(2)
    take = lambda h, i: h[i] if 0 <= i <= 240 else 0.0
    v = ref
    vp = np.concatenate([np.zeros(10), v, np.zeros(10)])
    u = np.array([sum(take(h_up, 120 + 12 * t + p) * vp[q - t + 10] for t in range(-10, 11)) for q in range(len(v)) for p in range(12)])
    assert np.abs(u - D.up_centred(v, D.resample_filter(12, 1))).max() <= 1e-12
    w = np.concatenate([np.zeros(120), u, np.zeros(132)])
    r = np.array([sum(take(h_dn, 120 - 12 * t - p) * w[12 * (i + t) + p + 120] for p in range(12) for t in range(-10, 11)) for i in range(len(v))])
    assert np.abs(r - D.down_centred(u, D.resample_filter(1, 12))).max() <= 1e-12
