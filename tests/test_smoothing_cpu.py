"""Randomized smoothing without a GPU: the host statistics against scipy, the counter layout of the noise (the host table
lipasr_smooth_noise_host against the Philox / Box-Muller restatement of tests/smoothing_ref.py), the argument checks of the two
launch functions, the oracle CERTIFY on a linear classifier whose exact radius is known, and the menu plumbing."""
import ctypes as C
import math
from statistics import NormalDist

import numpy as np
import pytest

import smoothing_ref as S

ALPHAS = (0.001, 0.05)
NS = (1, 2, 10, 100, 1000, 100000)


def _ks(n, lowest=1):
    return sorted({k for k in (0, 1, 2, n // 2, n // 2 + 1, int(0.9 * n), int(0.99 * n), n - 2, n - 1, n) if lowest <= k <= n})


# ---------------------------------------------------------------------------------------------------------------- statistics
def test_cp_lower_matches_scipy():
    """1 - p within 1e-9 relative of scipy.stats.beta.ppf, Phi^-1(p) within 1e-8 of scipy.stats.norm.ppf (the errors are taken on
    1 - p because Phi^-1 amplifies an error near 1).  Measured on the grid below: 7.3e-11 and 2.7e-10."""
    from scipy import stats

    from lipasr.smoothing import cp_lower

    worst_p = worst_r = 0.0
    for n in NS:
        for k in _ks(n):
            for alpha in ALPHAS:
                p, ref = cp_lower(k, n, alpha), float(stats.beta.ppf(alpha, k, n - k + 1))
                assert 0.0 < p < 1.0
                e_p = abs((1.0 - p) - (1.0 - ref)) / (1.0 - ref)
                e_r = abs(NormalDist().inv_cdf(p) - float(stats.norm.ppf(ref)))
                worst_p, worst_r = max(worst_p, e_p), max(worst_r, e_r)
                assert e_p <= 1e-9, (n, k, alpha, p, ref)
                assert e_r <= 1e-8, (n, k, alpha, p, ref)
    print(f"cp_lower: worst relative error of 1 - p {worst_p:.2e}, worst error of Phi^-1(p) {worst_r:.2e}")
    assert cp_lower(0, 10, 0.001) == 0.0
    for n in NS:
        assert cp_lower(n, n, 0.001) == 0.001 ** (1.0 / n)
    for bad in ((-1, 10, 0.1), (11, 10, 0.1), (1, 0, 0.1), (1, 10, 0.0), (1, 10, 1.0)):
        with pytest.raises(ValueError):
            cp_lower(*bad)


def test_binom_p_two_sided_matches_scipy():
    from scipy import stats

    from lipasr.smoothing import binom_p_two_sided

    worst = 0.0
    for n in NS:
        for n_a in _ks(n, lowest=0):
            p, ref = binom_p_two_sided(n_a, n - n_a), float(stats.binomtest(n_a, n, 0.5).pvalue)
            err = abs(p - ref) / ref if ref > 0 else abs(p - ref)
            worst = max(worst, err)
            assert err <= 1e-9, (n, n_a, p, ref)
    print(f"binom_p_two_sided: worst relative error {worst:.2e}")
    assert binom_p_two_sided(0, 0) == 1.0 and binom_p_two_sided(7, 7) == 1.0
    assert binom_p_two_sided(3, 9) == binom_p_two_sided(9, 3)
    with pytest.raises(ValueError):
        binom_p_two_sided(-1, 3)


# ---------------------------------------------------------------------------------------------------------------- the noise
def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10: the restatement is the published generator."""
    got = S.philox4x32(0, np.array([0], dtype=np.uint64), 0, 0)[:, 0]
    assert [int(v) for v in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    seed = 0xFFFFFFFF | (0xFFFFFFFF << 32)
    got = S.philox4x32(seed, np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64), 0xFFFFFFFF, 0xFFFFFFFF)[:, 0]
    assert [int(v) for v in got] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 881])
def test_noise_table_matches_the_restatement(n):
    """|z - z_ref| <= 1e-5: r = sqrt(-2 ln u) <= 5.8 (u >= 2^-24); the fp32 rounding of t = 2 pi u is at most 2.4e-7, two units in
    the last place of cosf another 2.4e-7, a few units in the last place on r about 2e-6: about 5e-6 in all.  A wrong counter
    moves z by order 1."""
    from lipasr import _native as N

    worst = 0.0
    for seed in (0, 1, 12345, 2 ** 40 + 7, 2 ** 64 - 1):
        for clip in (0, 1, 5, 70000, 2 ** 32 - 1):
            for draw in (0, 1, 99, 100000):
                z = N.smooth_noise(seed, clip, draw, n)
                assert z.dtype == np.float32 and z.shape == (n,)
                err = np.abs(z.astype(np.float64) - S.normal(seed, clip, draw, n)).max()
                worst = max(worst, err)
                assert err <= 1e-5, (seed, clip, draw, n, err)
    print(f"n = {n}: worst |z - z_ref| {worst:.2e}")


def test_noise_table_is_standard_normal_and_keyed_by_every_argument():
    from lipasr import _native as N

    z = N.smooth_noise(3, 2, 1, 200000).astype(np.float64)
    assert abs(z.mean()) < 4 / math.sqrt(z.size) and abs(z.var() - 1.0) < 4 * math.sqrt(2.0 / z.size)
    base = N.smooth_noise(3, 2, 1, 64)
    for other in ((4, 2, 1), (3, 3, 1), (3, 2, 2)):
        assert np.abs(N.smooth_noise(*other, 64) - base).max() > 0.5
    # a prefix of a longer call: element k depends on k alone
    np.testing.assert_array_equal(N.smooth_noise(3, 2, 1, 881)[:64], base)
    # draw 0 carries the counters of add_noise_kernel (ctr = k >> 2, hi0 = row, hi1 = 0)
    o = S.philox4x32(9, np.arange(2, dtype=np.uint64), 4, 0)
    u = ((o >> np.uint64(8)) + np.uint64(1)).astype(np.float64) / 16777216.0
    want = np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1])
    assert np.abs(N.smooth_noise(9, 4, 0, 8)[[0, 4]] - want).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _expand(h=None, x=None, out=None, batch=2, n=8, draws=3, sigma=0.1, lo=-math.inf, hi=math.inf):
    from lipasr import _native as N

    return N.lib.lipasr_smooth_expand(h, x, None, batch, n, draws, 0, 0, sigma, 0, lo, hi, out, None)


def test_abi_argument_checks_without_a_device():
    """Every argument check comes before the handle is looked at and before the device is touched; a fake non-null handle reaches
    the null-pointer checks (the handle is not dereferenced before them)."""
    from lipasr import _native as N

    assert N.lib.lipasr_version() >= 610 and N.has("lipasr_smooth_expand") and N.has("lipasr_smooth_vote")
    assert len(N.lib.lipasr_smooth_expand.argtypes) == 14 and len(N.lib.lipasr_smooth_vote.argtypes) == 7
    for kw, msg in ((dict(sigma=-0.1), "sigma -0.1"), (dict(sigma=math.inf), "sigma inf"), (dict(sigma=math.nan), "sigma"),
                    (dict(lo=1.0, hi=-1.0), "clip range"), (dict(lo=math.nan), "clip range"), (dict(batch=-1), "bad shape"),
                    (dict(), "null handle"), (dict(h=C.c_void_p(8)), "x or out is null"),
                    (dict(h=C.c_void_p(8), x=C.c_void_p(16)), "x or out is null")):
        assert _expand(**kw) == N.EINVAL, kw
        assert msg in N.last_error().lower(), (kw, N.last_error())
    for zero in (dict(batch=0), dict(draws=0), dict(n=0)):
        assert _expand(h=C.c_void_p(8), **zero) == N.OK
    vote = lambda h=None, logits=None, counts=None, classes=10: N.lib.lipasr_smooth_vote(h, logits, 2, 5, classes, counts, None)
    for kw, msg in ((dict(classes=0), "0 classes"), (dict(classes=33), "33 classes"), (dict(), "null handle"),
                    (dict(h=C.c_void_p(8)), "logits or counts is null"), (dict(h=C.c_void_p(8), logits=C.c_void_p(16)), "logits or counts is null")):
        assert vote(**kw) == N.EINVAL, kw
        assert msg in N.last_error(), (kw, N.last_error())
    assert N.lib.lipasr_smooth_noise_host(0, 0, 0, 4, None) == N.EINVAL and "z_out is null" in N.last_error()
    assert N.lib.lipasr_smooth_noise_host(0, 0, 0, -1, None) == N.EINVAL
    assert N.lib.lipasr_smooth_noise_host(0, 0, 0, 0, None) == N.OK


def test_smooth_is_exported_and_checks_its_arguments():
    import inspect

    from lipasr import attack_eval as V, smoothing as Z
    from lipasr.extract_features_construct_dataset import get_robustness_radius

    sig = inspect.signature(Z.Smooth.__init__)
    assert list(sig.parameters)[1:3] == ["estimator", "sigma"]
    for k, d in (("seed", 0), ("clip_values", None)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d
    sig = inspect.signature(Z.Smooth.certify)
    assert [sig.parameters[k].default for k in ("n0", "n", "alpha", "lengths")] == [100, 100_000, 0.001, None]
    sig = inspect.signature(Z.Smooth.predict)
    assert [sig.parameters[k].default for k in ("n", "alpha", "lengths")] == [1000, 0.001, None]
    with pytest.raises(TypeError):
        Z.Smooth(object(), 0.1)
    assert inspect.signature(get_robustness_radius).parameters["smoothing"].default is None
    assert callable(V.smooth_report)


def test_menu_accepts_smooth(tmp_path):
    """attack_eval.main takes --attack smooth (argparse would exit with status 2) and goes on to load the dataset; without --sigma
    it is refused before anything is loaded."""
    from lipasr import attack_eval as V

    missing = str(tmp_path) + "/missing/"
    for over in ("mfcc", "audio"):
        with pytest.raises(FileNotFoundError):
            V.main(["--attack", "smooth", "--sigma", "0.25", "--n0", "10", "--n", "100", "--alpha", "0.01", "--over", over, "--points", "8",
                    "--path", missing])
    with pytest.raises(FileNotFoundError):
        V.main(["--attack", "smooth", "--sigma", "0.25", "--path", missing])
    with pytest.raises(ValueError, match="sigma"):
        V.main(["--attack", "smooth", "--path", missing])
    with pytest.raises(ValueError, match="sigma"):
        V.main(["--attack", "smooth", "--sigma", "-1", "--path", missing])
    with pytest.raises(SystemExit):
        V.main(["--attack", "smooth", "--sigma", "x", "--path", missing])


# ---------------------------------------------------------------------------------------------------------------- CERTIFY
def host_noise(seed, clip, draw, n):
    from lipasr import _native as N

    return N.smooth_noise(seed, clip, draw, n)


def test_oracle_certify_on_a_linear_classifier():
    """One dense layer 880 -> 2; six rows at 1, 1, 1.5, 1.5, 2, 2 sigma from the boundary, where the smoothed classifier's exact
    radius is the distance itself.  The draws are the host table's, the classifier and CERTIFY are float64 (scipy's beta.ppf and
    norm.ppf).  smoothing_ref.LINEAR_SEED = 0 is the first seed tried; it passes with room (radius / d between 0.90 and 0.95)."""
    W, bias, x, d, cls = S.linear_case(S.LINEAR_SEED, S.LINEAR_SIGMA)
    np.testing.assert_allclose(d / S.LINEAR_SIGMA, [1, 1, 1.5, 1.5, 2, 2], rtol=1e-5)
    res = S.certify(S.linear_classify(W, bias), x, S.LINEAR_SIGMA, seed=S.LINEAR_SEED, noise=host_noise, **S.LINEAR)
    S.check_linear(res["cls"], res["radius"], d, cls)
    assert (res["counts"].sum(axis=1) == S.LINEAR["n"]).all() and (res["counts_select"].sum(axis=1) == S.LINEAR["n0"]).all()
    # the library's own bound on the same counts
    from lipasr.smoothing import cp_lower

    for b in range(len(d)):
        p = cp_lower(int(res["counts"][b, cls[b]]), S.LINEAR["n"], S.LINEAR["alpha"])
        assert abs(p - res["p_lower"][b]) <= 1e-9 * (1 - res["p_lower"][b])


def test_vote_and_expand_conventions_of_the_oracle():
    """The edges include/lipasr.h fixes, on the definition the device tests compare against."""
    z = np.array([[1.0, 3.0, 3.0], [np.inf, 2.0, np.inf], [np.nan, 9.0, 1.0], [-np.inf, -np.inf, -np.inf], [0.0, 0.0, 5.0], [1.0, 0.0, 0.0]])
    np.testing.assert_array_equal(S.vote(z, 2), [[1, 1, 0, 1], [2, 0, 1, 0]])
    x = np.arange(12, dtype=np.float32).reshape(2, 6)
    out, valid = S.expand(x, 3, 0.5, seed=1, n_valid=[4, -2], lo=1.0, hi=8.0)
    assert out.shape == (6, 6) and valid[:3, :4].all() and not valid[:3, 4:].any() and not valid[3:].any()
    np.testing.assert_array_equal(out[3:], np.repeat(x[1:2], 3, axis=0))
    np.testing.assert_array_equal(out[:3, 4:], np.repeat(x[:1, 4:], 3, axis=0))
    assert out[:3, :4].min() >= 1.0 and out[:3, :4].max() <= 8.0
    a, _ = S.expand(x, 5, 0.5, seed=1)
    b0, _ = S.expand(x[1:], 2, 0.5, seed=1, clip0=1, draw0=3)
    np.testing.assert_array_equal(b0, a[8:10])
