"""CPU: the Lp attack restatement (tests/lp_attacks_ref.py) keeps its invariants and reduces to oracle.attacks_ref at norm inf;
the library exports the Lp entry points, _native.py binds them, and the Python surface validates ART's keywords."""
import math

import numpy as np
import pytest

import lp_attacks_ref as L
import lipasr._native as N
from oracle import attacks_ref as A, mlp_ref as P


def _small_net(seed=0):
    spec = [P.LayerSpec(24, 16, True, 0.0, False), P.LayerSpec(16, 12, True, 0.0, False), P.LayerSpec(12, 5, False, 0.0, False)]
    p = P.init_params(spec, seed=seed, dtype=np.float64)
    return spec, p


def test_directions_have_unit_norm():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((16, 880)) * rng.uniform(1e-3, 1e3, (16, 1))
    d2 = L.direction(g, 2)
    d1 = L.direction(g, 1)
    n2 = np.sqrt((d2 ** 2).sum(axis=1))
    n1 = np.abs(d1).sum(axis=1)
    gn2, gn1 = np.sqrt((g ** 2).sum(axis=1)), np.abs(g).sum(axis=1)
    np.testing.assert_allclose(n2, gn2 / (gn2 + L.TOL), rtol=1e-12)
    np.testing.assert_allclose(n1, gn1 / (gn1 + L.TOL), rtol=1e-12)
    assert np.all(np.abs(n2 - 1) <= L.TOL / gn2 * 1.01) and np.all(np.abs(n1 - 1) <= L.TOL / gn1 * 1.01)
    np.testing.assert_array_equal(L.direction(g, np.inf), np.sign(g))


def test_nan_and_inf_rules():
    g = np.ones((3, 8))
    g[0, 2] = np.nan
    g[1, 3] = np.inf
    for norm in (1, 2):
        d = L.direction(g, norm)
        assert np.isfinite(d).all()
        assert d[0, 2] == 0 and d[0, 0] > 0        # NaN entry -> 0, the row still steps
        assert (d[1] == 0).all()                  # a non-finite gradient norm: no step
    d = L.direction(g, "inf")
    assert d[1, 3] == 1 and d[0, 2] == 0          # norm inf: +-inf steps by its sign


@pytest.mark.parametrize("norm", [1, 2, np.inf])
def test_projection_lands_inside_the_ball(norm):
    rng = np.random.default_rng(1)
    x0 = rng.standard_normal((40, 300))
    for eps in (0.01, 0.5, 5.0):
        xa = x0 + rng.standard_normal(x0.shape) * rng.uniform(0, 3, (40, 1))
        g = rng.standard_normal(x0.shape)
        out = L.lp_step(xa, x0, g, 0.7, eps, norm)
        dl = out - x0
        nrm = np.abs(dl).max(axis=1) if norm == np.inf else (np.abs(dl).sum(axis=1) if norm == 1 else np.sqrt((dl ** 2).sum(axis=1)))
        assert (nrm <= eps * (1 + 1e-12)).all()
        # a step that stays inside is left alone
        small = L.lp_step(x0, x0, g, 1e-3 * eps, eps, norm)
        np.testing.assert_allclose(small, x0 + 1e-3 * eps * L.direction(g, norm), rtol=0, atol=1e-15)


def test_norm_inf_reproduces_the_oracle_pgd_and_fgsm():
    spec, p = _small_net()
    x = np.random.default_rng(2).standard_normal((45, 24))
    np.testing.assert_array_equal(L.pgd(spec, p, x, 0.3, 0.1, 7, norm=np.inf), A.pgd(spec, p, x, 0.3, 0.1, 7, 32))
    # FGM projects on the eps ball (ART's project=True); for a sign step of eps from x that is the identity up to rounding
    np.testing.assert_allclose(L.fgm(spec, p, x, 0.3, norm="inf"), A.fgsm(spec, p, x, 0.3), rtol=0, atol=1e-15)


def test_restarts_and_targets():
    spec, p = _small_net(3)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((20, 24))
    deltas = [0.2 * rng.standard_normal(x.shape) for _ in range(3)]
    single = L.pgd(spec, p, x, 1.0, 0.2, 5, norm=2, deltas=deltas[:1])
    multi = L.pgd(spec, p, x, 1.0, 0.2, 5, norm=2, deltas=deltas)
    later = [L.pgd(spec, p, x, 1.0, 0.2, 5, norm=2, deltas=[d]) for d in deltas]
    y = L.labels(spec, p, x)
    # every row is restart 0's, or a later restart's where that one succeeds
    for i in range(len(x)):
        cands = [later[0][i]] + [later[r][i] for r in (1, 2) if L.success(spec, p, x[i:i + 1], y[i:i + 1], later[r][i:i + 1], False)[0]]
        assert any(np.array_equal(multi[i], c) for c in cands)
    np.testing.assert_array_equal(single, later[0])
    with pytest.raises(ValueError):
        L.labels(spec, p, x, None, targeted=True)


def test_library_exports_and_binds_the_lp_entry_points():
    assert N.lib.lipasr_version() >= 510
    for name in ("lipasr_lp_step", "lipasr_lp_ball_init", "lipasr_mlp_attack_step_lp"):
        assert hasattr(N.lib, name) and name in N.PROTOTYPES
    # argument validation needs no GPU: a bad norm is rejected before anything touches the device
    assert N.lib.lipasr_lp_step(None, None, None, None, 1, 1, 2.0, 0.1, 0.1, None) == N.EINVAL
    fake = 1  # a non-null handle value is never dereferenced on the validation path below
    for bad in (0.0, 3.0, -math.inf, math.nan):
        assert N.lib.lipasr_lp_step(fake, fake, fake, fake, 1, 1, bad, 0.1, 0.1, None) == N.EINVAL
        assert "norm" in N.last_error()
        assert N.lib.lipasr_lp_ball_init(fake, fake, fake, 1, 1, bad, 0.1, 0, None, 0, None) == N.EINVAL
        assert N.lib.lipasr_mlp_attack_step_lp(fake, fake, fake, fake, fake, fake, 1, bad, 0.1, 0.1, None) == N.EINVAL
        assert "norm" in N.last_error()
    assert N.lib.lipasr_lp_ball_init(fake, fake, fake, 1, 1, 2.0, math.inf, 0, None, 0, None) == N.EINVAL


def test_keyword_validation():
    from lipasr import attacks as AT

    assert AT._norm_value(np.inf) == math.inf and AT._norm_value("inf") == math.inf
    assert AT._norm_value(1) == 1.0 and AT._norm_value(2) == 2.0
    for bad in (3, "2", 0, None, "l2"):
        with pytest.raises(ValueError):
            AT._norm_value(bad)
