"""The over-the-air channel without a GPU: lipasr.room.synthetic_rirs against its formula and its restatement, the float64
restatement of tests/room_ref.py against np.convolve and against its own adjoint, the host twins (lipasr_room_apply_host /
lipasr_room_vjp_host, the CPU-side handle on the ABI) against the float32 restatement bit for bit at the shapes the GPU tests run,
and every refusal the two launch functions make before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import room_ref as RR
from room_ref import SHAPES, ids

import lipasr._native as N
from lipasr.room import synthetic_rirs


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------- synthetic_rirs
def test_synthetic_rirs_follow_the_formula():
    h = synthetic_rirs(5, sr=16000, taps=700, t60=0.3, drr_db=6.0, seed=4)
    assert h.shape == (5, 700) and h.dtype == np.float32
    assert (h[:, 0] == 1.0).all()
    tail = (h[:, 1:].astype(np.float64) ** 2).sum(axis=1)
    # 699 float32 roundings of relative size 2^-24 each, on squares: 2 * 2^-24 relative at worst, whatever their signs
    assert np.abs(tail / 10.0 ** -0.6 - 1.0).max() <= 2.0 ** -23
    # the envelope: with t60 fixed, h[k] / 10^(-3 k / (t60 sr)) is a * eps_k, white -- its two halves have the same level
    env = 10.0 ** (-3.0 * np.arange(1, 700) / (0.3 * 16000))
    w = h[:, 1:] / env
    assert 0.7 < np.sqrt((w[:, :350] ** 2).mean() / (w[:, 350:] ** 2).mean()) < 1.4
    assert same(h, RR.synthetic_rirs(5, sr=16000, taps=700, t60=0.3, drr_db=6.0, seed=4))


def test_synthetic_rirs_are_fixed_by_the_seed():
    a, b = synthetic_rirs(4, taps=257, seed=3), synthetic_rirs(4, taps=257, seed=3)
    assert same(a, b) and same(a, RR.synthetic_rirs(4, taps=257, seed=3))
    assert not np.array_equal(a, synthetic_rirs(4, taps=257, seed=5))
    assert same(synthetic_rirs(3), RR.synthetic_rirs(3)) and synthetic_rirs(3).shape == (3, 2048)  # the defaults: ranges for both
    # ranges: the tail energy of every room lies in the range, and the rooms differ
    tail = (synthetic_rirs(16, taps=512, drr_db=(3.0, 9.0), seed=1)[:, 1:].astype(np.float64) ** 2).sum(axis=1)
    assert (tail <= 10 ** -0.3 * (1 + 1e-6)).all() and (tail >= 10 ** -0.9 * (1 - 1e-6)).all() and np.ptp(tail) > 0
    for kw in (dict(t60=0.2), dict(drr_db=3.0), dict(t60=(0.1, 0.2), drr_db=(0.0, 1.0)), dict(t60=0.2, drr_db=2.0)):
        assert same(synthetic_rirs(3, taps=64, seed=9, **kw), RR.synthetic_rirs(3, taps=64, seed=9, **kw)), kw
    assert same(synthetic_rirs(2, taps=1), np.ones((2, 1), dtype=np.float32)) and synthetic_rirs(0, taps=8).shape == (0, 8)
    for bad in (dict(taps=0), dict(taps=8193), dict(t60=0.0), dict(t60=(0.5, 0.1)), dict(count=-1)):
        with pytest.raises(ValueError):
            synthetic_rirs(**{"count": 2, **bad})


# ------------------------------------------------------------------------------------------------- the float64 restatement
SMALL = [s for s in SHAPES if s[0] * s[1] * s[2] * s[3] <= 2_000_000]


@pytest.mark.parametrize("shape", SMALL, ids=ids)
def test_restatement_is_a_convolution_and_its_own_adjoint(shape):
    clips, r, taps, n = shape
    x, g, h = RR.inputs(shape)
    ragged = np.array([(0, n, 1, 37, n + 5)[i % 5] for i in range(clips)])
    for nv in [None, ragged] + RR.ragged_lengths(clips, n):
        nvc = RR.clamp_lengths(nv, clips, n)
        out = RR.apply(x, h, nv)
        for b in range(clips):
            for j in range(r):
                want = np.zeros(n)
                if nvc[b]:
                    want[:nvc[b]] = np.convolve(x[b, :nvc[b]].astype(np.float64), h[j].astype(np.float64))[:nvc[b]]
                assert np.abs(out[b * r + j] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) * taps
        gx = RR.vjp(g, h, nv)
        assert not gx[np.arange(n)[None, :] >= nvc[:, None]].any()
        terms = np.abs(out * g).sum() + np.abs(x * gx).sum()
        assert abs((out * g).sum() - (x * gx).sum()) <= 1e-12 * terms, (shape, nv)
        assert np.array_equal(RR.vjp(g, h, nv, scale=0.25), 0.25 * gx)


# ------------------------------------------------------------------------------------------------- the host twins
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_host_twins_equal_the_float32_restatement(shape):
    clips, r, taps, n = shape
    x, g, h = RR.inputs(shape)
    for nv in [None] + RR.ragged_lengths(clips, n):
        out = N.room_apply_host(x, h, n_valid=nv, out=np.full((clips * r, n), 7.0, dtype=np.float32))
        assert same(out, RR.apply(x, h, nv, dtype=np.float32)), (shape, nv)
        v32 = RR.vjp(g, h, nv, dtype=np.float32)
        for scale in (1.0, 1.0 / 3.0):
            gx = N.room_vjp_host(g, h, n_valid=nv, scale=scale, out=np.full((clips, n), 7.0, dtype=np.float32))
            assert same(gx, np.float32(scale) * v32), (shape, nv, scale)  # RR.vjp's last line: the sums, then one multiply
        assert same(RR.vjp(g, h, nv, scale=1.0 / 3.0, dtype=np.float32), np.float32(1.0 / 3.0) * v32)


# ------------------------------------------------------------------------------------------------- the ABI
def test_abi_has_the_channel():
    assert N.lib.lipasr_version() >= 680
    assert all(N.has(f"lipasr_room_{k}{t}") and hasattr(N.lib, f"lipasr_room_{k}{t}") for k in ("apply", "vjp") for t in ("", "_host"))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_launch_functions_refuse_before_the_device():
    """Every check of lipasr_room_apply / lipasr_room_vjp comes before the launch, so it is reached without a GPU; the pointers are
    host arrays that a refused call never reads."""
    x = np.zeros((2, 8), dtype=np.float32)
    rows = np.zeros((6, 8), dtype=np.float32)
    h = np.zeros((3, 4), dtype=np.float32)
    ap = lambda x_, nv, h_, taps, r, clips, n, out: N.lib.lipasr_room_apply(x_, nv, h_, taps, r, clips, n, out, None)
    vj = lambda g_, nv, h_, taps, r, clips, n, gx: N.lib.lipasr_room_vjp(g_, nv, h_, taps, r, clips, n, 1.0, gx, None)
    for fn, sig, big in ((ap, x, rows), (vj, rows, x)):
        first, last = _p(sig), _p(big)
        # nothing to do: LIPASR_OK without a launch, whatever the pointers
        assert fn(None, None, None, 4, 3, 0, 8, None) == N.OK and fn(None, None, None, 4, 0, 2, 8, None) == N.OK
        assert fn(None, None, None, 4, 3, 2, 0, None) == N.OK
        for taps in (0, -1, 8193):
            assert fn(first, None, _p(h), taps, 3, 2, 8, last) == N.EINVAL and "taps" in N.last_error()
            assert fn(None, None, None, taps, 3, 0, 8, None) == N.EINVAL  # also where there is nothing to do
        assert fn(first, None, _p(h), 4, -1, 2, 8, last) == N.EINVAL and fn(first, None, _p(h), 4, 3, -2, 8, last) == N.EINVAL
        assert fn(first, None, _p(h), 4, 3, 2, -8, last) == N.EINVAL
        for args in ((None, _p(h), last), (first, None, last), (first, _p(h), None)):
            assert fn(args[0], None, args[1], 4, 3, 2, 8, args[2]) == N.EINVAL and "null" in N.last_error()
    # an output that overlaps an input
    flat = np.zeros(100, dtype=np.float32)
    at = lambda off: C.c_void_p(flat.ctypes.data + 4 * off)
    assert ap(at(0), None, _p(h), 4, 3, 2, 8, at(15)) == N.EINVAL and "overlaps" in N.last_error()   # x [0, 16), out [15, 63)
    assert ap(at(0), None, at(60), 4, 3, 2, 8, at(16)) == N.EINVAL                                   # out [16, 64) over rirs [60, 72)
    assert vj(at(0), None, _p(h), 4, 3, 2, 8, at(47)) == N.EINVAL and "overlaps" in N.last_error()   # g [0, 48), gx [47, 63)
    assert vj(at(0), None, at(50), 4, 3, 2, 8, at(60)) == N.EINVAL                                   # gx [60, 76) over rirs [50, 62)
    assert N.lib.lipasr_room_vjp(_p(rows), None, _p(h), 4, 3, 2, 8, float("nan"), _p(x), None) == N.EINVAL and "scale" in N.last_error()
    # the host twins make the same checks
    assert N.lib.lipasr_room_apply_host(at(0), None, _p(h), 4, 3, 2, 8, at(15)) == N.EINVAL
    assert N.lib.lipasr_room_vjp_host(at(0), None, _p(h), 9000, 3, 2, 8, 1.0, at(50)) == N.EINVAL
    with pytest.raises(ValueError):
        N.room_vjp_host(np.zeros((5, 8), dtype=np.float32), h)  # 5 rows are no multiple of 3 rooms


def test_the_estimator_is_part_of_the_surface():
    from lipasr import attacks, estimators

    assert attacks.OverTheAirClassifier is estimators.OverTheAirClassifier
    assert issubclass(estimators.OverTheAirClassifier, estimators.WaveformClassifier)
    assert "OverTheAirClassifier" in estimators.__doc__ and "predict_each_device" in estimators.OverTheAirClassifier.__doc__
    with pytest.raises(TypeError):
        estimators.OverTheAirClassifier(object(), None)
