"""The time-warp operator without a GPU: the table, known answers bit for bit, the host twins against the float64 restatement of
tests/warp_ref.py within a DERIVED bound, what the parameter gradient means (central differences of the float64 restatement), the
float64 attack drivers on the test bed of the device tests (not vacuous: a quarter of the rows flip, not all, none near a tie, and
the refinement lowers a margin), candidate_grid, and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

import warp_ref as R

import lipasr._native as N

Z, P = R.Z, R.P
IDENT = (0.0, 1.0, 1.0)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def test_version_and_symbols():
    names = ["lipasr_warp_table_host", "lipasr_warp_apply", "lipasr_warp_param_vjp", "lipasr_warp_apply_host",
             "lipasr_warp_param_vjp_host", "lipasr_debug_warp_launches"]
    assert N.lib.lipasr_version() >= 720 and all(N.has(n) and N.SINCE[n] == 720 and n in N.PROTOTYPES for n in names)
    assert N.lib.lipasr_debug_warp_launches(0) >= 0 and N.lib.lipasr_debug_warp_launches(1) >= 0
    assert N.lib.lipasr_debug_warp_launches(-1) == -1 and N.lib.lipasr_debug_warp_launches(2) == -1


def test_table():
    win, delta = N.warp_table_host()
    assert win.dtype == delta.dtype == np.float32 and win.shape == delta.shape == (Z * P + 1,)
    assert win[0] == 1.0 and np.all(win[P::P] == 0.0) and len(win[P::P]) == Z and win[Z * P] == 0.0
    ref = R.table_formula()
    # one fp32 rounding of the float64 value (half a spacing), plus what two float64 evaluations of it may differ by
    err = np.abs(win.astype(np.float64) - ref)
    assert np.all(err <= 0.5 * R.spacing32(ref) + 1e-15), float((err / R.spacing32(ref)).max())
    assert np.array_equal(delta[:-1], win[1:] - win[:-1]) and delta[-1] == 0.0


@pytest.mark.parametrize("n,nv", [(37, 37), (37, 20), (4099, 4099), (4099, 2 * Z - 1), (5, 1)])
def test_known_answers_bit_for_bit(n, nv):
    rng = np.random.default_rng(n + nv)
    x = f32(rng.standard_normal((2, n)))
    lens = np.array([nv, n], dtype=np.int32)
    shifts = [0, 1, 5, nv - 1, nv, nv + 40, -1, -3, -nv]
    params = f32([(s, 1.0, 1.0) for s in shifts] + [(0.0, 1.0, 0.5), (2.0, 1.0, 0.5)])
    K = len(params)
    out = N.warp_apply_host(x, np.tile(params, (2, 1)), K, n_valid=lens)
    for b, v in enumerate((nv, n)):
        for j, s in enumerate(shifts + [0, 2]):
            want = np.zeros(n, dtype=np.float32)
            src = np.arange(v) - s
            ok = (src >= 0) & (src < v)
            want[:v][ok] = x[b, src[ok]]
            if j >= len(shifts):
                want = want * np.float32(0.5)
            assert np.array_equal(out[b * K + j], want), (b, j, s)
    assert np.array_equal(N.warp_apply_host(x, np.tile(f32([IDENT]), (2, 1)), 1), x)


CASES = [(n, nv, K) for n in R.NS for nv in R.nvs(n) for K in (1, 5)]


@pytest.mark.parametrize("n,nv,K", CASES)
def test_twin_against_float64(n, nv, K):
    x, lens, params, g = R.grid_case(n, nv, K)
    out = N.warp_apply_host(x, params, K, n_valid=lens)
    ref, rows = R.warp_apply(x, params, K, lens, parts=True)
    worst = 0.0
    for r, row in enumerate(rows):
        v = R.clamp_nv(lens, r // K, n)
        bound = R.out_bound(row, params[r, 2])
        err = np.abs(out[r].astype(np.float64) - ref[r])
        assert np.all(err <= bound), (r, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(out[r, v:] == 0.0)
        worst = max(worst, float((err[:v] / np.maximum(bound[:v], 1e-300)).max()) if v else 0.0)
    gp = N.warp_param_vjp_host(x, g, params, K, n_valid=lens)
    gref, gbound = R.param_vjp(x, g, params, K, lens)
    gerr = np.abs(gp - gref)
    assert np.all(gerr <= gbound), (gerr / np.maximum(gbound, 1e-300)).max()
    gworst = float((gerr / np.maximum(gbound, 1e-300)).max())
    print(f"n={n} nv={nv} K={K}: worst |out32 - out64| / bound {worst:.3f}, worst |gp - gp64| / bound {gworst:.3f}")
    # the same call made twice gives the same bits
    assert np.array_equal(out, N.warp_apply_host(x, params, K, n_valid=lens))
    # no lengths: every row is whole
    if nv == n:
        assert np.array_equal(N.warp_apply_host(x[:1], params[:K], K), out[:K])


def test_bad_rows_are_nan_and_stay_in_their_rows():
    x, lens, params, g = R.grid_case(37, 30, 5)
    good_out = N.warp_apply_host(x, params, 5, n_valid=lens)
    good_gp = N.warp_param_vjp_host(x, g, params, 5, n_valid=lens)
    bad = params.copy()
    bad[1] = (np.nan, 1.0, 1.0)
    bad[3] = (0.0, 3.0, 1.0)
    bad[7] = (0.0, 1.0, np.inf)
    bad[9] = (0.0, 0.4, 1.0)
    out = N.warp_apply_host(x, bad, 5, n_valid=lens)
    gp = N.warp_param_vjp_host(x, g, bad, 5, n_valid=lens)
    for r in range(15):
        v = R.clamp_nv(lens, r // 5, 37)
        if r in (1, 3, 7, 9):
            assert np.isnan(out[r, :v]).all() and np.all(out[r, v:] == 0.0) and np.isnan(gp[r]).all()
        else:
            assert np.array_equal(out[r], good_out[r]) and np.array_equal(gp[r], good_gp[r])


def test_gradient_meaning():
    """The float64 restatement's gp against central differences of sum_t g_t out_t on a smooth two-tone."""
    n = 600
    t = np.arange(n)
    x = (0.6 * np.sin(2 * np.pi * 0.031 * t + 0.3) + 0.4 * np.sin(2 * np.pi * 0.0773 * t + 1.1))[None, :]
    # per parameter q the cotangent is d out / d p_q itself, so that the sum is one of squares: against an arbitrary cotangent
    # the terms cancel (the rate's factor t - c is odd about the centre, a shift keeps a tone's energy) and no relative figure
    # means much
    worst = 0.0
    for triple in [(3.37, 1.0, 1.0), (-100.25, 1.07, 0.7), (12.5, 0.9, 1.4)]:
        p = np.array([triple])
        row = R.warp_row(x[0], n, *triple)
        tc = t - (n - 1) / 2.0
        cots = [-triple[2] * row["dxu"], triple[2] * row["dxu"] * tc, row["acc"]]
        for q, h in enumerate((1e-4, 5e-8, 1e-4)):
            g = cots[q][None, :]
            gp, _ = R.param_vjp(x, g, p, 1)
            assert gp[0, q] > 0
            e = np.zeros((1, 3))
            e[0, q] = h
            fd = (np.sum(g * R.warp_apply(x, p + e, 1)) - np.sum(g * R.warp_apply(x, p - e, 1))) / (2 * h)
            rel = abs(fd - gp[0, q]) / abs(fd)
            worst = max(worst, rel)
            assert rel <= 2e-3, (triple, q, fd, gp[0, q])
    print(f"worst relative distance to central differences {worst:.2e}")


def test_float64_drivers_are_not_vacuous():
    from lipasr.warp import candidate_grid

    x, lengths = R.clips()
    m = R.model()
    y = R.own_labels(m, x, lengths)
    grid = candidate_grid(256.0, counts=(9, 1, 1))
    pick, ms, zs = R.worst_of_grid(m, x, lengths, grid, y)
    best = ms[np.arange(len(x)), pick]
    flipped = int((best < 0).sum())
    print(f"float64 worst-of-grid, +-256 positions, 9 delays: {flipped} of {len(x)} labels flip; smallest |margin| {np.abs(ms).min():.3e}")
    assert len(x) / 4 <= flipped < len(x)
    assert np.abs(ms).min() >= 1e-3
    assert np.array_equal(ms[:, 4], [R.margin(zs[b, 4], y[b]) for b in range(len(x))]) and np.all(ms[:, 4] > 0)  # the identity
    # a 3-delay grid, then two steps of the float64 refinement: at least one margin falls strictly
    grid3 = candidate_grid(256.0, counts=(3, 1, 1))
    pick3, ms3, _ = R.worst_of_grid(m, x[:6], lengths[:6], grid3, y[:6])
    lo, hi, step = np.array([-256.0, 1.0, 1.0]), np.array([256.0, 1.0, 1.0]), np.array([64.0, 0.0, 0.0])
    fell = 0
    for b in range(6):
        start = ms3[b, pick3[b]]
        _, got = R.refine(m, x[b], int(R.positions(lengths)[b]), grid3[pick3[b]], y[b], lo, hi, step, 2)
        assert got <= start
        fell += got < start
    assert fell >= 1


def test_candidate_grid():
    from lipasr.warp import candidate_axes, candidate_grid

    g = candidate_grid(100.0, 1.1, 3.0)
    assert g.shape == (81, 3) and g.dtype == np.float64
    s, r, a = candidate_axes(100.0, 1.1, 3.0)
    assert np.array_equal(s, np.linspace(-100, 100, 9)) and len(r) == len(a) == 3
    assert np.allclose(np.log(r), np.linspace(-math.log(1.1), math.log(1.1), 3), atol=1e-15)
    assert np.allclose(20 * np.log10(a), [-3.0, 0.0, 3.0], atol=1e-13)
    assert np.array_equal(g[40], [0.0, 1.0, 1.0])  # the identity, the middle candidate
    for i in range(9):  # the shift slowest, the gain fastest
        for j in range(3):
            for k in range(3):
                assert np.array_equal(g[(i * 3 + j) * 3 + k], [s[i], r[j], a[k]])
    assert np.array_equal(s, -s[::-1]) and np.allclose(r * r[::-1], 1.0, atol=1e-15) and np.allclose(a * a[::-1], 1.0, atol=1e-15)
    assert candidate_grid(0.0, counts=(1, 1, 1)).tolist() == [[0.0, 1.0, 1.0]]
    for counts in [(8, 3, 3), (9, 2, 3), (9, 3, 4), (0, 1, 1), (9, 3)]:
        with pytest.raises(ValueError):
            candidate_grid(10.0, 1.1, 1.0, counts=counts)
    with pytest.raises(ValueError):
        candidate_grid(-1.0)
    with pytest.raises(ValueError):
        candidate_grid(1.0, 0.9)


def test_refusals():
    n, K, b = 16, 2, 2
    x = np.zeros((b, n), np.float32)
    params = np.tile(f32([IDENT]), (b * K, 1))
    table = np.stack(N.warp_table_host(), axis=1).copy()
    out = np.zeros((b * K, n), np.float32)
    g = np.zeros((b * K, n), np.float32)
    gp = np.zeros((b * K, 3), np.float64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    ap, vj = N.lib.lipasr_warp_apply_host, N.lib.lipasr_warp_param_vjp_host
    assert ap(p(x), None, p(params), p(table), b, K, n, p(out)) == N.OK
    assert vj(p(x), p(g), None, p(params), p(table), b, K, n, p(gp)) == N.OK
    for args in [(None, None, p(params), p(table), b, K, n, p(out)), (p(x), None, None, p(table), b, K, n, p(out)),
                 (p(x), None, p(params), None, b, K, n, p(out)), (p(x), None, p(params), p(table), b, K, n, None),
                 (p(x), None, p(params), p(table), -1, K, n, p(out)), (p(x), None, p(params), p(table), b, K, (1 << 24) + 1, p(out)),
                 (p(x), None, p(params), p(table), 1, 1, n, p(x)),                       # out is x
                 (p(out), None, p(params), p(table), 1, 1, n, C.c_void_p(out.ctypes.data + 4 * (n - 1))),  # out meets x's last float
                 (p(x), None, p(out), p(table), 1, 1, n, p(out)), (p(x), None, p(params), p(out), 1, 1, n, p(out))]:
        assert ap(*args) == N.EINVAL, args
        assert N.lib.lipasr_warp_apply(*args, None) == N.EINVAL  # the device entry point refuses before it touches a device
    for args in [(None, p(g), None, p(params), p(table), b, K, n, p(gp)), (p(x), None, None, p(params), p(table), b, K, n, p(gp)),
                 (p(x), p(g), None, None, p(table), b, K, n, p(gp)), (p(x), p(g), None, p(params), None, b, K, n, p(gp)),
                 (p(x), p(g), None, p(params), p(table), b, K, n, None), (p(x), p(g), None, p(params), p(table), b, -2, n, p(gp)),
                 (p(x), p(g), None, p(params), p(table), b, K, n, p(g)), (p(x), p(g), None, p(params), p(table), b, K, n, p(x))]:
        assert vj(*args) == N.EINVAL, args
        assert N.lib.lipasr_warp_param_vjp(*args, None) == N.EINVAL
    # nothing to do: LIPASR_OK without a launch, whatever the pointers
    before = [N.lib.lipasr_debug_warp_launches(k) for k in (0, 1)]
    for shape in [(0, K, n), (b, 0, n), (b, K, 0)]:
        assert ap(None, None, None, None, *shape, None) == N.OK and N.lib.lipasr_warp_apply(None, None, None, None, *shape, None, None) == N.OK
        assert vj(None, None, None, None, None, *shape, None) == N.OK
        assert N.lib.lipasr_warp_param_vjp(None, None, None, None, None, *shape, None, None) == N.OK
    assert [N.lib.lipasr_debug_warp_launches(k) for k in (0, 1)] == before
    assert N.lib.lipasr_warp_table_host(None, None) == N.EINVAL
