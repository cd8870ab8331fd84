"""The universal perturbation without a GPU: the host twins lipasr_universal_{shifts,apply,reduce,step}_host (the CPU-side pin of
the counters and of the arithmetic the device kernels share with them) against the NumPy restatement of tests/universal_ref.py,
every refusal of the ABI, the surface of lipasr.universal, and two known answers on the restatement's driver over the oracle.

Bounds.  shifts, apply, reduce and step under norm inf are integer arithmetic, single fp32 additions, clamps and fp64 additions in
a stated order: every comparison is of bits.  step under norm 2 is fp64 arithmetic rounded once to fp32, with two sums whose
order is the implementation's: against the float64 restatement it is held to 8 x the worst error, over the cases of a shape, of
the SAME restatement run in float32 (no floor).  Measured: the host twin's worst error per shape is 6e-9 to 3e-8 -- its one
rounding to float32 -- against 1e-8 to 4e-8 for the float32 restatement: 0.03 to 0.125 of the bound is used (printed per shape;
0.125 where the rounding of the result is all the error either side has).
"""
import ctypes as C
import math

import numpy as np
import pytest

import universal_ref as R
from philox_ref import philox

# (batch, n, P): P == n; P < n dividing and not; P > n; P == 1; batches on both sides of the group edge
SHAPES = [(1, 1, 1), (63, 5, 5), (64, 36, 12), (65, 101, 7), (130, 36, 50), (3, 1030, 1), (2, 1030, 1030), (130, 101, 101), (5, 5, 1030),
          (65, 1030, 257)]
ids = lambda s: "x".join(map(str, s))
INF = math.inf


def _N():
    from lipasr import _native as N

    return N


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_but_nan(a, b):
    """Bit for bit, a NaN matching any NaN (the payload of fl(NaN + y) is the adder's business)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and (nan == np.isnan(b)).all() and same(np.where(nan, 0, a), np.where(nan, 0, b))


def rows(B, n, seed, scale=0.3):
    return (scale * np.random.default_rng(seed).standard_normal((B, n))).astype(np.float32)


def ragged(B, n):
    return np.array(([0, 1, n, n + 3, -2, n // 2, n - 1] * (B // 7 + 1))[:B], dtype=np.int32)


def offsets(B, P, seed):
    """The cases of ``offs``: None, zeros, P - 1, drawn, and values outside [0, P) that the kernels must reduce."""
    wild = np.array(([-1, P, -P - 1, 3 * P + 2, 0] * (B // 5 + 1))[:B], dtype=np.int32)
    return {"none": None, "zero": np.zeros(B, dtype=np.int32), "last": np.full(B, P - 1, dtype=np.int32),
            "drawn": R.shifts(B, P, 3, seed), "wild": wild}


def cases(shape):
    """(name, offs, n_valid) over the cases of a shape."""
    B, n, P = shape
    for name, offs in offsets(B, P, 7 + sum(shape)).items():
        for nv_name, nv in (("whole", None), ("ragged", ragged(B, n))):
            yield f"{name}-{nv_name}", offs, nv


# ---------------------------------------------------------------------------------------------------------------- shifts
def test_shifts_are_the_philox_draw():
    N = _N()
    for P in (1, 2, 7, 880, 22050, 1 << 17):
        got = N.universal_shifts_host(70, P, 5, 0x1234567890ABCDEF, clip0=9)
        want = np.array([(philox(0x1234567890ABCDEF, 9 + b, 5, 0x554E4956)[0] * P) >> 32 for b in range(70)], dtype=np.int32)
        assert same(got, want) and same(got, R.shifts(70, P, 5, 0x1234567890ABCDEF, clip0=9))
        assert (got >= 0).all() and (got < P).all()
    whole = N.universal_shifts_host(130, 1000, 2, 11)
    parts = np.concatenate([N.universal_shifts_host(b, 1000, 2, 11, clip0=c) for c, b in ((0, 1), (1, 63), (64, 66))])
    assert same(whole, parts)
    for kw in (dict(it=3), dict(seed=12)):  # the iteration and the seed are part of the counter
        args = dict(it=2, seed=11)
        args.update(kw)
        assert (N.universal_shifts_host(130, 1000, args["it"], args["seed"]) != whole).mean() > 0.9
    assert (N.universal_shifts_host(129, 1000, 2, 11, clip0=1) == whole[1:]).all()
    seven = N.universal_shifts_host(4096, 7, 0, 1)
    counts = np.bincount(seven, minlength=7)
    assert (counts > 0).all() and len(counts) == 7
    q = 1.0 / 7
    assert (np.abs(counts / 4096 - q) <= 5 * math.sqrt(q * (1 - q) / 4096)).all(), counts  # 5-sigma binomial


# ---------------------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_apply_matches_the_restatement(shape):
    N = _N()
    B, n, P = shape
    x, noise = rows(B, n, 1), rows(1, P, 2, 0.2)[0]
    x[0, 0] = math.nan
    x[-1, -1] = -math.nan
    for name, offs, nv in cases(shape):
        for lo, hi in ((-INF, INF), (-0.25, 0.3)):
            got = N.universal_apply_host(x, noise, offs=offs, n_valid=nv, clip_lo=lo, clip_hi=hi)
            assert same_but_nan(got, R.apply(x, noise, offs, nv, lo, hi)), (name, lo)
            keep = np.arange(n)[None, :] >= (np.full(B, n) if nv is None else np.clip(nv, 0, n))[:, None]
            assert same(got[keep], x[keep]), name  # the padding keeps x's bits, a NaN's included
            inside = got[~keep & ~np.isnan(got)]
            assert lo == -INF or (inside.size == 0 or (inside.min() >= np.float32(lo) and inside.max() <= np.float32(hi)))
    assert np.isnan(N.universal_apply_host(x, noise, clip_lo=-1.0, clip_hi=1.0)[0, 0])  # a NaN stays through the clamp


def test_apply_pairs_position_k_with_noise_k_plus_off():
    N = _N()
    x = np.zeros((3, 7), dtype=np.float32)
    noise = np.arange(1, 6, dtype=np.float32)  # P = 5 < n = 7: the snippet loops
    got = N.universal_apply_host(x, noise, offs=np.array([0, 2, 4], dtype=np.int32))
    assert got.tolist() == [[1, 2, 3, 4, 5, 1, 2], [3, 4, 5, 1, 2, 3, 4], [5, 1, 2, 3, 4, 5, 1]]
    wide = np.arange(1, 11, dtype=np.float32)  # P = 10 > n = 7: a window
    assert N.universal_apply_host(x[:1], wide, offs=np.array([6], dtype=np.int32)).tolist() == [[7, 8, 9, 10, 1, 2, 3]]


# ---------------------------------------------------------------------------------------------------------------- reduce
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_reduce_matches_the_restatement(shape):
    N = _N()
    B, n, P = shape
    g = rows(B, n, 3, 1.0) * np.float32(10.0) ** np.random.default_rng(4).integers(-6, 6, (B, n)).astype(np.float32)
    g[0, 0] = math.nan
    g[-1, n // 2] = math.nan
    for name, offs, nv in cases(shape):
        sums = np.full(((B + 63) // 64, P), 7.0)
        got = N.universal_reduce_host(g, P, offs=offs, n_valid=nv, sums=sums)
        assert same(got, R.reduce(g, P, offs, nv)), name
        assert np.isfinite(got).all()  # a NaN counts as 0
    clean = np.where(np.isnan(g), np.float32(0), g)
    assert same(N.universal_reduce_host(clean, P), N.universal_reduce_host(g, P))


def test_reduce_is_the_adjoint_of_the_broadcast_and_cuts_at_the_group():
    N = _N()
    g = rows(130, 36, 5, 1.0)
    for P in (36, 50):  # P >= n, zero shifts, no lengths: the rows themselves, summed per group in ascending order
        got = N.universal_reduce_host(g, P)
        want = np.zeros((3, P))
        for b in range(130):
            want[b // 64, :36] += g[b].astype(np.float64)
        assert same(got, want)
    offs, nv = R.shifts(130, 12, 0, 5), ragged(130, 36)
    whole = N.universal_reduce_host(g, 12, offs=offs, n_valid=nv)
    head = N.universal_reduce_host(g[:64], 12, offs=offs[:64], n_valid=nv[:64])
    tail = N.universal_reduce_host(g[64:], 12, offs=offs[64:], n_valid=nv[64:])
    assert same(whole, np.concatenate([head, tail]))
    # <apply(0, noise), g> = <noise, reduce(g)>: the pairing of positions is the same on the way in and on the way back
    noise = rows(1, 12, 6)[0]
    xa = N.universal_apply_host(np.zeros_like(g), noise, offs=offs, n_valid=nv).astype(np.float64)
    lhs, rhs = (xa * g).sum(), (noise.astype(np.float64) * whole.sum(axis=0)).sum()
    assert abs(lhs - rhs) <= 1e-12 * np.abs(xa * g).sum()


# ---------------------------------------------------------------------------------------------------------------- step
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_step_inf_matches_the_restatement(shape):
    N = _N()
    B, n, P = shape
    groups = (B + 63) // 64
    sums = np.random.default_rng(8).standard_normal((groups, P))
    sums[:, ::3] = 0.0
    if P > 4:
        sums[0, 1], sums[0, 2], sums[-1, 4] = INF, -INF, math.nan
    if groups > 1 and P > 7:
        sums[0, 7], sums[1, 7] = 1.5, -1.5  # cancels: sign 0
    noise0 = rows(1, P, 9, 0.1)[0]
    noise0[0] = -0.0
    for alpha in (0.05, -0.05, 0.0):
        for eps in (0.12, 0.0, INF):
            got = N.universal_step_host(noise0.copy(), sums, np.inf, alpha, eps)
            assert same(got, R.step(noise0, sums, np.inf, alpha, eps)), (alpha, eps)
            if eps < INF:
                assert np.abs(got).max() <= np.float32(eps)
    moved = N.universal_step_host(np.zeros(P, dtype=np.float32), sums, np.inf, 0.25, INF)
    G = R.total(sums)
    with np.errstate(invalid="ignore"):
        assert same(moved, (np.float32(0.25) * np.sign(np.nan_to_num(G, nan=0.0))).astype(np.float32) + np.float32(0))


def step2_cases(shape):
    """(noise, sums, alpha, eps) over the cases of a shape under norm 2."""
    B, n, P = shape
    groups = (B + 63) // 64
    rng = np.random.default_rng(10 + sum(shape))
    for k, (alpha, eps, scale) in enumerate(((0.3, 0.5, 1.0), (-0.3, 0.5, 1e-3), (0.7, INF, 40.0), (0.2, 0.05, 1.0), (0.0, 0.1, 1.0))):
        sums = scale * rng.standard_normal((groups, P))
        noise = (0.2 * rng.standard_normal(P)).astype(np.float32)
        yield noise, sums, alpha, eps


def step2_errors(run, shape):
    """(worst |run - float64 restatement|, worst |float32 restatement - float64 restatement|) over the cases of a shape."""
    err = yard = 0.0
    for noise, sums, alpha, eps in step2_cases(shape):
        want = R.step(noise, sums, 2, alpha, eps)
        got = run(noise.copy(), sums, alpha, eps)
        assert got.dtype == np.float32
        err = max(err, float(np.abs(got.astype(np.float64) - want).max()))
        yard = max(yard, float(np.abs(R.step(noise, sums, 2, alpha, eps, dtype=np.float32).astype(np.float64) - want).max()))
        if eps < INF:
            assert np.linalg.norm(got.astype(np.float64)) <= eps * (1 + 1e-6)
    return err, yard


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_step_2_within_the_float32_yardstick(shape):
    N = _N()
    err, yard = step2_errors(lambda noise, sums, alpha, eps: N.universal_step_host(noise, sums, 2, alpha, eps), shape)
    print(f"step norm 2 {ids(shape)}: worst error {err:.3e}, float32 restatement {yard:.3e}, ratio of the bound used {err / (8 * yard) if yard else 0:.3f}")
    assert err <= 8 * yard


def test_step_2_conventions():
    N = _N()
    noise0 = np.array([0.3, -0.4, 0.0, 0.0], dtype=np.float32)
    sums = np.array([[3.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    got = N.universal_step_host(noise0.copy(), sums, 2, 0.5, INF)  # a step of length alpha along G / |G|, no projection
    np.testing.assert_allclose(got, [0.6, -0.4, 0.4, 0.0], rtol=1e-6)
    got = N.universal_step_host(noise0.copy(), sums, 2, -0.5, INF)  # alpha < 0 descends
    np.testing.assert_allclose(got, [0.0, -0.4, -0.4, 0.0], rtol=1e-6, atol=1e-7)
    got = N.universal_step_host(noise0.copy(), sums, 2, 0.5, 0.25)
    assert abs(np.linalg.norm(got.astype(np.float64)) - 0.25) <= 1e-6
    for bad in (INF, -INF, math.nan):  # a non-finite N takes no step and only projects
        s = sums.copy()
        s[1, 3] = bad
        assert same(N.universal_step_host(noise0.copy(), s, 2, 0.5, INF), noise0)
        got = N.universal_step_host(noise0.copy(), s, 2, 0.5, 0.25)
        np.testing.assert_allclose(got, noise0 * 0.5, rtol=1e-6)
        assert same(got, R.step(noise0, s, 2, 0.5, 0.25).astype(np.float32))
    zero = N.universal_step_host(np.zeros(4, dtype=np.float32), np.zeros((1, 4)), 2, 0.5, 0.25)  # G = 0: 0 / 1e-7
    assert same(zero, np.zeros(4, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_abi_argument_checks_without_a_device():
    N = _N()
    names = ("shifts", "apply", "reduce", "step")
    assert N.lib.lipasr_version() >= 700 and N.UNIVERSAL_GROUP == 64
    assert all(N.has(f"lipasr_universal_{k}{s}") and N.SINCE[f"lipasr_universal_{k}{s}"] == 700 for k in names for s in ("", "_host"))
    assert [len(getattr(N.lib, f"lipasr_universal_{k}").argtypes) for k in names] == [8, 12, 9, 9]
    assert [len(getattr(N.lib, f"lipasr_universal_{k}_host").argtypes) for k in names] == [6, 10, 7, 7]
    fake = C.c_void_p(8)
    buf = np.zeros(512, dtype=np.float32)
    at = lambda k: C.c_void_p(buf.ctypes.data + 4 * k)
    dbl = np.zeros(256, dtype=np.float64)
    dp = lambda k=0: C.c_void_p(dbl.ctypes.data + 8 * k)
    ints = np.zeros(64, dtype=np.int32)
    ip = C.c_void_p(ints.ctypes.data)
    L = N.lib

    def shifts(host, h=fake, B=2, P=5, out=ip):
        return L.lipasr_universal_shifts_host(B, P, 0, 0, 0, out) if host else L.lipasr_universal_shifts(h, B, P, 0, 0, 0, out, None)

    def apply(host, h=fake, B=2, n=21, P=5, lo=-INF, hi=INF, x=at(0), noise=at(100), offs=None, nv=None, out=at(50)):
        if host:
            return L.lipasr_universal_apply_host(x, noise, offs, nv, B, n, P, lo, hi, out)
        return L.lipasr_universal_apply(h, x, noise, offs, nv, B, n, P, lo, hi, out, None)

    def reduce(host, h=fake, B=2, n=21, P=5, g=at(0), offs=None, nv=None, sums=dp()):
        return L.lipasr_universal_reduce_host(g, offs, nv, B, n, P, sums) if host else L.lipasr_universal_reduce(h, g, offs, nv, B, n, P, sums, None)

    def step(host, h=fake, groups=2, P=5, norm=INF, alpha=0.1, eps=0.2, noise=at(0), sums=dp()):
        return L.lipasr_universal_step_host(noise, sums, groups, P, norm, alpha, eps) if host else \
            L.lipasr_universal_step(h, noise, sums, groups, P, norm, alpha, eps, None)

    big = (1 << 17) + 1
    overlap_d = C.c_void_p(buf.ctypes.data + 16)  # doubles laid over the floats
    table = {
        shifts: ("lipasr_universal_shifts", ((dict(B=-1), "bad shape"), (dict(P=-1), "bad shape"), (dict(B=65536), "65536 rows"),
                                             (dict(P=big), "period 131073"), (dict(out=None), "a null pointer")),
                 (dict(B=0, out=None), dict(P=0, out=None))),
        apply: ("lipasr_universal_apply", ((dict(B=-1), "bad shape"), (dict(n=-1), "bad shape"), (dict(P=-1), "bad shape"),
                                           (dict(B=65536), "65536 rows"), (dict(n=big), "rows of 131073"), (dict(P=big), "period 131073"),
                                           (dict(x=None), "a null pointer"), (dict(noise=None), "a null pointer"), (dict(out=None), "a null pointer"),
                                           (dict(lo=1.0, hi=-1.0), "clip range"), (dict(lo=math.nan), "clip range"),
                                           (dict(out=at(41)), "out overlaps x"), (dict(out=at(0)), "out overlaps x"),
                                           (dict(out=at(100 - 41)), "out overlaps noise"), (dict(out=at(104)), "out overlaps noise")),
                (dict(B=0, x=None, noise=None, out=None), dict(n=0, x=None, noise=None, out=None), dict(P=0, x=None, noise=None, out=None))),
        reduce: ("lipasr_universal_reduce", ((dict(B=-1), "bad shape"), (dict(n=-1), "bad shape"), (dict(P=-1), "bad shape"),
                                             (dict(B=65536), "65536 rows"), (dict(n=big), "rows of 131073"), (dict(P=big), "period 131073"),
                                             (dict(g=None), "a null pointer"), (dict(sums=None), "a null pointer"),
                                             (dict(sums=overlap_d), "sums overlaps g")),
                 (dict(B=0, g=None, sums=None), dict(n=0, g=None, sums=None), dict(P=0, g=None, sums=None))),
        step: ("lipasr_universal_step", ((dict(groups=-1), "bad shape"), (dict(P=-1), "bad shape"), (dict(groups=1025), "1025 groups"),
                                         (dict(P=big), "period 131073"), (dict(norm=1.0), "norm 1"), (dict(norm=math.nan), "norm"),
                                         (dict(norm=-INF), "norm"), (dict(alpha=INF), "alpha"), (dict(alpha=math.nan), "alpha"),
                                         (dict(eps=-0.1), "eps -0.1"), (dict(eps=math.nan), "eps"), (dict(noise=None), "a null pointer"),
                                         (dict(sums=None), "a null pointer"), (dict(sums=overlap_d), "noise overlaps sums")),
               (dict(groups=0, noise=None, sums=None), dict(P=0, noise=None, sums=None))),
    }
    for fn, (name, refused, empty) in table.items():
        for host in (False, True):
            full = name + ("_host:" if host else ":")
            for kw, msg in refused + (() if host else ((dict(h=None), "null handle"),)):
                assert fn(host, **kw) == N.EINVAL, (full, kw)
                assert msg in N.last_error() and N.last_error().startswith(full), (kw, N.last_error())
            for kw in empty:
                assert fn(host, **kw) == N.OK, (full, kw)
            assert fn(True) == N.OK  # the same arguments untouched are accepted (host side: it runs)
    for norm in (2.0, INF):
        assert step(True, norm=norm) == N.OK
    with pytest.raises(ValueError, match="out overlaps x"):  # through the NumPy wrapper
        one = np.zeros((2, 21), dtype=np.float32)
        N.universal_apply_host(one, np.zeros(5, dtype=np.float32), out=one)


def test_empty_calls_write_nothing():
    N = _N()
    sums = np.full((1, 5), 7.0)
    N.universal_reduce_host(np.zeros((2, 0), dtype=np.float32), 5, sums=sums)
    assert (sums == 7.0).all()
    out = np.full((2, 3), 7.0, dtype=np.float32)
    N.check(N.lib.lipasr_universal_apply_host(None, None, None, None, 2, 3, 0, -INF, INF, C.c_void_p(out.ctypes.data)))
    assert (out == 7.0).all()


def test_universal_perturbation_is_exported_and_checks_its_arguments():
    import inspect

    from lipasr import attack_eval as V, attacks as A, universal as U

    assert A.UniversalPerturbation is U.UniversalPerturbation and callable(V.universal_sweep)
    assert all(callable(getattr(U, f"universal_{k}")) for k in ("shifts", "apply", "reduce", "step"))
    sig = inspect.signature(U.UniversalPerturbation.__init__)
    assert list(sig.parameters)[1:] == ["estimator", "attacker", "delta", "max_iter", "eps", "eps_step", "norm", "batch_size", "targeted",
                                        "length", "random_shift", "seed", "clip_values"]
    for k, d in (("attacker", "pgd"), ("delta", 0.2), ("max_iter", 20), ("eps", 10.0), ("eps_step", None), ("norm", np.inf), ("batch_size", 32),
                 ("targeted", False), ("length", None), ("random_shift", False), ("seed", None)):
        assert sig.parameters[k].default == d or sig.parameters[k].default is d, k
    assert list(inspect.signature(U.UniversalPerturbation.generate_device).parameters)[1:] == ["xt", "yt", "lengths"]
    assert list(inspect.signature(U.UniversalPerturbation.generate).parameters)[1:] == ["x", "y", "lengths"]
    assert list(inspect.signature(U.UniversalPerturbation.apply).parameters)[1:] == ["x", "lengths", "offs"]
    with pytest.raises(TypeError):
        U.UniversalPerturbation(object())
    doc = U.UniversalPerturbation.__doc__
    assert "Shafahi" in doc and "Mummadi" in doc and "DeepFool" in doc and "cannot be batched" in doc


def test_menu_accepts_universal(tmp_path):
    from lipasr import attack_eval as V

    missing = str(tmp_path) + "/missing/"
    for over in ("mfcc", "audio"):
        for extra in ([], ["--norm", "2"], ["--shift", "--length", "100", "--max-iter", "2"]):
            with pytest.raises(FileNotFoundError):
                V.main(["--attack", "white", "--kind", "universal", "--over", over, "--points", "1", "--path", missing] + extra)
    with pytest.raises(FileNotFoundError):
        V.main(["--attack", "white", "--kind", "universal", "--over", "audio", "--room", "2", "--points", "1", "--path", missing])
    with pytest.raises(ValueError, match="--kind universal runs in --norm inf or 2"):
        V.main(["--attack", "white", "--kind", "universal", "--norm", "1", "--path", missing])
    with pytest.raises(ValueError, match="--shift and --length go with --kind universal"):
        V.main(["--attack", "white", "--kind", "pgd", "--shift", "--path", missing])


# ---------------------------------------------------------------------------------------------------------------- known answers
def oracle_model(spec, p):
    """(grad, predict, ce) of the float64 oracle: d CE / dx as float32 rows, logits, and the mean cross-entropy."""
    from oracle import mlp_ref as P

    p64 = p.astype(np.float64)
    C_ = spec[-1].n_out
    onehot = lambda y: np.eye(C_)[np.asarray(y)]
    grad = lambda xa, y: P.input_gradient_infer(spec, p64, np.asarray(xa, dtype=np.float64), onehot(y)).astype(np.float32)
    predict = lambda xa: P.forward_infer(spec, p64, np.asarray(xa, dtype=np.float64), return_logits=True)

    def ce(xa, y):
        prob = P.forward_infer(spec, p64, np.asarray(xa, dtype=np.float64))
        return float(-np.log(prob[np.arange(len(y)), y]).mean())

    return grad, predict, ce


def linear_rows():
    """The one-layer two-class model of test_apgd_cpu.linear_model and its rows of class 0 -> (spec, p, x, w_other - w_own, eps):
    eps is half the smallest L-inf distance of those rows to the boundary, so that no noise in the ball fools a row (Hoelder) and
    the fit runs all its epochs."""
    from test_apgd_cpu import linear_model

    spec, p, x, cls, w, d, _ = linear_model()
    own = cls == 0
    assert own.sum() >= 2
    return spec, p, x[own], w[own][0], 0.5 * float(d[own].min())


def test_known_answer_linear_one_class():
    """CE of a linear two-class model has the gradient p_other (w_other - w_own) on every row of class `own`, p_other > 0: every
    minibatch steps by eps_step sign(w_other - w_own), and once eps_step x (minibatches x max_iter) >= eps the clamp leaves
    float32(eps) sign(w_other - w_own) exactly."""
    spec, p, x, w, eps = linear_rows()
    grad, predict, _ = oracle_model(spec, p)
    labels = np.zeros(len(x), dtype=np.int64)
    assert (predict(x).argmax(axis=1) == 0).all()
    batches = -(-len(x) // 2)
    r = R.fit(grad, predict, x, labels, eps, eps / 4, max_iter=-(-4 // batches) + 1, batch_size=2, delta=0.0)
    assert (eps / 4) * batches * r["epochs"] >= eps and not r["converged"] and r["fooling_rate"] == 0.0
    nz = w != 0
    assert nz.sum() > 800 and same(r["noise"][nz], (np.float32(eps) * np.sign(w[nz])).astype(np.float32))


HELD = dict(eps=0.2, eps_step=0.04, max_iter=10, batch_size=32, delta=0.0, clip=(-2.0, 2.0))


def held_out_case():
    from local_lip_ref import setup_params
    from oracle import mlp_ref as P

    spec = P.vd_unconstrained_spec()
    p = setup_params(spec, 3)
    x = np.clip(np.random.default_rng(11).standard_normal((128, 880)), -2, 2).astype(np.float32)
    return spec, p, x[:64], x[64:]


def random_sign_rates(predict, held, own):
    """The held-out fooling rates of the eight random sign vectors eps sign(N(0, 1)), seeds 0 .. 7."""
    rates = []
    for k in range(8):
        v = (np.float32(HELD["eps"]) * np.sign(np.random.default_rng(k).standard_normal(880))).astype(np.float32)
        rates.append(float((np.asarray(predict(R.apply(held, v, lo=HELD["clip"][0], hi=HELD["clip"][1]))).argmax(axis=1) != own).mean()))
    return rates


def test_known_answer_held_out_generalisation():
    """A noise fitted on 64 rows fools MORE of 64 rows it never saw than any of eight random sign vectors of the same L-inf norm,
    and the mean cross-entropy of the fitting rows rises.  On the float64 oracle: held-out fooling rate 0.78 against a largest
    random 0.23; cross-entropy 1.51 -> 2.14."""
    spec, p, fit_rows, held = held_out_case()
    grad, predict, ce = oracle_model(spec, p)
    own_fit, own_held = predict(fit_rows).argmax(axis=1), predict(held).argmax(axis=1)
    lo, hi = HELD["clip"]
    r = R.fit(grad, predict, fit_rows, own_fit, HELD["eps"], HELD["eps_step"], HELD["max_iter"], HELD["batch_size"], delta=HELD["delta"],
              lo=lo, hi=hi)
    assert np.abs(r["noise"]).max() <= np.float32(HELD["eps"])
    rate = float((predict(R.apply(held, r["noise"], lo=lo, hi=hi)).argmax(axis=1) != own_held).mean())
    random = random_sign_rates(predict, held, own_held)
    ce0, ce1 = ce(fit_rows, own_fit), ce(R.apply(fit_rows, r["noise"], lo=lo, hi=hi), own_fit)
    print(f"held-out fooling rate {rate:.3f} against random sign vectors {max(random):.3f} (all: {random}); fitting rows: fooling rate "
          f"{r['fooling_rate']:.3f}, mean CE {ce0:.3f} -> {ce1:.3f}")
    assert rate > max(random)
    assert ce1 > ce0
