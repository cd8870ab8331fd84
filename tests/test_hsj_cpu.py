"""HopSkipJump without a GPU: the four host twins (lipasr_hsj_*_host, the CPU-side pin of the counters and of the arithmetic the
device kernels share with them) against the NumPy restatement of tests/hsj_ref.py, every refusal of the ABI, the surface of
lipasr.hopskipjump, and the restatement's own answer on a linear two-class model.

Bounds.  Bits: the L-inf copies of expand, both sums and both counts of accumulate (one call, and split 1 + 2 + rest), sign(g), and
every array of the search except the two L2 distances.  One unit in the last place of float32: the L2 direction and the L2
distance -- the twin adds squares serially in fp64, NumPy pairwise: n 2^-52 relative, far below 2^-24.  The L2 copies of expand
depend on the libm's logf / sinf / cosf: against the float64 restatement the bound is 8 x the worst error of a float32 NumPy
restatement against that same float64 one over the cases of the shape, the form the psychoacoustic tests use (no floor).

The linear model.  On sign(w x + b) the true distance is |w x + b| / ||w||_2 (L2) and / ||w||_1 (L-inf).  With n = 36, 12 rows,
max_iter 10, init_eval 100, max_eval 1000 and the seeds below the restatement reaches, over all rows, a worst distance / true of
R = 1.0208 (L2) and R = 1.0812 (L-inf), both rounded up, improves on its start on every row and never goes below the true distance; the iterate's
own distance goes up between two iterations on 9 (L2) and 11 (L-inf) of the 12 rows."""
import inspect
import math

import numpy as np
import pytest

import hsj_ref as R

SHAPES = [(1, 1), (1, 5), (2, 36), (3, 880), (2, 1030), (1, 22050)]
NORMS = [2, np.inf]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
LIN_SEED = {2: 3, np.inf: 3}
LIN_R = {2: 1.0208, np.inf: 1.0812}  # measured by test_restatement_on_a_linear_model (printed there), rounded up in the last digit


def _N():
    from lipasr import _native as N

    return N


def rows(B, n, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((B, n))).astype(np.float32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def within_one_ulp(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
    with np.errstate(invalid="ignore"):
        return bool((both_inf | (np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))).all())


def n_valid_cases(B, n):
    """Lists of B lengths that between them hold 0, 1, 5, n - 1, n, n + 3 and -2."""
    values = [0, 1, 5, n - 1, n, n + 3, -2]
    return [(values[s:] + values)[:B] for s in range(0, len(values), B)]


def logits_for(B, draws, C, labels, seed, share=0.5):
    """Hand-made logits [B * draws, C]: about ``share`` of the rows adversarial, one NaN row and one tie where there is room."""
    rng = np.random.default_rng(seed + 900)
    z = rng.standard_normal((B * draws, C)).astype(np.float32)
    keep = rng.random(B * draws) >= share
    lab = np.repeat(np.asarray(labels), draws)
    z[keep, lab[keep]] += 8.0
    if len(z) > 3:
        z[2, 0] = np.nan  # never adversarial
        z[3, :] = 1.0  # a tie: class 0 wins
    return z


# ------------------------------------------------------------------------------------------------------------------ the tools
def test_philox_and_fma_restatements():
    for seed, lo, hi, h0, h1 in [(0, 0, 0, 0, 0), (0x48534A0000000007, 5, 99, 3, R.TAG_LINF | 9), (2**64 - 1, 2**32 - 1, 7, 2**32 - 1, 1)]:
        assert [int(v) for v in R.philox_np(seed, lo, hi, h0, h1)] == R.philox(seed, lo | (hi << 32), h0, h1)
    from fractions import Fraction

    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    c[:500] = (-a[:500].astype(np.float64) * b[:500]).astype(np.float32)  # cancellation
    got = R.fmaf32(a, b, c)
    for k in range(0, 2000, 7):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo_, hi_ = np.nextafter(got[k], np.float32(-np.inf)), np.nextafter(got[k], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[k]))) <= min(abs(exact - Fraction(float(lo_))), abs(exact - Fraction(float(hi_))))
    a, b, c = (rng.standard_normal(300) for _ in range(3))
    c[:100] = -a[:100] * b[:100]
    got = R.fma64(a, b, c)
    for k in range(300):
        exact = Fraction(a[k]) * Fraction(b[k]) + Fraction(c[k])
        assert abs(exact - Fraction(got[k])) <= abs(exact - Fraction(float(np.nextafter(got[k], np.inf))))
        assert abs(exact - Fraction(got[k])) <= abs(exact - Fraction(float(np.nextafter(got[k], -np.inf))))


# ---------------------------------------------------------------------------------------------------------------------- expand
def expand_cases(shape):
    B, n = shape
    yield dict(draws=1), None
    yield dict(draws=3, clip0=5, draw0=2, clip_lo=-0.4, clip_hi=0.45), None
    if n <= 1030:
        yield dict(draws=100), None
    for nv in n_valid_cases(B, n):
        yield dict(draws=3), nv


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_expand_linf_host_twin_bit_for_bit(shape):
    N = _N()
    B, n = shape
    x = rows(B, n, 1 + n)
    delta = np.linspace(0.05, 0.3, B).astype(np.float32)
    for kw, nv in expand_cases(shape):
        got = N.hsj_expand_host(x, delta, kw["draws"], 4, 77, np.inf, n_valid=nv, **{k: v for k, v in kw.items() if k != "draws"})
        want = R.expand(x, delta, kw["draws"], 4, 77, np.inf, nv, kw.get("clip0", 0), kw.get("draw0", 0), kw.get("clip_lo", -np.inf),
                        kw.get("clip_hi", np.inf))
        assert same(got, want), (shape, kw, nv)
    # the copy is delta away in L2 (the clamp aside), and padding keeps the bits of x
    got = N.hsj_expand_host(x, delta, 3, 4, 77, np.inf).reshape(B, 3, n)
    dist = np.sqrt(((got.astype(np.float64) - x[:, None]) ** 2).sum(axis=2))
    assert np.allclose(dist, delta[:, None], rtol=1e-5, atol=1e-7 * math.sqrt(n))
    # chunks of draws and of clips reproduce one call
    whole = N.hsj_expand_host(x, delta, 5, 2, 9, np.inf)
    parts = np.concatenate([N.hsj_expand_host(x[b:b + 1], delta[b:b + 1], d, 2, 9, np.inf, clip0=b, draw0=d0)
                            for b in range(B) for d0, d in ((0, 2), (2, 3))])
    assert same(whole, parts)
    # an infinite delta (a row without a start) leaves the row alone
    assert same(N.hsj_expand_host(x, np.full(B, np.inf, dtype=np.float32), 1, 1, 0, np.inf), x)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_expand_l2_host_twin_against_float64(shape):
    N = _N()
    B, n = shape
    x = rows(B, n, 2 + n)
    delta = np.linspace(0.05, 0.3, B).astype(np.float32)
    cases = []  # (case, the twin's error, the float32 restatement's error), both against the float64 restatement
    for kw, nv in expand_cases(shape):
        if kw["draws"] > 3:
            continue
        args = (nv, kw.get("clip0", 0), kw.get("draw0", 0), kw.get("clip_lo", -np.inf), kw.get("clip_hi", np.inf))
        want = R.expand(x, delta, kw["draws"], 4, 77, 2, *args)
        f32_err = float(np.abs(R.expand(x, delta, kw["draws"], 4, 77, 2, *args, dtype=np.float32) - want).max())
        got = N.hsj_expand_host(x, delta, kw["draws"], 4, 77, 2, n_valid=nv, **{k: v for k, v in kw.items() if k != "draws"})
        cases.append(((kw, nv), float(np.abs(got - want).max()), f32_err))
        valid = np.arange(n)[None, :] < (np.full(B, n) if nv is None else np.clip(nv, 0, n))[:, None]
        assert same(got.reshape(B, -1, n)[~np.broadcast_to(valid[:, None], (B, kw["draws"], n))],
                    np.broadcast_to(x[:, None], (B, kw["draws"], n))[~np.broadcast_to(valid[:, None], (B, kw["draws"], n))])
    yard = max(c[2] for c in cases)  # the worst error of the float32 restatement over the cases of this shape
    print(f"{ids(shape)}: worst host twin {max(c[1] for c in cases):.3e}, float32 restatement {yard:.3e}, bound {8 * yard:.3e}")
    for case, err, _ in cases:
        assert err <= 8 * yard, (shape, case, err, yard)
    if n >= 880:  # the draws are standard normal: mean 0, variance 1 before the scaling (5 sigma)
        got = N.hsj_expand_host(x[:1], np.ones(1, dtype=np.float32), 20, 1, 5, 2)
        r = (got.astype(np.float64) - x[:1]) * math.sqrt(n)
        assert abs(r.mean()) < 5 / math.sqrt(r.size) and abs((r * r).mean() - 1) < 1e-6


# ------------------------------------------------------------------------------------------------- accumulate and direction
def workspace(B, n):
    return np.zeros((B, 2, n)), np.zeros((B, 2), dtype=np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_accumulate_and_direction_host_twins(shape):
    N = _N()
    B, n = shape
    x = rows(B, n, 3 + n)
    delta = np.full(B, 0.2, dtype=np.float32)
    for draws, C, targeted in ((1, 2, False), (3, 10, True), (100 if n <= 1030 else 7, 32, False)):
        labels = (np.arange(B) % C).astype(np.int32)
        for nv in [None] + (n_valid_cases(B, n) if draws == 3 else []):
            p = N.hsj_expand_host(x, delta, draws, 1, 5, np.inf, n_valid=nv)
            for share in (0.5, 0.0, 1.0):  # mixed, every phi -1, every phi +1 (the NaN row and the tie aside)
                z = logits_for(B, draws, C, labels, draws + C, share)
                if share != 0.5:
                    z = np.nan_to_num(z, nan=0.0)
                    z[np.arange(B * draws), np.repeat(labels, draws)] += -50.0 if (share == 1.0) != targeted else 50.0
                sums, counts = workspace(B, n)
                N.hsj_accumulate_host(z, labels, p, x, sums=sums, counts=counts, n_valid=nv, targeted=targeted)
                ws, wc = workspace(B, n)
                R.accumulate(z, labels, p, x, ws, wc, nv, targeted)
                assert same(sums, ws) and same(counts, wc), (shape, draws, C, nv, share)
                if share != 0.5:
                    assert (counts[:, 1] == (draws if share == 1.0 else 0)).all()
                if draws >= 3:  # the same draws split 1 + 2 + rest
                    ss, sc = workspace(B, n)
                    pr, zr = p.reshape(B, draws, n), z.reshape(B, draws, C)
                    for a, b in ((0, 1), (1, 3), (3, draws)):
                        if b > a:
                            N.hsj_accumulate_host(zr[:, a:b].reshape(-1, C), labels, pr[:, a:b].reshape(-1, n), x, sums=ss, counts=sc,
                                                  n_valid=nv, targeted=targeted)
                    assert same(ss, sums) and same(sc, counts)
                u_inf, g = R.direction(sums, counts, np.inf, nv)
                assert same(N.hsj_direction_host(sums, counts, np.inf, n_valid=nv), u_inf), (shape, draws, C, nv, share)
                u_2, _ = R.direction(sums, counts, 2, nv)
                got = N.hsj_direction_host(sums, counts, 2, n_valid=nv)
                assert within_one_ulp(got, u_2)
                nrm = np.sqrt((got.astype(np.float64) ** 2).sum(axis=1))
                assert (np.isclose(nrm, 1.0, atol=1e-6) | (np.abs(g).sum(axis=1) == 0)).all()
    # no draws at all: u = 0
    sums, counts = workspace(B, n)
    assert not N.hsj_direction_host(sums, counts, 2).any() and not N.hsj_direction_host(sums, counts, np.inf).any()


# ---------------------------------------------------------------------------------------------------------------------- search
def search_script(B, C, labels, seed, init=4, bisect=10, halve=4):
    """The calls of one chain over all three modes: (mode, flags, draw, logits or None, step_scale)."""
    def forced(z, adv):  # row b adversarial exactly where adv[b]
        z = np.nan_to_num(z, nan=0.0)
        z[np.arange(B), labels] = np.where(adv, -9.0, 9.0)
        return z

    calls = [(R.START, R.FIRST, 0, None, 1.0)]
    for k in range(init):  # row b finds its start at draw b % (init - 1): the LAST draw finds none
        calls.append((R.START, R.LAST if k + 1 == init else 0, k, forced(logits_for(B, 1, C, labels, seed + k), np.arange(B) % (init - 1) == k), 1.0))
    step = 0
    for rnd in range(2):
        calls.append((R.BISECT, R.FIRST, 0, None, 1.0))
        calls += [(R.BISECT, 0, 0, logits_for(B, 1, C, labels, seed + 100 * rnd + 10 + k), 1.0) for k in range(bisect)]
        if rnd == 0:
            calls.append((R.HALVE, R.FIRST, 0, None, 0.7))
            # row 0 never lands on the adversarial side and gives up; row b > 0 lands after b % 3 halvings
            calls += [(R.HALVE, 0, 0, forced(logits_for(B, 1, C, labels, seed + 50 + k), (np.arange(B) > 0) & (np.arange(B) % 3 == k)), 0.7)
                      for k in range(halve)]
        step += 1
    return calls


def search_setup(shape, norm, seed, nv, C=4, clip=(-np.inf, np.inf)):
    B, n = shape
    x0 = np.clip(rows(B, n, seed), *clip).astype(np.float32)
    lo, hi = max(clip[0], -0.8), min(clip[1], 0.9)  # the start draws stay inside the clip range, as the attack has them
    labels = (np.arange(B) % C).astype(np.int32)
    rng = np.random.default_rng(seed + 1)
    u = rng.standard_normal((B, n)).astype(np.float32)
    u = np.sign(u) if norm != 2 else (u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    d = np.maximum(np.full(B, n) if nv is None else np.clip(nv, 0, n), 1)
    theta = (0.3 / np.sqrt(d) if norm == 2 else 0.3 / d).astype(np.float32)
    attack = np.ones(B, dtype=bool)
    attack[B - 1] = B == 1  # with more than one row the last row is not attacked
    return dict(x0=x0, labels=labels, u=u, theta=theta, attack=attack, start_lo=np.full(B, lo, dtype=np.float32),
                start_hi=np.full(B, hi, dtype=np.float32))


STATE = ("x_cand", "x_far", "x_adv", "x_best", "f", "i")


def assert_state(got, want, l2, what):
    for k in STATE:
        if k == "f" and l2:
            assert same(got[k][:, :5], want[k][:, :5]) and same(got[k][:, 7], want[k][:, 7]), f"{what}: {k}"
            assert within_one_ulp(got[k][:, 5:7], want[k][:, 5:7]), f"{what}: dist {got[k][:, 5:7]} {want[k][:, 5:7]}"
        else:
            assert same(got[k], want[k]), f"{what}: {k} differs"


def host_search(st, z, s, mode, flags, draw, scale, norm, seed, nv, clip, max_halvings=3, clip0=2):
    _N().hsj_search_host(z, s["labels"], s["x0"], mode, flags, seed, norm, x_cand=st["x_cand"], x_far=st["x_far"], x_adv=st["x_adv"],
                         x_best=st["x_best"], fstate=st["f"], istate=st["i"], start_lo=s["start_lo"], start_hi=s["start_hi"],
                         theta=s["theta"], u=s["u"], n_valid=nv, clip0=clip0, draw=draw, step_scale=scale, max_halvings=max_halvings,
                         clip_lo=clip[0], clip_hi=clip[1], classes=4)


@pytest.mark.parametrize("norm", NORMS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_search_host_twin_against_the_restatement(shape, norm):
    B, n = shape
    seen = set()
    for nv, clip in [(None, (-np.inf, np.inf)), (None, (-0.5, 0.6))] + [(v, (-1.0, 1.0)) for v in n_valid_cases(B, n)]:
        seed = 21 + n
        s = search_setup(shape, norm, seed, nv, clip=clip)
        host = R.new_state(B, n, s["attack"])
        for k in ("x_cand", "x_far"):
            host[k][:] = 7.0  # junk: FIRST must not depend on it
        for step, (mode, flags, draw, z, scale) in enumerate(search_script(B, 4, s["labels"], seed)):
            ref = {k: v.copy() for k, v in host.items()}  # the restatement restarts from the twin's state
            host_search(host, z, s, mode, flags, draw, scale, norm, seed, nv, clip)
            R.search(ref, z, s["labels"], s["x0"], mode, flags, seed, norm, s["start_lo"], s["start_hi"], s["theta"], s["u"], nv, False, 2,
                     draw, scale, 3, *clip)
            if step == 0:
                for k in ("x_cand", "x_far"):
                    ref[k] = np.where(ref[k] == 7.0, host[k], ref[k])  # rows nobody writes keep the junk on both sides
            assert_state(host, ref, norm == 2, f"{ids(shape)} norm {norm} n_valid {nv} step {step} mode {mode} flags {flags}")
            valid = np.arange(n)[None, :] < (np.full(B, n) if nv is None else np.clip(nv, 0, n))[:, None]
            for k in ("x_cand", "x_adv", "x_best") + (("x_far",) if host["i"][:, 1].all() else ()):
                rows_ = host["i"][:, 1] != 0 if k == "x_far" else slice(None)
                assert same(host[k][rows_][~valid[rows_]], s["x0"][rows_][~valid[rows_]]), f"{k}: padding moved"
                assert host[k][rows_][valid[rows_]].min(initial=0) >= clip[0] and host[k][rows_][valid[rows_]].max(initial=0) <= clip[1]
            seen.update((mode, int(a), int(f), int(o)) for a, f, o in host["i"][:, :3])
        if B > 1:
            assert host["i"][B - 1, 5] == 0 and same(host["x_best"][B - 1], s["x0"][B - 1])  # the row that was not attacked
        q = host["i"][:, 5]
        assert (q[host["i"][:, 1] != 0] > 0).all()
    if B >= 3:  # the script reaches a start, a step that succeeds and a step that gives up
        assert {(R.START, 0, 1, 1), (R.HALVE, 0, 1, 1), (R.HALVE, 0, 1, 0)} <= seen, seen


def test_the_returned_iterate_is_a_queried_point():
    """After a bisection x_adv holds the bits of the last candidate the model called adversarial (or of the far point)."""
    for norm in NORMS:
        shape, seed = (2, 36), 8
        s = search_setup(shape, norm, seed, None)
        s["attack"][:] = True
        st = R.new_state(2, 36, s["attack"])
        clip = (-1.0, 1.0)
        last_adv = [None, None]
        for mode, flags, draw, z, scale in search_script(2, 4, s["labels"], seed)[:16]:
            cand_before, active = st["x_cand"].copy(), st["i"][:, 0].copy()
            host_search(st, z, s, mode, flags, draw, scale, norm, seed, None, clip)
            if z is not None:
                for b in range(2):
                    if active[b] and R.adversarial(z[b], int(s["labels"][b])):
                        last_adv[b] = cand_before[b]
        for b in range(2):
            if st["i"][b, 1] and not st["i"][b, 0]:
                assert same(st["x_adv"][b], last_adv[b])


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_abi_refusals_and_surface():
    N = _N()
    assert N.lib.lipasr_version() >= 670 and all(N.has(f"lipasr_hsj_{k}{t}") for k in ("expand", "accumulate", "direction", "search")
                                                 for t in ("", "_host"))
    assert [N.lib.lipasr_debug_hsj_path(n, 1) for n in (880, 2020, 8192, 16000, 22050, 24576, 24577, 30000)] == [65, 66, 72, 100, 38, 102, 0, 64]
    assert N.lib.lipasr_debug_hsj_path(880, 0) == 1 and N.lib.lipasr_debug_hsj_path(0, 1) == -1
    x, delta = rows(2, 8, 0), np.ones(2, dtype=np.float32)
    p = N.hsj_expand_host(x, delta, 3, 1, 0, 2)
    z, lab = logits_for(2, 3, 4, [0, 1], 0), np.array([0, 1], dtype=np.int32)
    sums, counts = workspace(2, 8)
    st = R.new_state(2, 8, [1, 1])
    s = dict(labels=lab, x0=x, u=np.zeros((2, 8), dtype=np.float32), theta=delta, start_lo=-delta, start_hi=delta)
    search = lambda **kw: N.hsj_search_host(kw.pop("z", z[:2]), lab, x, kw.pop("mode", R.BISECT), kw.pop("flags", 0), 0, kw.pop("norm", 2),
                                            **{**dict(x_cand=st["x_cand"], x_far=st["x_far"], x_adv=st["x_adv"], x_best=st["x_best"],
                                                      fstate=st["f"], istate=st["i"], start_lo=s["start_lo"], start_hi=s["start_hi"],
                                                      theta=s["theta"], u=s["u"]), **kw})
    search(mode=R.START, flags=R.FIRST)
    for bad in (lambda: N.hsj_expand_host(x, delta, 3, 1, 0, 1), lambda: N.hsj_expand_host(x, delta, 3, 1 << 24, 0, 2),
                lambda: N.hsj_expand_host(x, delta, -1, 1, 0, 2), lambda: N.hsj_expand_host(x, delta, 3, 1, 0, 2, clip_lo=1.0, clip_hi=-1.0),
                lambda: N.hsj_expand_host(x, delta[:1], 3, 1, 0, 2), lambda: N.hsj_expand_host(x, delta, 3, 1, 0, 2, out=p[:5]),
                lambda: N.hsj_expand_host(np.zeros((1, (1 << 17) + 1), dtype=np.float32), delta[:1], 1, 1, 0, np.inf),
                lambda: N.hsj_accumulate_host(logits_for(2, 3, 33, [0, 1], 0), lab, p, x, sums=sums, counts=counts),
                lambda: N.hsj_accumulate_host(z[:5], lab, p, x, sums=sums, counts=counts),
                lambda: N.hsj_accumulate_host(z, lab, p, x, sums=sums.astype(np.float32), counts=counts),
                lambda: N.hsj_accumulate_host(z, lab, p, x, sums=sums, counts=counts[:1]),
                lambda: N.hsj_accumulate_host(np.zeros((2 * 16385, 2), dtype=np.float32), lab, np.zeros((2 * 16385, 8), dtype=np.float32), x,
                                              sums=sums, counts=counts),
                lambda: N.hsj_direction_host(sums, counts, 1), lambda: N.hsj_direction_host(sums, counts[:1], 2),
                lambda: search(norm=1), lambda: search(mode=3), lambda: search(flags=4), lambda: search(max_halvings=0),
                lambda: search(step_scale=-1.0), lambda: search(step_scale=math.inf), lambda: search(clip_lo=1.0, clip_hi=0.0),
                lambda: search(z=None), lambda: search(z=logits_for(2, 1, 33, [0, 1], 0)), lambda: search(x_far=st["x_cand"]),
                lambda: search(x_best=st["x_adv"]), lambda: search(fstate=st["f"][:1]), lambda: search(mode=R.HALVE, u=None)):
        with pytest.raises(ValueError):
            bad()
    assert N.hsj_expand_host(x[:0], delta[:0], 3, 1, 0, 2).shape == (0, 8)  # nothing to do

    from lipasr import attacks
    from lipasr.hopskipjump import HopSkipJump

    assert attacks.HopSkipJump is HopSkipJump
    sig = inspect.signature(HopSkipJump.__init__)
    positional = [(k, p.default) for k, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD][1:]
    assert positional == [("classifier", inspect.Parameter.empty), ("batch_size", 64), ("targeted", False), ("norm", 2), ("max_iter", 50),
                          ("max_eval", 10000), ("init_eval", 100), ("init_size", 100), ("verbose", True)]
    keyword = {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert set(keyword) == {"seed", "clip_values", "gamma", "max_halvings", "check_every"} and keyword["gamma"] == 0.01 and keyword["seed"] == 0
    assert list(inspect.signature(HopSkipJump.generate).parameters)[1:] == ["x", "y", "x_adv_init", "lengths"]
    with pytest.raises(TypeError):
        HopSkipJump(object())


def test_overlap_refusals_name_what_overlaps():
    """Every host twin refuses a written span that overlaps another, by one element here, and says which: views of one buffer."""
    N = _N()
    x, delta = rows(2, 8, 0), np.ones(2, dtype=np.float32)
    p = N.hsj_expand_host(x, delta, 3, 1, 0, 2)
    z, lab = logits_for(2, 3, 4, [0, 1], 0), np.array([0, 1], dtype=np.int32)
    _, counts = workspace(2, 8)
    st = R.new_state(2, 8, [1, 1])
    search = lambda **kw: N.hsj_search_host(z[:2], lab, x, R.BISECT, 0, 0, 2,
                                            **{**dict(x_cand=st["x_cand"], x_far=st["x_far"], x_adv=st["x_adv"], x_best=st["x_best"],
                                                      fstate=st["f"], istate=st["i"], start_lo=-delta, start_hi=delta, theta=delta,
                                                      u=np.zeros((2, 8), dtype=np.float32)), **kw})
    big = np.zeros(64, dtype=np.float64)
    f32 = lambda a, b, shape: big[a:b].view(np.float32).reshape(shape)
    inside = f32(0, 8, (2, 8))
    for bad, msg in ((lambda: N.hsj_expand_host(inside, delta, 3, 1, 0, 2, out=f32(7, 31, (6, 8))), "lipasr_hsj_expand_host: out overlaps x"),
                     (lambda: N.hsj_accumulate_host(z, lab, f32(31, 55, (6, 8)), x, sums=big[:32].reshape(2, 2, 8), counts=counts),
                      "lipasr_hsj_accumulate_host: sums overlaps an input"),
                     (lambda: N.hsj_accumulate_host(z, lab, p, f32(31, 39, (2, 8)), sums=big[:32].reshape(2, 2, 8), counts=counts),
                      "lipasr_hsj_accumulate_host: sums overlaps an input"),
                     (lambda: N.hsj_direction_host(big[:32].reshape(2, 2, 8), counts, 2, u=f32(31, 39, (2, 8))),
                      "lipasr_hsj_direction_host: u overlaps sums"),
                     (lambda: search(x_far=st["x_cand"]), "lipasr_hsj_search_host: x_cand overlaps x_far"),
                     (lambda: search(x_best=st["x_adv"]), "lipasr_hsj_search_host: x_adv overlaps x_best"),
                     (lambda: search(x_cand=x), "lipasr_hsj_search_host: x0 overlaps x_cand"),
                     (lambda: search(u=st["x_best"]), "lipasr_hsj_search_host: x_best overlaps u")):
        with pytest.raises(ValueError) as e:
            bad()
        assert msg in str(e.value), (msg, str(e.value))


# ------------------------------------------------------------------------------------------------------------- the linear model
def linear_model(n=36, seed=0):
    """sign(w x + b) as the two-layer, two-class network relu((w, -w) x + (b, -b)) -> identity: (W1 [n, 2], b1, W2, b2), w, b."""
    rng = np.random.default_rng(seed + 40)
    w = rng.standard_normal(n).astype(np.float32)
    b = np.float32(0.1)
    return (np.stack([w, -w], axis=1), np.array([b, -b], dtype=np.float32), np.eye(2, dtype=np.float32), np.zeros(2, dtype=np.float32)), w, b


def linear_predict(params):
    W1, b1, W2, b2 = params
    return lambda x: (np.maximum(np.asarray(x, dtype=np.float32) @ W1 + b1, 0) @ W2 + b2).astype(np.float32)


def linear_truth(w, b, x, norm):
    a = np.abs(x.astype(np.float64) @ w.astype(np.float64) + float(b))
    return a / (np.linalg.norm(w.astype(np.float64)) if norm == 2 else np.abs(w.astype(np.float64)).sum())


LIN_KW = dict(max_iter=10, init_eval=100, max_eval=1000, init_size=100)
HSJ_KEY = 0x48534A0000000000


@pytest.mark.parametrize("norm", NORMS, ids=ids)
def test_restatement_on_a_linear_model(norm):
    params, w, b = linear_model()
    x = rows(12, 36, 5)
    predict = linear_predict(params)
    labels = predict(x).argmax(axis=1).astype(np.int32)
    out = R.run(predict, x, labels, norm, seed=HSJ_KEY + LIN_SEED[norm], **LIN_KW)
    true = linear_truth(w, b, x, norm)
    ratio = out["dist_best"] / true
    ups = int((np.diff(out["dists"], axis=0) > 0).any(axis=0).sum())
    print(f"norm {norm}: worst distance / true R = {ratio.max():.4f}, rows {np.round(ratio, 3).tolist()}; the iterate's distance went up "
          f"between two iterations on {ups} of 12 rows; queries {out['queries'].tolist()}")
    assert out["found"].all() and not out["already"].any()
    assert (out["dist_best"] >= true - 36 * 2.0 ** -24 * np.abs(x).max()).all()
    assert (out["dist_best"] < out["start_dist"]).all()
    assert ratio.max() <= LIN_R[norm], "LIN_R is the figure the GPU test's bound is made from: measure it again"
    assert (predict(out["x_best"]).argmax(axis=1) != labels).all()
    assert within_one_ulp(out["dist_best"], R.distance(out["x_best"], x, norm).astype(np.float32))
