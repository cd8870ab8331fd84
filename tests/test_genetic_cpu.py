"""The genetic black-box attack without a GPU: lipasr_genetic_breed_host (the CPU-side pin of the counters and of the arithmetic the
device kernel shares with it) against the NumPy restatement of tests/genetic_ref.py, the argument checks of the three entry points,
the surface of lipasr.genetic, and the float64 oracle of the whole algorithm on a linear classifier whose L-inf distances are known.

Bounds.  Which parent an element takes and which elements mutate: exact.  A mutated value: half a unit in the last place of the
fp32 result (the restatement adds in float64 and would round a second time; the library rounds once, in fmaf).  The clamps:
exact -- where a bound binds in exact arithmetic the result IS the bound (rounding is monotone).  Padding: the bits of x0."""
import ctypes as C
import math

import numpy as np
import pytest

import genetic_ref as G

SHAPES = [(1, 2, 1), (3, 5, 880), (2, 4, 881), (2, 3, 22050), (4, 64, 67)]
FULL = 1 << 24


def _rows(B, n, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((B, n))).astype(np.float32)


def _pop(B, P, n, seed):
    return (0.3 * np.random.default_rng(seed + 1000).standard_normal((B, P, n))).astype(np.float32)


def _parents(B, P, seed, copies=True):
    par = np.random.default_rng(seed + 2000).integers(0, P, size=(B, P, 2)).astype(np.int32)
    if copies:
        par[:, 0, 1] = -1  # the elite's slot
    if copies and B > 1:
        par[B - 1, :, 1] = -1  # a finished clip
        par[B - 1, :, 0] = np.arange(P)
    return par


def _host(x0, P, generation, seed, thresh, step, eps, **kw):
    from lipasr import _native as N

    return N.genetic_breed_host(x0, P, generation, seed, thresh, step, eps, **kw)


def check_breed(got, ref, x0, what):
    """``got`` float32 [B, P, n] against genetic_ref.breed's dict; shared with the device tests."""
    B, P, n = got.shape
    valid, want = ref["valid"], ref["want"]
    xr = np.broadcast_to(x0[:, None, :], got.shape)
    assert got[~valid].tobytes() == xr[~valid].tobytes(), f"{what}: padding moved"
    exact = valid & (ref["copied"][:, :, None] | ~ref["mut"] | ref["low"] | ref["high"])  # copies, unmutated picks, bound values
    assert np.array_equal(got[exact], want[exact].astype(np.float32)) and np.array_equal(got[exact].astype(np.float64), want[exact]), \
        f"{what}: a copied, picked or clamped element differs"
    rest = valid & ~exact
    err = np.abs(got.astype(np.float64) - want)[rest]
    bound = 0.5 * np.spacing(np.abs(got[rest])).astype(np.float64)
    assert (err <= bound).all(), f"{what}: worst error {(err / np.maximum(bound, 1e-300)).max():.3f} half units in the last place"


# ---------------------------------------------------------------------------------------------------------------- breed_host
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_breed_host_matches_the_restatement(shape):
    B, P, n = shape
    seed = sum(shape)
    x0, pop_in, par = _rows(B, n, seed), _pop(B, P, n, seed), _parents(B, P, seed)
    step, eps, thresh = 0.05, 0.1, round(0.3 * FULL)
    # pop_in == NULL: the initial population
    got = _host(x0, P, 0, seed, thresh, step, eps)
    check_breed(got, G.breed(x0, P, 0, seed, thresh, step, eps), x0, f"{shape} initial")
    # two parents, copies, and the ball around x0 (pop_in is up to ~1 away: the ball's clamp binds on most elements)
    got = _host(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par)
    ref = G.breed(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par)
    check_breed(got, ref, x0, f"{shape} generation 3")
    assert B * P * n < 100 or (ref["low"].any() and ref["high"].any())
    # a wide ball: which parent, which mutation -- and then the clip range binds instead
    wide = 1e30
    got = _host(x0, P, 3, seed, 0, step, wide, pop_in=pop_in, parents=par)
    ref = G.breed(x0, P, 3, seed, 0, step, wide, pop_in=pop_in, parents=par)
    a, c = (pop_in[np.arange(B)[:, None], np.clip(par[:, :, k], 0, P - 1)] for k in (0, 1))  # [B, P, n] each
    picked = np.where(ref["pick"] & ~ref["copied"][:, :, None], c, a)
    assert got.tobytes() == picked.tobytes(), "no mutation, no clamp: every element is one parent's, bit for bit"
    got = _host(x0, P, 3, seed, thresh, 1.0, wide, pop_in=pop_in, parents=par)
    ref = G.breed(x0, P, 3, seed, thresh, 1.0, wide, pop_in=pop_in, parents=par)
    check_breed(got, ref, x0, f"{shape} step 1")
    moved = got != picked
    assert np.array_equal(moved, ref["mut"] & ~ref["copied"][:, :, None] & (ref["v"] != 0)), "which elements mutate"
    got = _host(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par, clip_lo=-0.05, clip_hi=0.2)
    ref = G.breed(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par, lo=np.float32(-0.05), hi=np.float32(0.2))
    check_breed(got, ref, x0, f"{shape} clip range")
    bred = ~ref["copied"][:, :, None] & ref["valid"]
    assert got[bred].min() >= np.float32(-0.05) and got[bred].max() <= np.float32(0.2)
    # every n_valid of the issue, cycled over the rows
    values = [0, 1, 5, n - 1, n, n + 3, -2]
    base = _host(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par)
    for s in range(0, len(values), B):
        nv = np.array((values[s:] + values)[:B], dtype=np.int32)
        got = _host(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par, n_valid=nv)
        ref = G.breed(x0, P, 3, seed, thresh, step, eps, pop_in=pop_in, parents=par, n_valid=nv)
        check_breed(got, ref, x0, f"{shape} n_valid {nv.tolist()}")
        assert np.array_equal(got[ref["valid"]], base[ref["valid"]])  # the valid part is what the call without lengths wrote


def test_mutation_threshold_edges():
    x0, pop_in, par = _rows(2, 881, 1), _pop(2, 5, 881, 1), _parents(2, 5, 1, copies=False)
    none = G.breed(x0, 5, 1, 7, 0, 0.05, 1e30, pop_in=pop_in, parents=par)
    every = G.breed(x0, 5, 1, 7, FULL, 1.0, 1e30, pop_in=pop_in, parents=par)
    assert not none["mut"].any() and every["mut"].all()
    got0, got1 = (_host(x0, 5, 1, 7, t, 1.0, 1e30, pop_in=pop_in, parents=par) for t in (0, FULL))
    check_breed(got0, G.breed(x0, 5, 1, 7, 0, 1.0, 1e30, pop_in=pop_in, parents=par), x0, "thresh 0")
    check_breed(got1, every, x0, "thresh 2^24")
    assert ((got0 != got1) == (every["v"] != 0)).all()  # everything moved (but where the amplitude is exactly 0)
    assert np.abs(got1 - got0).max() <= 1.0 + 1e-6 and np.abs(got1 - got0).max() > 0.99
    # step = 0 and eps = 0: a mutation of nothing; the ball of radius 0 is x0
    assert _host(x0, 5, 1, 7, FULL, 0.0, 1e30, pop_in=pop_in, parents=par).tobytes() == got0.tobytes()
    assert _host(x0, 5, 1, 7, FULL, 1.0, 0.0, pop_in=pop_in, parents=par).tobytes() == np.repeat(x0[:, None], 5, axis=1).tobytes()


def test_draws_do_not_depend_on_the_chunk():
    B, P, n = 3, 4, 881
    x0, pop_in, par = _rows(B, n, 2), _pop(B, P, n, 2), _parents(B, P, 2)
    args = (P, 5, 11, round(0.2 * FULL), 0.05, 0.4)
    whole = _host(x0, *args, pop_in=pop_in, parents=par)
    for r in range(B):
        alone = _host(x0[r:r + 1], *args, pop_in=pop_in[r:r + 1], parents=par[r:r + 1], clip0=r)
        assert alone.tobytes() == whole[r:r + 1].tobytes()
    assert _host(x0, *args, pop_in=pop_in, parents=par).tobytes() == whole.tobytes()
    bred = par[:, :, 1] >= 0
    for other in ((P, 6, 11), (P, 5, 12)):  # another generation, another seed: other draws
        diff = _host(x0, *other, *args[3:], pop_in=pop_in, parents=par) != whole
        assert diff[bred].mean() > 0.1 and not diff[~bred].any()
    # the clip index is part of the counter: the same row as clip 0 and as clip 1 draws differently
    assert (_host(x0[:1], *args, clip0=0) != _host(x0[:1], *args, clip0=1)).mean() > 0.1
    # members differ from each other (the member index is part of the counter)
    init = _host(x0, *args)
    assert (init[:, 0] != init[:, 1]).mean() > 0.1


def test_rates():
    """Over B * P * n = 4 * 16 * 22050 = 1 411 200 elements: the mutated share and the share taken from parent c, each inside a
    5-sigma binomial interval; the amplitudes are uniform on (-1, 1] (mean and variance of 70 000 of them inside 5 sigma)."""
    B, P, n, p_mut = 4, 16, 22050, 0.05
    x0 = np.zeros((B, n), dtype=np.float32)
    pop_in = np.zeros((B, P, n), dtype=np.float32)
    pop_in[:, 1] = 1.0
    par = np.zeros((B, P, 2), dtype=np.int32)
    par[:, :, 1] = 1  # a = member 0 (all 0), c = member 1 (all 1)
    thresh = round(p_mut * FULL)
    plain = _host(x0, P, 2, 5, 0, 1.0, 1e30, pop_in=pop_in, parents=par)
    total = plain.size
    assert total >= 10 ** 6 and set(np.unique(plain)) == {0.0, 1.0}
    share_c = plain.mean(dtype=np.float64)
    assert abs(share_c - 0.5) <= 5 * math.sqrt(0.25 / total), share_c
    got = _host(x0, P, 2, 5, thresh, 1.0, 1e30, pop_in=pop_in, parents=par)
    moved = got != plain
    q = thresh / FULL
    assert abs(moved.mean(dtype=np.float64) - q) <= 5 * math.sqrt(q * (1 - q) / total), moved.mean()
    v = (got - plain)[moved].astype(np.float64)
    assert np.abs(v).max() <= 1.0 and abs(v.mean()) <= 5 * math.sqrt(1 / 3 / v.size) and abs(v.var() - 1 / 3) <= 5 * math.sqrt(4 / 45 / v.size)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_abi_argument_checks_without_a_device():
    from lipasr import _native as N

    assert N.lib.lipasr_version() >= 620 and N.has("lipasr_genetic_breed") and N.has("lipasr_genetic_select")
    assert len(N.lib.lipasr_genetic_breed.argtypes) == 18 and len(N.lib.lipasr_genetic_select.argtypes) == 16
    assert len(N.lib.lipasr_genetic_breed_host.argtypes) == 16
    inf = math.inf

    def breed(h=None, x0=None, pop_in=None, parents=None, out=None, B=2, P=4, n=8, generation=0, thresh=0, step=0.1, eps=0.1, lo=-inf,
              hi=inf, host=False):
        if host:
            return N.lib.lipasr_genetic_breed_host(x0, None, pop_in, parents, B, P, n, 0, generation, 0, thresh, step, eps, lo, hi, out)
        return N.lib.lipasr_genetic_breed(h, x0, None, pop_in, parents, B, P, n, 0, generation, 0, thresh, step, eps, lo, hi, out, None)

    fake = C.c_void_p(8)
    buf = np.zeros(2 * 4 * 8 * 2 + 8, dtype=np.float32)
    at = lambda k: C.c_void_p(buf.ctypes.data + 4 * k)
    par = np.zeros((2, 4, 2), dtype=np.int32)
    pp = C.c_void_p(par.ctypes.data)
    common = ((dict(P=1), "population 1"), (dict(P=65), "population 65"), (dict(generation=1 << 24), "generation 16777216"),
              (dict(thresh=FULL + 1), "mutate_thresh"), (dict(step=-0.1), "step -0.1"), (dict(step=inf), "step inf"),
              (dict(step=math.nan), "step"), (dict(eps=-1.0), "eps -1"), (dict(eps=inf), "eps inf"), (dict(eps=math.nan), "eps"),
              (dict(lo=1.0, hi=-1.0), "clip range"), (dict(lo=math.nan), "clip range"), (dict(B=-1), "bad shape"), (dict(n=-1), "bad shape"))
    for host, name in ((False, "lipasr_genetic_breed:"), (True, "lipasr_genetic_breed_host:")):
        pointers = ((dict(), "x0 or pop_out is null"), (dict(x0=at(0)), "x0 or pop_out is null"),
                    (dict(x0=at(0), out=at(16), pop_in=at(100)), "pop_in and parents go together"),
                    (dict(x0=at(0), out=at(16), parents=pp), "pop_in and parents go together"),
                    (dict(x0=at(0), out=at(16), pop_in=at(16 + 63), parents=pp), "pop_out overlaps pop_in"),
                    (dict(x0=at(0), out=at(16 + 63), pop_in=at(16), parents=pp), "pop_out overlaps pop_in"),
                    (dict(x0=at(0), out=at(15)), "pop_out overlaps x0"), (dict(x0=at(64), out=at(1)), "pop_out overlaps x0"))
        for kw, msg in common + pointers + (() if host else ((dict(x0=at(0), out=at(16), h=None), "null handle"),)):
            kw = dict(dict(h=fake), **kw)
            assert breed(host=host, **kw) == N.EINVAL, (name, kw)
            assert msg in N.last_error() and N.last_error().startswith(name), (kw, N.last_error())
        for zero in (dict(B=0), dict(n=0)):
            assert breed(host=host, h=fake, **zero) == N.OK
    with pytest.raises(ValueError, match="pop_out overlaps pop_in"):  # through the NumPy wrapper: the first member is the output
        pop = np.zeros((2, 4, 8), dtype=np.float32)
        N.genetic_breed_host(np.zeros((2, 8), dtype=np.float32), 4, 1, 0, 0, 0.1, 0.1, pop_in=pop, parents=par, out=pop)

    def select(h=fake, logits=at(0), labels=pp, B=2, P=4, classes=4, T=0.01, generation=0, out=pp):
        return N.lib.lipasr_genetic_select(h, logits, labels, B, P, classes, 0, T, 0, generation, 0, out, out, out, out, None)

    for kw, msg in ((dict(classes=0), "0 classes"), (dict(classes=33), "33 classes"), (dict(P=1), "population 1"), (dict(P=65), "population 65"),
                    (dict(T=0.0), "temperature 0"), (dict(T=-1.0), "temperature -1"), (dict(T=inf), "temperature inf"),
                    (dict(T=math.nan), "temperature"), (dict(generation=1 << 24), "generation"), (dict(B=-1), "batch -1"),
                    (dict(h=None), "null handle"), (dict(logits=None), "a null pointer"), (dict(labels=None), "a null pointer"),
                    (dict(out=None), "a null pointer")):
        assert select(**kw) == N.EINVAL, kw
        assert msg in N.last_error() and N.last_error().startswith("lipasr_genetic_select:"), (kw, N.last_error())
    assert select(B=0) == N.OK


def test_genetic_attack_is_exported_and_checks_its_arguments():
    import inspect

    from lipasr import attack_eval as V, attacks as A, genetic as Z

    assert A.GeneticAttack is Z.GeneticAttack and callable(V.genetic_sweep)
    sig = inspect.signature(Z.GeneticAttack.__init__)
    assert list(sig.parameters)[1:3] == ["estimator", "eps"]
    for k, d in (("pop_size", 20), ("max_iter", 500), ("mutation_p", 0.0005), ("step", None), ("temperature", 0.01), ("targeted", False),
                 ("seed", 0), ("check_every", 10)):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == d
    assert sig.parameters["clip_values"].kind is inspect.Parameter.KEYWORD_ONLY
    for fn in (Z.GeneticAttack.generate, Z.GeneticAttack.generate_device):
        assert list(inspect.signature(fn).parameters)[1:] == [("x" if fn is Z.GeneticAttack.generate else "xt"),
                                                               ("y" if fn is Z.GeneticAttack.generate else "yt"), "lengths"]
    with pytest.raises(TypeError):
        Z.GeneticAttack(object(), 0.1)
    assert Z.mutate_threshold(0.0) == 0 and Z.mutate_threshold(1.0) == FULL and Z.mutate_threshold(0.0005) == 8389
    with pytest.raises(ValueError):
        Z.mutate_threshold(1.5)


def test_menu_accepts_genetic(tmp_path):
    """attack_eval.main takes --attack black --kind genetic over either domain and goes on to load the dataset."""
    from lipasr import attack_eval as V

    missing = str(tmp_path) + "/missing/"
    for over in ("mfcc", "audio"):
        with pytest.raises(FileNotFoundError):
            V.main(["--attack", "black", "--kind", "genetic", "--over", over, "--points", "1", "--path", missing])


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_conventions_of_select():
    """The edges include/lipasr.h fixes, on the definition the device tests compare against."""
    z = np.array([[0.0, 1.0, 3.0], [2.0, 1.0, 0.0], [np.nan, 9.0, 1.0], [1.0, 1.0, 1.0],   # clip 0, label 0
                  [0.0, 5.0, 0.0], [0.0, 5.0, 1.0], [0.0, 7.0, 0.0], [0.0, 5.0, 1.0]], dtype=np.float32)  # clip 1, label 1
    f = G.fitness(z, [0, 1], 4)
    np.testing.assert_array_equal(f, [[3.0, -1.0, -np.inf, 0.0], [-5.0, -4.0, -7.0, -4.0]])
    np.testing.assert_array_equal(G.fitness(z, [0, 1], 4, targeted=True)[1], [5.0, 4.0, 7.0, 4.0])
    r = G.select(z, [0, 1], 4, 6, 1, 0.5)
    np.testing.assert_array_equal(r["best"], [0, 1])  # the lowest index on a tie
    np.testing.assert_array_equal(r["done"], [7, 0])  # generation + 1
    np.testing.assert_array_equal(r["parents"][0], [[0, -1], [1, -1], [2, -1], [3, -1]])
    np.testing.assert_array_equal(r["parents"][1, 0], [1, -1])
    assert r["drawn"].tolist() == [[False] * 4, [False, True, True, True]] and (r["parents"][1, 1:] >= 0).all()
    again = G.select(z, [0, 1], 4, 9, 1, 0.5, done=r["done"])
    assert again["done"].tolist() == [7, 0] and again["best"].tolist() == [-1, 1]
    nan = G.select(np.full((4, 3), np.nan, dtype=np.float32), [0], 4, 0, 1, 0.5)
    assert nan["best"].tolist() == [0] and nan["done"].tolist() == [0] and nan["parents"][0].tolist() == [[0, -1], [1, -1], [2, -1], [3, -1]]
    assert np.isneginf(G.fitness(np.ones((2, 1), dtype=np.float32), [0], 2)).all()  # one class, untargeted
    # at T = 0.01 the weight of a member 1 below the best is e^-100: every draw lands on the best two
    r = G.select(z, [2, 1], 4, 0, 3, 0.01)
    assert set(r["parents"][1, 1:].reshape(-1)) <= {1, 3}


LINEAR_WORST = 38  # generations the oracle needs on its slowest row at eps = 4 d (measured, see the test below)
LINEAR_BUDGET = 2 * LINEAR_WORST


def _host_classify(W, bias):
    return G.linear_classify(W, bias)


def test_oracle_attack_on_a_linear_classifier():
    """One dense layer 880 -> 2, six rows at the same L2 distance 0.25, so at (almost) one L-inf distance d = |w . x + c| / ||w||_1
    from the boundary; P = 16, mutation_p = 0.05, T = 0.01, step = eps, seed genetic_ref.LINEAR_SEED = 0 (the first tried).
    eps = 0.9 min d: no perturbation inside the ball changes the class (a theorem), so no row succeeds in the full budget.
    eps = 4 max d: every row succeeds; with the real Philox stream the oracle's rows take 38, 33, 32, 33, 35, 34 generations (the issue's
    simulation with an ordinary generator: 26 .. 78), so LINEAR_WORST = 38 and the budget every row must succeed in -- here and on
    the device -- is LINEAR_BUDGET = 2 x 38 = 76 generations."""
    W, bias, x, d, cls = G.linear_case_inf()
    assert d.max() / d.min() < 1.001
    classify = _host_classify(W, bias)
    small = G.attack(classify, x, cls, 0.9 * d.min(), max_iter=LINEAR_BUDGET, seed=G.LINEAR_SEED, **G.LINEAR)
    assert not small["success"].any() and (small["generations"] == LINEAR_BUDGET).all() and (small["fitness"] < 0).all()
    assert G.within_ball(small["adv"], x, 0.9 * d.min())
    eps = 4.0 * d.max()
    big = G.attack(classify, x, cls, eps, max_iter=LINEAR_BUDGET, seed=G.LINEAR_SEED, **G.LINEAR)
    print(f"oracle, eps = 4 d: generations per row {big['generations'].tolist()}")
    assert big["success"].all() and (big["fitness"] > 0).all()
    assert big["generations"].max() == LINEAR_WORST and big["generations"].max() * 2 <= LINEAR_BUDGET
    assert (classify(big["adv"].astype(np.float64)).argmax(axis=1) != cls).all()
    assert G.within_ball(big["adv"], x, eps)
    # the library's host breed gives the oracle's initial population
    got = _host(x, 16, 0, G.LINEAR_SEED, round(0.05 * FULL), eps, eps)
    check_breed(got, G.breed(x, 16, 0, G.LINEAR_SEED, round(0.05 * FULL), eps, eps), x, "initial population")
