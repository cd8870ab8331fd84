"""The genetic black-box attack on the MI355X: lipasr_genetic_breed against lipasr_genetic_breed_host bit for bit (the host
function is pinned to the NumPy restatement in tests/test_genetic_cpu.py), lipasr_genetic_select against the float64 oracle of
tests/genetic_ref.py, lipasr.genetic.GeneticAttack against a hand-built chain of the same calls and across chunks, and the attack
end to end where the answer is known and on small real models.

Bounds.  breed: exact (one shared inline function, no libm).  select: fitness within 2 units in the last place of max |logit| (the
kernel takes the difference in fp64 and rounds once: half a unit of the result); best, done and the frozen / elite rows exact;
a parent draw whose u * total lies within 1e-5 * total of one of the oracle's cumulative weights may come out as either
neighbour, every other draw is exact, and the oracle's own share of such draws is asserted to be at most 1 %."""
import itertools
import math
import wave

import numpy as np
import pytest
import torch

import genetic_ref as G
import local_lip_ref as R
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P
from test_genetic_cpu import FULL, LINEAR_BUDGET, SHAPES, _parents, _pop, _rows

pytestmark = pytest.mark.gpu


def _place(x, offset=0, dtype=torch.float32, fill=0.0):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation."""
    buf = torch.full((x.size + offset,), fill, device="cuda", dtype=dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _breed(x0, P_, generation, seed, thresh, step, eps, pop_in=None, parents=None, n_valid=None, clip0=0, clip=None, offs=(0, 0, 0)):
    """One lipasr_genetic_breed -> NumPy float32 [B, P, n]."""
    from lipasr.genetic import genetic_breed

    B, n = x0.shape
    xt = _place(x0, offs[0])
    pin = None if pop_in is None else _place(pop_in.reshape(B * P_, n), offs[1])
    par = None if parents is None else torch.as_tensor(parents).cuda()
    nv = None if n_valid is None else torch.as_tensor(np.asarray(n_valid, dtype=np.int32)).cuda()
    out = torch.full((B * P_ * n + offs[2],), 7.0, device="cuda")[offs[2]:].view(B * P_, n)
    got = genetic_breed(xt, P_, generation, seed, thresh, step, eps, pop_in=pin, parents=par, n_valid=nv, clip0=clip0, clip_values=clip, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy().reshape(B, P_, n)


def _host(x0, P_, generation, seed, thresh, step, eps, clip=None, **kw):
    from lipasr import _native as N

    lo, hi = (-math.inf, math.inf) if clip is None else clip
    return N.genetic_breed_host(x0, P_, generation, seed, thresh, step, eps, clip_lo=lo, clip_hi=hi, **kw)


# =================================================================================================
# 1. breed
# =================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_breed_equals_the_host_function_bit_for_bit(cuda, shape):
    B, P_, n = shape
    seed = sum(shape)
    x0, pop_in, par = _rows(B, n, seed), _pop(B, P_, n, seed), _parents(B, P_, seed)
    args = (P_, 3, seed, round(0.3 * FULL), 0.05, 0.1)
    want = _host(x0, *args, pop_in=pop_in, parents=par)
    for offs in itertools.product((0, 1), repeat=3):  # x0, pop_in, pop_out: the alignment picks the loads, never a value
        got = _breed(x0, *args, pop_in=pop_in, parents=par, offs=offs)
        assert got.tobytes() == want.tobytes(), f"{shape} offsets {offs}"
    init = _host(x0, P_, 0, seed, FULL, 0.05, 0.1)
    for offs in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)):
        assert _breed(x0, P_, 0, seed, FULL, 0.05, 0.1, offs=offs).tobytes() == init.tobytes(), f"{shape} initial, offsets {offs}"
    values = [0, 1, 5, n - 1, n, n + 3, -2]
    for s in range(0, len(values), B):
        nv = np.array((values[s:] + values)[:B], dtype=np.int32)
        want_nv = _host(x0, *args, pop_in=pop_in, parents=par, n_valid=nv, clip=(-0.05, 0.2))
        for offs in ((0, 0, 0), (1, 1, 1)):
            got = _breed(x0, *args, pop_in=pop_in, parents=par, n_valid=nv, clip=(-0.05, 0.2), offs=offs)
            assert got.tobytes() == want_nv.tobytes(), f"{shape} n_valid {nv.tolist()} offsets {offs}"
        pad = np.arange(n)[None, None, :] >= np.clip(nv, 0, n)[:, None, None]
        assert got[np.broadcast_to(pad, got.shape)].tobytes() == np.broadcast_to(x0[:, None], got.shape)[np.broadcast_to(pad, got.shape)].tobytes()
    # a chunk that starts at clip 1 draws what the whole call drew there
    if B > 1:
        assert _breed(x0[1:], *args, pop_in=pop_in[1:], parents=par[1:], clip0=1).tobytes() == want[1:].tobytes()


def test_breed_refuses_overlap_and_bad_arguments(cuda):
    from lipasr import _native as N
    from lipasr.genetic import genetic_breed

    B, P_, n = 2, 4, 16
    x0 = torch.zeros(B, n, device="cuda")
    buf = torch.zeros(2 * B * P_ * n, device="cuda")
    par = torch.zeros(B, P_, 2, dtype=torch.int32, device="cuda")
    whole = B * P_ * n
    for start in (0, 1, whole - 1):
        with pytest.raises(ValueError, match="pop_out overlaps pop_in"):
            genetic_breed(x0, P_, 1, 0, 0, 0.1, 0.1, pop_in=buf[:whole].view(B * P_, n), parents=par, out=buf[start:start + whole].view(B * P_, n))
        with pytest.raises(ValueError, match="pop_out overlaps pop_in"):
            genetic_breed(x0, P_, 1, 0, 0, 0.1, 0.1, pop_in=buf[start:start + whole].view(B * P_, n), parents=par, out=buf[:whole].view(B * P_, n))
    genetic_breed(x0, P_, 1, 0, 0, 0.1, 0.1, pop_in=buf[:whole].view(B * P_, n), parents=par, out=buf[whole:].view(B * P_, n))  # adjacent: fine
    with pytest.raises(ValueError, match="pop_out overlaps x0"):
        genetic_breed(buf[:B * n].view(B, n), P_, 0, 0, 0, 0.1, 0.1, out=buf[:whole].view(B * P_, n))
    with pytest.raises(ValueError, match="go together"):
        genetic_breed(x0, P_, 1, 0, 0, 0.1, 0.1, pop_in=buf[:whole].view(B * P_, n), out=buf[whole:].view(B * P_, n))
    for kw in (dict(step=-1.0), dict(eps=math.inf), dict(clip_values=(1.0, -1.0))):
        a = dict(dict(step=0.1, eps=0.1), **kw)
        with pytest.raises(ValueError):
            genetic_breed(x0, P_, 0, 0, 0, a.pop("step"), a.pop("eps"), **a)
    with pytest.raises(ValueError):
        genetic_breed(x0, 65, 0, 0, 0, 0.1, 0.1)
    with pytest.raises(ValueError):
        genetic_breed(x0, P_, 1 << 24, 0, 0, 0.1, 0.1)
    with pytest.raises(ValueError):
        genetic_breed(x0.t(), P_, 0, 0, 0, 0.1, 0.1)
    assert genetic_breed(x0[:0], P_, 0, 0, 0, 0.1, 0.1).shape == (0, n)
    h = N.get_handle(0)
    assert N.lib.lipasr_genetic_breed(h.h, None, None, None, None, 0, P_, n, 0, 0, 0, 0, 0.1, 0.1, -np.inf, np.inf, None, N.stream_ptr()) == N.OK
    assert N.lib.lipasr_genetic_breed(h.h, None, None, None, None, 2, P_, n, 0, 0, 0, 0, 0.1, 0.1, -np.inf, np.inf, None, N.stream_ptr()) == N.EINVAL
    # parent indices outside the population are clamped into it, never followed
    pop = torch.arange(whole, device="cuda", dtype=torch.float32).view(B * P_, n)
    par[:, :, 0], par[:, :, 1] = 99, -1
    out = genetic_breed(x0, P_, 1, 0, 0, 0.1, 1e30, pop_in=pop, parents=par)
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, P_, n), pop.view(B, P_, n)[:, -1:].expand(B, P_, n))


# =================================================================================================
# 2. select
# =================================================================================================
def _select_logits(B, P_, C, rng, spread, targeted=False):
    """Clips whose members sit ``spread`` apart around one row of logits, so that at T = spread several members carry weight.
    Labels: the class of member 0 (targeted: the next one), so that most of the fitness is negative and parents are drawn."""
    base = rng.standard_normal((B, 1, C)) * 2.0
    z = (base + spread * rng.standard_normal((B, P_, C))).astype(np.float32)
    labels = ((z[:, 0].argmax(axis=1) + int(targeted)) % C).astype(np.int32)
    return z, labels


def _run_select(z, labels, P_, generation, seed, T_, targeted, done):
    from lipasr.genetic import genetic_select

    B = labels.shape[0]
    zt = _place(z.reshape(B * P_, -1))
    out = dict(fitness=torch.full((B, P_), 7.0, device="cuda"), best=torch.full((B,), -5, dtype=torch.int32, device="cuda"),
               done=torch.as_tensor(np.asarray(done, dtype=np.int32)).cuda(), parents=torch.full((B, P_, 2), -9, dtype=torch.int32, device="cuda"))
    genetic_select(zt, torch.as_tensor(labels).cuda(), P_, generation, seed, T_, targeted=targeted, clip0=3, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_select(got, ref, z, labels, P_, best_before, what):
    """-> (draws, ambiguous draws) of the oracle."""
    B = labels.shape[0]
    f = ref["fitness"]
    scale = 2.0 * np.spacing(np.float32(np.abs(np.where(np.isfinite(z), z, 0)).max()))
    fin = np.isfinite(f)
    assert np.array_equal(got["fitness"][~fin], f[~fin].astype(np.float32)), f"{what}: a non-finite fitness differs"
    assert (np.abs(got["fitness"][fin].astype(np.float64) - f[fin]) <= scale).all(), f"{what}: fitness"
    np.testing.assert_array_equal(got["done"], ref["done"], err_msg=what)
    top = np.sort(np.where(np.isnan(f), -np.inf, f), axis=1)[:, ::-1]
    clear = np.isinf(top[:, 0]) | np.isinf(top[:, 1]) | (np.abs(np.where(np.isinf(top), 0, top)[:, 0] - np.where(np.isinf(top), 0, top)[:, 1]) > scale)
    fresh = ref["best"] >= 0
    assert np.array_equal(got["best"][fresh & clear], ref["best"][fresh & clear]), f"{what}: best"
    assert np.array_equal(got["best"][~fresh], best_before[~fresh]), f"{what}: a finished clip lost its best"
    drawn = ref["drawn"]
    fixed = ~drawn
    for b in range(B):
        if not clear[b] and fresh[b]:
            continue
        assert np.array_equal(got["parents"][b][fixed[b]], ref["parents"][b][fixed[b]]), f"{what}: clip {b} frozen / elite rows"
    gp, rp, alt = got["parents"][drawn], ref["parents"][drawn], ref["alt"][drawn]
    assert ((gp == rp) | (gp == alt)).all(), f"{what}: {int(((gp != rp) & (gp != alt)).sum())} parent draws differ"
    nan_member = np.isnan(z).any(axis=2)  # [B, P]
    assert not nan_member[np.nonzero(drawn)[0][:, None].repeat(2, axis=1), gp].any(), f"{what}: a NaN member was drawn"
    return rp.size, int((rp != alt).sum())


@pytest.mark.parametrize("P_,C", list(itertools.product((2, 5, 20, 64), (1, 2, 10, 32))), ids=lambda v: str(v))
def test_select_matches_float64(cuda, P_, C):
    B = 24
    draws = ambiguous = 0
    for T_, targeted in itertools.product((0.01, 1.0), (False, True)):
        rng = np.random.default_rng(1000 * P_ + 10 * C + int(targeted) + int(T_ * 100))
        z, labels = _select_logits(B, P_, C, rng, T_, targeted)
        z[1, P_ - 1, 0] = np.nan  # a NaN member
        z[2] = np.nan  # a clip with nothing but NaN
        z[3, 0, C - 1] = np.inf  # +inf is a value like any other
        if C > 1:
            other = (labels[4] + 1) % C
            z[4, 1, other if not targeted else labels[4]] += 50.0  # a member of clip 4 succeeds
            z[5, :, labels[5]] += (50.0 if not targeted else -50.0)  # a hopeless clip: every fitness far below 0
        seed, gen = 77 + P_, 5
        ref = G.select(z.reshape(B * P_, C), labels, P_, gen, seed, T_, targeted, clip0=3)
        got = _run_select(z, labels, P_, gen, seed, T_, targeted, np.zeros(B))
        what = f"P {P_} C {C} T {T_} targeted {targeted}"
        d, a = _check_select(got, ref, z, labels, P_, got["best"], what)
        draws, ambiguous = draws + d, ambiguous + a
        assert (got["parents"][2] == np.stack([np.arange(P_), -np.ones(P_)], axis=1)).all() and got["done"][2] == 0  # all NaN: copies
        if C > 1:
            assert got["done"][4] == gen + 1 and (got["parents"][4][:, 1] == -1).all() and got["best"][4] == 1
            assert got["done"][5] == 0 and got["parents"][5][0].tolist() == [got["best"][5], -1]
        else:
            rest = np.arange(B) != 2  # one class: z_y - (-inf) = +inf, or -inf untargeted
            assert (got["done"][rest] == (gen + 1 if targeted else 0)).all()
        # sticky: the next generation's logits would finish other clips and move every best; the finished ones stay as they are
        z2, _ = _select_logits(B, P_, C, rng, T_, targeted)
        if C > 1:
            z2[6, 0, (labels[6] + 1) % C if not targeted else labels[6]] += 50.0
        ref2 = G.select(z2.reshape(B * P_, C), labels, P_, gen + 1, seed, T_, targeted, clip0=3, done=ref["done"])
        got2 = _run_select(z2, labels, P_, gen + 1, seed, T_, targeted, got["done"])
        best2 = np.where(ref2["best"] >= 0, got2["best"], got["best"])
        # the kernel leaves best alone on a finished clip: hand it the first call's value, as the attack's buffer would hold
        d, a = _check_select(dict(got2, best=best2), ref2, z2, labels, P_, got["best"], what + " (second call)")
        draws, ambiguous = draws + d, ambiguous + a
        was = got["done"] != 0
        assert np.array_equal(got2["done"][was], got["done"][was]) and (got2["parents"][was][:, :, 1] == -1).all()
        assert (got2["best"][was] == -5).all()  # untouched: _run_select filled it with -5
        if C > 1:
            assert got2["done"][6] == (got["done"][6] or gen + 2)
        # two runs, the same bits
        again = _run_select(z, labels, P_, gen, seed, T_, targeted, np.zeros(B))
        assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    print(f"P {P_} C {C}: {draws} parent draws of the oracle, {ambiguous} ambiguous")
    assert ambiguous <= 0.01 * draws


def test_select_argument_checks(cuda):
    from lipasr.genetic import genetic_select

    B, P_, C = 2, 4, 3
    ok = dict(fitness=torch.zeros(B, P_, device="cuda"), best=torch.zeros(B, dtype=torch.int32, device="cuda"),
              done=torch.zeros(B, dtype=torch.int32, device="cuda"), parents=torch.zeros(B, P_, 2, dtype=torch.int32, device="cuda"))
    z, lab = torch.zeros(B * P_, C, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    genetic_select(z, lab, P_, 0, 0, 0.01, **ok)
    for bad in (dict(temperature=0.0), dict(temperature=math.inf), dict(generation=1 << 24), dict(logits=torch.zeros(B * P_, 33, device="cuda")),
                dict(labels=lab.long()), dict(fitness=torch.zeros(B, P_ + 1, device="cuda")), dict(pop=3)):
        a = dict(dict(logits=z, labels=lab, pop=P_, generation=0, seed=0, temperature=0.01), **{k: v for k, v in bad.items() if k not in ok})
        kw = dict(ok, **{k: v for k, v in bad.items() if k in ok})
        with pytest.raises(ValueError):
            genetic_select(a["logits"], a["labels"], a["pop"], a["generation"], a["seed"], a["temperature"], **kw)
    # a label outside the classes: every fitness -inf, the clip copies itself, nothing is read out of bounds
    lab[1] = 7
    genetic_select(z, lab, P_, 0, 0, 0.01, **ok)
    torch.cuda.synchronize()
    assert torch.isneginf(ok["fitness"][1]).all() and (ok["parents"][1, :, 1] == -1).all() and int(ok["done"][1]) == 0


# =================================================================================================
# 3. GeneticAttack against the hand-built chain, and across chunks
# =================================================================================================
SMALL = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]


@pytest.fixture(scope="module")
def small(cuda):
    from lipasr.attacks import TensorFlowV2Classifier

    m = build_model(SMALL, max_batch=64)
    load_params(m, R.setup_params(SMALL, 2))
    x = np.random.default_rng(4).standard_normal((5, 36)).astype(np.float32)
    return dict(model=m, x=x, clf=TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,)))


def test_generate_equals_the_hand_built_chain(small):
    from lipasr.attacks import GeneticAttack
    from lipasr.genetic import genetic_breed, genetic_select, mutate_threshold

    clf, xt = small["clf"], dev(small["x"])
    B, n, P_, eps, seed = 5, 36, 6, 0.3, 9
    atk = GeneticAttack(clf, eps, pop_size=P_, max_iter=3, mutation_p=0.1, temperature=0.05, seed=seed)
    adv = atk.generate_device(xt)
    thresh = mutate_threshold(0.1)
    labels = clf.model.predict_device(xt, logits=True).argmax(dim=1).to(torch.int32)
    fitness, best = torch.empty(B, P_, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    done, parents = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.empty(B, P_, 2, dtype=torch.int32, device="cuda")
    pop = genetic_breed(xt, P_, 0, seed, thresh, eps, eps)
    for g in range(3):
        genetic_select(clf.model.predict_device(pop, logits=True), labels, P_, g, seed, 0.05, fitness=fitness, best=best, done=done, parents=parents)
        if g < 2:
            pop = genetic_breed(xt, P_, g + 1, seed, thresh, eps, eps, pop_in=pop, parents=parents)
    rows = torch.arange(B, device="cuda")
    want = pop.view(B, P_, n)[rows, best.long()]
    assert adv.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert torch.equal(atk.success_, done != 0) and atk.success_.dtype == torch.bool
    assert torch.equal(atk.queries_, P_ * torch.where(done != 0, done, torch.full_like(done, 3)).long()) and atk.queries_.dtype == torch.int64
    assert torch.equal(atk.fitness_, fitness[rows, best.long()]) and atk.fitness_.dtype == torch.float32
    assert G.within_ball(adv.cpu().numpy(), small["x"], eps) and adv.data_ptr() != xt.data_ptr()
    # NumPy in, NumPy out; labels given as one-hot or as indices are the labels found above
    onehot = np.eye(5, dtype=np.float32)[labels.cpu().numpy()]
    for y in (None, onehot, labels.cpu().numpy()):
        assert atk.generate(small["x"], y).tobytes() == want.cpu().numpy().tobytes()
    assert GeneticAttack(clf, eps, pop_size=P_, max_iter=3, mutation_p=0.1, temperature=0.05, seed=seed + 1).generate(small["x"]).tobytes() \
        != want.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        atk.generate_device(xt, lengths=[36] * 5)
    with pytest.raises(ValueError):
        atk.generate_device(xt[:, :35])
    with pytest.raises(ValueError):
        GeneticAttack(clf, eps, targeted=True).generate_device(xt)
    for bad in (dict(pop_size=1), dict(pop_size=65), dict(max_iter=0), dict(mutation_p=1.5), dict(temperature=0.0), dict(step=-1.0), dict(check_every=0)):
        with pytest.raises(ValueError):
            GeneticAttack(clf, eps, **bad)
    with pytest.raises(ValueError):
        GeneticAttack(clf, -0.1)
    assert atk.generate_device(xt[:0]).shape == (0, 36)


def test_results_do_not_depend_on_the_chunks(small):
    """Five clips, population 4: whole (20 rows in one chunk) against a classifier whose batch_limit of 8 forces chunks of two clips.
    A chunk whose clips are all done stops early; the whole call goes on copying them: the same rows come back."""
    from lipasr.attacks import GeneticAttack, TensorFlowV2Classifier

    class Limited(TensorFlowV2Classifier):
        batch_limit = 8

    clf, xt = small["clf"], dev(small["x"])
    lim = Limited(model=small["model"], nb_classes=5, input_shape=(36,))
    assert clf.batch_limit >= 20 and lim.batch_limit == 8
    kw = dict(pop_size=4, max_iter=12, mutation_p=0.1, temperature=0.05, seed=3, check_every=2)
    for eps in (0.05, 1.0):
        whole, parts = GeneticAttack(clf, eps, **kw), GeneticAttack(lim, eps, **kw)
        a, b = whole.generate_device(xt), parts.generate_device(xt)
        print(f"eps {eps}: success {whole.success_.tolist()} queries {whole.queries_.tolist()}")
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert torch.equal(whole.success_, parts.success_) and torch.equal(whole.queries_, parts.queries_)
        assert torch.equal(whole.fitness_, parts.fitness_)
        alone = GeneticAttack(clf, eps, **kw)
        # a clip's draws are keyed by its row index in x: row 0 alone is row 0 of the batch
        assert alone.generate_device(xt[:1]).cpu().numpy().tobytes() == a[:1].cpu().numpy().tobytes()


# =================================================================================================
# 4. end to end where the answer is known
# =================================================================================================
def test_linear_case_on_the_device(cuda):
    """The case of test_genetic_cpu.test_oracle_attack_on_a_linear_classifier through a one-layer Model: at eps = 0.9 d no row ever
    succeeds (a theorem: the fp32 logits of a row inside the ball differ from the exact ones by ~1e-6 of a margin that is at least
    0.1 d ||w||_1), at eps = 4 d every row succeeds within the budget fixed there (twice the oracle's worst row).  The device's
    trajectory may leave the oracle's at an ambiguous draw: the assertion is success within the budget, not equal iterates."""
    from lipasr.attacks import GeneticAttack, TensorFlowV2Classifier

    W, bias, x, d, cls = G.linear_case_inf()
    spec = [P.LayerSpec(880, 2, False, 0.0, False)]
    m = build_model(spec)
    load_params(m, P.Params(W=[W], b=[bias], gamma=[None], beta=[None], mov_mean=[None], mov_var=[None]))
    clf = TensorFlowV2Classifier(model=m, nb_classes=2, input_shape=(880,))
    np.testing.assert_array_equal(clf.predict(x).argmax(axis=1), cls)
    kw = dict(pop_size=G.LINEAR["pop"], mutation_p=G.LINEAR["mutation_p"], temperature=G.LINEAR["temperature"], seed=G.LINEAR_SEED,
              max_iter=LINEAR_BUDGET)
    small_ = GeneticAttack(clf, 0.9 * d.min(), **kw)
    adv = small_.generate(x)
    assert not small_.success_.any() and (small_.queries_ == 16 * LINEAR_BUDGET).all() and (small_.fitness_ < 0).all()
    assert G.within_ball(adv, x, 0.9 * d.min()) and (clf.predict(adv).argmax(axis=1) == cls).all()
    eps = 4.0 * d.max()
    big = GeneticAttack(clf, eps, **kw)
    adv = big.generate(x)
    print(f"device, eps = 4 d: generations per row {(big.queries_ // 16).tolist()} (budget {LINEAR_BUDGET})")
    assert big.success_.all() and (big.queries_ <= 16 * LINEAR_BUDGET).all() and (big.fitness_ > 0).all()
    assert G.within_ball(adv, x, eps) and (clf.predict(adv).argmax(axis=1) != cls).all()


# =================================================================================================
# 5. small real models
# =================================================================================================
def _check_attack(atk, clf_predict, x, adv, labels, eps, clip, valid=None):
    """The properties of the issue on one call: the ball, the clip range, success_ against a fresh prediction, queries_."""
    P_, iters = atk.pop_size, atk.max_iter
    valid = np.ones(x.shape, dtype=bool) if valid is None else valid
    assert adv[~valid].tobytes() == x[~valid].tobytes(), "padding moved"
    assert G.within_ball(np.where(valid, adv, x), x, eps)
    assert adv[valid].min() >= np.float32(clip[0]) and adv[valid].max() <= np.float32(clip[1])
    ok, q = atk.success_.cpu().numpy(), atk.queries_.cpu().numpy()
    pred = clf_predict(adv).argmax(axis=1)
    hit = (pred == labels) if atk.targeted else (pred != labels)
    np.testing.assert_array_equal(ok, hit)
    assert (q % P_ == 0).all() and (q[~ok] == P_ * iters).all() and ((q[ok] >= P_) & (q[ok] <= P_ * iters)).all()
    fit = atk.fitness_.cpu().numpy()
    assert ((fit > 0) == ok).all()
    return ok, q


def test_attack_over_mfcc_rows_of_a_real_model(cuda):
    from lipasr.attacks import GeneticAttack, TensorFlowV2Classifier

    # the unconstrained 880 -> 10 model: in the float64 oracle with these settings 7 of the 8 rows leave their class after 1 .. 17
    # generations and one does not in 20 (on the constrained oracle model none does at eps 0.5 and one at eps 1)
    spec = P.vd_unconstrained_spec()
    m = build_model(spec)
    load_params(m, R.setup_params(spec, 3))
    clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
    clip = (-2.0, 2.0)
    x = np.clip(np.random.default_rng(3).standard_normal((8, 880)), *clip).astype(np.float32)
    own = clf.predict(x).argmax(axis=1)
    kw = dict(pop_size=8, max_iter=20, mutation_p=0.05, seed=1, clip_values=clip, check_every=5)
    eps = 0.5
    atk = GeneticAttack(clf, eps, **kw)
    assert GeneticAttack(clf, eps).clip_values is None  # a TensorFlowV2Classifier has no clip_values
    adv = atk.generate(x)
    ok, q = _check_attack(atk, clf.predict, x, adv, own, eps, clip)
    print(f"unconstrained 880 -> 10, eps {eps}: {int(ok.sum())} of 8 rows left their class, generations {(q // 8).tolist()}")
    assert ok.any()
    # queries_ is pop_size x the generations to done: with exactly that many generations the first clips to finish finish, no other does
    first = int(q[ok].min()) // 8
    short = GeneticAttack(clf, eps, **dict(kw, max_iter=first))
    adv_short = short.generate(x)
    np.testing.assert_array_equal(short.success_.cpu().numpy(), q == 8 * first)
    assert adv_short[q == 8 * first].tobytes() == adv[q == 8 * first].tobytes()
    # targeted: where it succeeds it lands on the target
    target = (own + 1) % 10
    tgt = GeneticAttack(clf, eps, targeted=True, **kw)
    adv_t = tgt.generate(x, np.eye(10, dtype=np.float32)[target])
    ok_t, _ = _check_attack(tgt, clf.predict, x, adv_t, target, eps, clip)
    print(f"targeted: {int(ok_t.sum())} of 8 rows reached class own + 1")
    assert (clf.predict(adv_t).argmax(axis=1)[ok_t] == target[ok_t]).all()


RAGGED = [16000, 9000, 37]


@pytest.fixture(scope="module")
def audio(cuda):
    """Three synthetic clips of 16000, 9000 and 37 samples in rows of 16000 at 16 kHz as 22 050 Hz rows, and a WaveformClassifier
    over the unconstrained 880 -> 10 model (the fixture of tests/test_smoothing_gpu.py)."""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, R.setup_params(spec, 3))
    ex = MfccExtractor(16000, 16000, batch_max=32)
    w = np.asarray(synth_clips(3, seed=31)[0], dtype=np.float32)
    for r, n in enumerate(RAGGED):
        w[r, n:] = 0
    lt = torch.as_tensor(np.array(RAGGED, dtype=np.int32)).to(cuda)
    rows = ex.resample(torch.as_tensor(w).to(cuda).contiguous(), n_valid=lt)
    yield dict(lt=lt, rows=rows, clf=WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k"))
    ex.close()


def test_attack_over_audio_with_lengths(audio):
    from lipasr.attacks import GeneticAttack

    clf, rows, lt = audio["clf"], audio["rows"], audio["lt"]
    x = rows.cpu().numpy()
    assert x.shape == (3, 22050)
    pos = [int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED]
    valid = np.arange(22050)[None, :] < np.array(pos)[:, None]
    own = clf.predict_device(rows, lengths=lt).argmax(dim=1).cpu().numpy()
    eps = 0.02
    atk = GeneticAttack(clf, eps, pop_size=4, max_iter=6, mutation_p=0.01, seed=2, check_every=3)
    assert atk.clip_values == (-1.0, 1.0)  # the estimator's
    adv = atk.generate_device(rows, lengths=lt).cpu().numpy()
    predict = lambda a: clf.predict_device(torch.as_tensor(a).cuda(), logits=True, lengths=lt).cpu().numpy()
    ok, q = _check_attack(atk, predict, x, adv, own, eps, (-1.0, 1.0), valid)
    print(f"audio 3 x 22050 with lengths, eps {eps}: success {ok.tolist()} generations {(q // 4).tolist()}")
    assert (np.abs(adv - x)[valid] > 0).mean() > 0.001  # the members did move inside the clips
    # a narrower clip range is respected inside the clips, and the padding still carries the bits of x
    tight = GeneticAttack(clf, eps, pop_size=4, max_iter=2, mutation_p=0.01, seed=2, clip_values=(-0.05, 0.05))
    adv = tight.generate_device(rows, lengths=lt).cpu().numpy()
    assert adv[valid].min() >= np.float32(-0.05) and adv[valid].max() <= np.float32(0.05) and adv[~valid].tobytes() == x[~valid].tobytes()
    # no lengths: the whole row is the clip
    free = GeneticAttack(clf, eps, pop_size=4, max_iter=2, mutation_p=0.01, seed=2)
    adv = free.generate_device(rows).cpu().numpy()
    assert G.within_ball(adv, x, eps) and (adv != x)[~valid].any()


# =================================================================================================
# 6. the menu
# =================================================================================================
def test_menu_runs_the_genetic_sweep(cuda, tmp_path, capsys):
    from lipasr import attack_eval as V
    from lipasr.extract_features_construct_dataset import compute_mfcc_all_files
    from lipasr.synth import synth_clips

    waves, lab = synth_clips(12, seed=31)
    files = []
    for i in range(12):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(waves[i], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = compute_mfcc_all_files(files)
    lab = np.asarray(lab).astype(np.int64) % 10
    lab[-1] = 9  # main() sizes the one-hot labels by the largest test label
    data, noise = tmp_path / "processed", tmp_path / "noise"
    data.mkdir()
    noise.mkdir()
    for name, sl in (("train", slice(0, 4)), ("dev", slice(4, 8)), ("test", slice(8, 12))):
        np.save(data / f"{name}_data.npy", feats[sl])
        np.save(data / f"{name}_label.npy", lab[sl])
    np.save(noise / "test_filenames.npy", np.array(files[8:12]))
    np.save(noise / "test_label.npy", lab[8:12])
    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, R.setup_params(spec, 3))
    h5 = str(tmp_path / "model.h5")
    m.save(h5)
    base = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--attack", "black", "--kind",
            "genetic", "--points", "1", "--pop-size", "4", "--max-iter", "3"]
    capsys.readouterr()
    grid, acc, queries = V.main(base)
    out = capsys.readouterr().out
    assert len(grid) == 1 and np.isclose(grid[0], 0.01) and set(acc) == set(queries) == {"constrained", "unconstrained"}
    assert all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
    assert "Accuracy on genetic black-box test examples" in out and "mean queries of those" in out
    grid, acc, queries = V.main(base + ["--over", "audio"])
    out = capsys.readouterr().out
    assert grid == V.GENETIC_AUDIO_EPS[:1] and all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
    assert "Accuracy on genetic black-box audio test examples unconstrained" in out
    with pytest.raises(ValueError):
        V.genetic_sweep({"constrained": m}, feats[:4], feats[4:8], feats[8:], np.eye(10)[lab[8:12]], over="audio")
