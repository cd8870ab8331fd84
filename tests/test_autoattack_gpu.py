"""AutoAttack on the MI355X: the ensemble against the hand composition of its members on the shrinking robust subset, bit for
bit; the ball predicate (tests/apgd_ref.py::within_ball, row by row, on the host) applied to every member's result, DeepFool's
unbounded one included; rows misclassified when clean; norm 2.

Bounds: none -- the ensemble only gathers rows, calls its members and scatters their results, so every comparison is of bits."""
import numpy as np
import pytest
import torch

import apgd_ref as A
import local_lip_ref as L
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

SMALL = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
ROWS, WRONG = 48, (3, 17, 40)  # rows of the fixture; the rows whose given label is not the model's prediction
EPS = 0.12  # see test_equals_the_hand_composition


@pytest.fixture(scope="module")
def small(cuda):
    from lipasr.attacks import TensorFlowV2Classifier

    m = build_model(SMALL, max_batch=64)
    load_params(m, L.setup_params(SMALL, 2))
    clf = TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,))
    x = np.random.default_rng(14).standard_normal((ROWS, 36)).astype(np.float32)
    xt = dev(x)
    labels = clf.predict_device(xt, logits=True).argmax(dim=1)
    for r in WRONG:
        labels[r] = (labels[r] + 1) % 5
    return dict(model=m, clf=clf, x=x, xt=xt, labels=labels)


def members(clf, eps, norm, seed, shape=None, batch_size=32):
    """The list AutoAttack(attacks=None) is documented to build."""
    from lipasr.attacks import AutoProjectedGradientDescent, DeepFool, SquareAttack

    kw = dict(norm=norm, eps=eps, eps_step=0.1, batch_size=batch_size, seed=seed)
    out = [AutoProjectedGradientDescent(clf, loss_type="cross_entropy", **kw)]
    if clf.nb_classes >= 3:
        out.append(AutoProjectedGradientDescent(clf, loss_type="difference_logits_ratio", **kw))
    out.append(DeepFool(clf, batch_size=batch_size, verbose=False, norm=norm))
    if norm == np.inf:
        out.append(SquareAttack(clf, norm=np.inf, eps=eps, batch_size=batch_size, shape=shape, seed=seed))
    return out


def in_ball(cand, x, eps, norm):
    return np.array([A.within_ball(cand[i:i + 1], x[i:i + 1], eps, norm) for i in range(len(x))], dtype=bool)


def hand(clf, xt, labels, attacks, eps, norm):
    """Each member in turn on the rows that are still robust -> (adv, broken_by, robust counts after every member, what every
    member alone leaves robust of the rows it was handed)."""
    from lipasr.attacks import DeepFool

    pred = clf.predict_device(xt, logits=True).argmax(dim=1)
    robust = (pred == labels).cpu().numpy()
    broken_by = np.where(robust, -1, -2).astype(np.int32)
    adv = xt.clone()
    counts, alone = [int(robust.sum())], []
    for i, atk in enumerate(attacks):
        idx = np.flatnonzero(robust)
        if idx.size == 0:
            break
        it = torch.as_tensor(idx).cuda()
        xs, ys = xt[it].contiguous(), labels[it]
        cand = atk.generate_device(xs) if isinstance(atk, DeepFool) else atk.generate_device(xs, ys)
        moved = (clf.predict_device(cand, logits=True).argmax(dim=1) != ys).cpu().numpy()
        ok = moved & in_ball(cand.cpu().numpy(), xs.cpu().numpy(), eps, norm)
        adv[it[torch.as_tensor(ok).cuda()]] = cand[torch.as_tensor(ok).cuda()]
        broken_by[idx[ok]] = i
        robust[idx[ok]] = False
        counts.append(int(robust.sum()))
        alone.append(int((~ok).sum()))
    return adv, broken_by, counts, alone


def test_equals_the_hand_composition(small):
    """48 rows of the 36 -> 16 -> 5 model (three of them given a wrong label) at eps = EPS = 0.12, chosen on the first run on the
    device as a radius at which the members disagree: of the 45 rows that are robust when clean APGD-CE breaks 29, APGD-DLR 3 of the
    16 it is handed, DeepFool and SquareAttack none of the 13 left (robust after each member: 45, 16, 13, 13, 13).  The assertion
    is that the ensemble is the composition, bit for bit; the counts are printed."""
    from lipasr.attacks import AutoAttack

    clf, xt, labels = small["clf"], small["xt"], small["labels"]
    auto = AutoAttack(clf, eps=EPS, seed=5, shape=(6, 6))
    assert [type(a).__name__ for a in auto.attacks] == ["AutoProjectedGradientDescent", "AutoProjectedGradientDescent", "DeepFool", "SquareAttack"]
    assert [getattr(a, "loss_type", None) for a in auto.attacks[:2]] == ["cross_entropy", "difference_logits_ratio"]
    assert auto.attacks[3].shape == (6, 6) and auto.attacks[3].eps == np.float64(EPS) and auto.attacks[0].eps_step == 0.1
    adv = auto.generate_device(xt, labels)
    want, broken_by, counts, alone = hand(clf, xt, labels, members(clf, EPS, np.inf, 5, (6, 6)), EPS, np.inf)
    per = [int((broken_by == i).sum()) for i in range(4)]
    print(f"eps {EPS}: robust after each member {counts}, broken per member {per}, each member alone leaves {alone} of the rows handed to it")
    assert adv.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and adv.data_ptr() != xt.data_ptr()
    np.testing.assert_array_equal(auto.broken_by_.cpu().numpy(), broken_by)
    assert auto.broken_by_.dtype == torch.int32 and auto.success_.dtype == torch.bool
    np.testing.assert_array_equal(auto.success_.cpu().numpy(), broken_by >= 0)
    assert auto.robust_accuracy_ == counts[-1] / ROWS
    # the robust accuracy is at most what each member leaves on its own over the rows it was handed
    assert all(counts[-1] <= a for a in alone) and all(b <= a for a, b in zip(counts, counts[1:]))
    assert 0 < counts[-1] < counts[0], "choose eps so that some rows break and some survive"
    # rows misclassified when clean come back untouched
    bad = list(WRONG)
    assert (broken_by[bad] == -2).all() and (broken_by == -2).sum() == len(bad)
    assert adv[bad].cpu().numpy().tobytes() == small["x"][bad].tobytes()
    # broken rows are misclassified inside the ball, the others are returned clean
    pred = clf.predict_device(adv, logits=True).argmax(dim=1).cpu().numpy()
    lab = labels.cpu().numpy()
    hit = broken_by >= 0
    assert (pred[hit] != lab[hit]).all() and in_ball(adv.cpu().numpy(), small["x"], EPS, np.inf).all()
    assert adv.cpu().numpy()[~hit].tobytes() == small["x"][~hit].tobytes()
    # y=None: the model's own predictions -- no row is misclassified when clean; NumPy in, NumPy out
    own = AutoAttack(clf, eps=EPS, seed=5, shape=(6, 6))
    out = own.generate(small["x"][:16])
    assert isinstance(out, np.ndarray) and (own.broken_by_ != -2).all() and own.robust_accuracy_ == float((own.broken_by_ == -1).double().mean())


def test_a_result_outside_the_ball_is_not_counted(small):
    """eps = 1e-4: DeepFool leaves the class of every one of the 16 rows, all but one (a row that sits within 1e-4 of its boundary)
    far outside a ball that small, and only what lies inside the ball counts."""
    from lipasr.attacks import AutoAttack, DeepFool

    clf, xt = small["clf"], small["xt"][:16].contiguous()
    eps = 1e-4
    fool = DeepFool(clf, batch_size=32, verbose=False, norm=np.inf)
    cand = fool.generate_device(xt)
    flipped = fool.last["flipped"].copy()
    inside = in_ball(cand.cpu().numpy(), small["x"][:16], eps, np.inf)
    assert (flipped & ~inside).sum() >= 8, "DeepFool must leave the ball on most rows for this test to say anything"
    auto = AutoAttack(clf, eps=eps, seed=5, attacks=[fool])
    adv = auto.generate_device(xt)
    counted = flipped & inside
    np.testing.assert_array_equal(auto.success_.cpu().numpy(), counted)
    np.testing.assert_array_equal(auto.broken_by_.cpu().numpy(), np.where(counted, 0, -1))
    assert auto.robust_accuracy_ == float((~counted).mean())
    assert adv.cpu().numpy()[~counted].tobytes() == small["x"][:16][~counted].tobytes()
    assert adv.cpu().numpy()[counted].tobytes() == cand.cpu().numpy()[counted].tobytes()
    full = AutoAttack(clf, eps=eps, seed=5)
    full.generate_device(xt)
    assert (full.broken_by_.cpu().numpy()[~inside] != 2).all()  # a DeepFool result outside the ball is never what broke a row
    wide = AutoAttack(clf, eps=100.0, seed=5, attacks=[fool])  # the same result counts once the ball holds it
    wide.generate_device(xt)
    np.testing.assert_array_equal(wide.success_.cpu().numpy(), fool.last["flipped"])


def test_norm_2_runs_three_attacks(small):
    from lipasr.attacks import AutoAttack

    clf, xt, labels = small["clf"], small["xt"][:24].contiguous(), small["labels"][:24]
    eps = 0.5
    auto = AutoAttack(clf, norm=2, eps=eps, seed=5)
    assert [type(a).__name__ for a in auto.attacks] == ["AutoProjectedGradientDescent", "AutoProjectedGradientDescent", "DeepFool"]
    adv = auto.generate_device(xt, labels)
    want, broken_by, counts, _ = hand(clf, xt, labels, members(clf, eps, 2, 5), eps, 2)
    print(f"norm 2, eps {eps}: robust after each member {counts}")
    assert adv.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    np.testing.assert_array_equal(auto.broken_by_.cpu().numpy(), broken_by)
    assert in_ball(adv.cpu().numpy(), small["x"][:24], eps, 2).all() and auto.success_.any()
    for bad in (dict(norm=1), dict(targeted=True), dict(eps=-1.0), dict(batch_size=0), dict(attacks=[object()])):
        with pytest.raises((ValueError, TypeError)):
            AutoAttack(clf, **bad)
    with pytest.raises(ValueError):
        auto.generate_device(xt, lengths=[36] * 24)


def test_over_audio_with_lengths(cuda):
    """Three clips of 16000, 9000 and 37 samples as 22 050 Hz rows through a WaveformClassifier, a short list of members: the
    ensemble hands every member the rows that are still robust WITH their lengths, the ball counts a clip's own samples only, and
    the rest of every row comes back bit for bit."""
    import math

    from lipasr.attacks import AutoAttack, AutoProjectedGradientDescent, SquareAttack, WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    ragged = [16000, 9000, 37]
    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, L.setup_params(spec, 3))
    ex = MfccExtractor(16000, 16000, batch_max=32)
    try:
        w = np.asarray(synth_clips(3, seed=31)[0], dtype=np.float32)
        for r, n in enumerate(ragged):
            w[r, n:] = 0
        lt = torch.as_tensor(np.array(ragged, dtype=np.int32)).to(cuda)
        rows = ex.resample(torch.as_tensor(w).to(cuda).contiguous(), n_valid=lt)
        clf = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
        x = rows.cpu().numpy()
        valid = np.arange(22050)[None, :] < np.array([int(math.ceil(n * 22050.0 / 16000.0)) for n in ragged])[:, None]
        eps = 0.004
        make = lambda: [AutoProjectedGradientDescent(clf, eps=eps, max_iter=6, nb_random_init=1, seed=5),
                        SquareAttack(clf, eps=eps, max_iter=8, seed=5)]
        auto = AutoAttack(clf, eps=eps, attacks=make())
        adv = auto.generate_device(rows, lengths=lt)
        a = adv.cpu().numpy()
        assert a[~valid].tobytes() == x[~valid].tobytes(), "padding moved"
        own = clf.predict_device(rows, logits=True, lengths=lt).argmax(dim=1)
        pred = clf.predict_device(adv, logits=True, lengths=lt).argmax(dim=1)
        np.testing.assert_array_equal(auto.success_.cpu().numpy(), (pred != own).cpu().numpy())
        assert all(A.within_ball(a[i:i + 1], x[i:i + 1], eps, np.inf, valid[i:i + 1]) for i in range(3))
        # the hand composition with lengths
        first, second = make()
        c0 = first.generate_device(rows, own, lengths=lt)
        hit0 = (clf.predict_device(c0, logits=True, lengths=lt).argmax(dim=1) != own).cpu().numpy()
        want, by = x.copy(), np.full(3, -1)
        want[hit0], by[hit0] = c0.cpu().numpy()[hit0], 0
        rest = np.flatnonzero(~hit0)
        if rest.size:
            it = torch.as_tensor(rest).cuda()
            c1 = second.generate_device(rows[it].contiguous(), own[it], lengths=lt[it].contiguous())
            hit1 = (clf.predict_device(c1, logits=True, lengths=lt[it].contiguous()).argmax(dim=1) != own[it]).cpu().numpy()
            want[rest[hit1]], by[rest[hit1]] = c1.cpu().numpy()[hit1], 1
        print(f"audio with lengths, eps {eps}: broken by {by.tolist()}")
        assert a.tobytes() == want.tobytes()
        np.testing.assert_array_equal(auto.broken_by_.cpu().numpy(), by)
    finally:
        ex.close()
