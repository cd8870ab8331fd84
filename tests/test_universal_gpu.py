"""The universal perturbation on the MI355X: lipasr_universal_{shifts,apply,reduce,step} against the NumPy restatement of
tests/universal_ref.py and against their host twins, lipasr.universal.UniversalPerturbation against a hand-built chain of the four
wrappers around the estimator, and the attack end to end where the answer is known, on a real model with held-out rows, over audio
with lengths, through a room and from the menu.

Bounds.  shifts, apply, reduce and step under norm inf: bits (integer arithmetic, single fp32 additions, clamps, fp64 additions
in a stated order), at element offsets 0 and 1 of the allocations and into outputs pre-filled with 7.0.  step under norm 2:
against the float64 restatement, 8 x the worst error over the cases of the shape of the same restatement run in float32, no
floor (tests/test_universal_cpu.py, step2_errors).  Measured on the MI355X: worst error per shape 6e-9 to 3e-8 -- the one rounding
to float32 -- which uses 0.03 to 0.125 of the bound (printed per shape)."""
import functools
import math
import wave

import numpy as np
import pytest
import torch

import local_lip_ref as LR
import universal_ref as R
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P
from test_genetic_gpu import RAGGED, SMALL, audio, small  # noqa: F401  (the fixtures of the genetic tests)
from test_universal_cpu import (HELD, INF, SHAPES, cases, held_out_case, ids, linear_rows, oracle_model, random_sign_rates, rows, same,
                                same_but_nan, step2_cases, step2_errors)

pytestmark = pytest.mark.gpu


def _place(x, offset=0, fill=0.0):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation."""
    x = np.asarray(x)
    buf = torch.full((x.size + offset,), fill, device="cuda", dtype=torch.as_tensor(x[:0]).dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _out(shape, offset, dtype=torch.float32):
    """An output of ``shape`` pre-filled with 7.0 that starts ``offset`` elements into its allocation."""
    size = int(np.prod(shape))
    return torch.full((size + offset,), 7.0, device="cuda", dtype=dtype)[offset:].view(*shape)


def _opt(a, offset):
    return None if a is None else _place(a, offset)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Inputs, cases and the restatement's results for a shape, computed once and left unchanged."""
    B, n, P_ = shape
    x, noise = rows(B, n, 1), rows(1, P_, 2, 0.2)[0]
    x[0, 0] = math.nan
    x[-1, -1] = -math.nan
    g = rows(B, n, 3, 1.0) * np.float32(10.0) ** np.random.default_rng(4).integers(-6, 6, (B, n)).astype(np.float32)
    g[0, 0] = math.nan
    g[-1, n // 2] = math.nan
    out = []
    for name, offs, nv in cases(shape):
        out.append(dict(name=name, offs=offs, nv=nv, apply=R.apply(x, noise, offs, nv, -0.25, 0.3), reduce=R.reduce(g, P_, offs, nv)))
    return x, noise, g, out


# =================================================================================================
# 1. the four kernels
# =================================================================================================
def test_shifts_equal_the_host_twin_and_the_restatement(cuda):
    from lipasr import _native as N
    from lipasr.universal import universal_shifts

    for P_, batch, clip0, it in ((1, 5, 0, 0), (7, 4096, 0, 0), (880, 130, 9, 5), (22050, 1024, 64, R.EVAL_IT + 3), (1 << 17, 300, 1 << 20, 7)):
        for offset in (0, 1):
            out = torch.full((batch + offset,), 7, dtype=torch.int32, device="cuda")[offset:]
            got = universal_shifts(batch, P_, it, 0x1234567890ABCDEF, clip0=clip0, out=out).cpu().numpy()
            assert same(got, N.universal_shifts_host(batch, P_, it, 0x1234567890ABCDEF, clip0=clip0))
            assert (got >= 0).all() and (got < P_).all()
        if batch <= 300:
            assert same(got, R.shifts(batch, P_, it, 0x1234567890ABCDEF, clip0=clip0))
    whole = universal_shifts(130, 1000, 2, 11).cpu().numpy()
    parts = np.concatenate([universal_shifts(b, 1000, 2, 11, clip0=c).cpu().numpy() for c, b in ((0, 1), (1, 63), (64, 66))])
    assert same(whole, parts)
    assert (np.bincount(universal_shifts(4096, 7, 0, 1).cpu().numpy(), minlength=7) > 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_apply_equals_the_host_twin_and_the_restatement(cuda, shape):
    from lipasr import _native as N
    from lipasr.universal import universal_apply

    B, n, P_ = shape
    x, noise, _, ref = reference(shape)
    for k, c in enumerate(ref):
        o = (k % 2, (k // 2) % 2, 1 - k % 2)  # the element offsets of x, noise and out
        out = _out((B, n), o[2])
        got = universal_apply(_place(x, o[0]), _place(noise, o[1]), offs=_opt(c["offs"], o[0]), n_valid=_opt(c["nv"], o[1]),
                              clip_values=(-0.25, 0.3), out=out)
        assert got.data_ptr() == out.data_ptr()
        got = got.cpu().numpy()
        assert same_but_nan(got, c["apply"]), c["name"]
        assert same_but_nan(got, N.universal_apply_host(x, noise, offs=c["offs"], n_valid=c["nv"], clip_lo=-0.25, clip_hi=0.3)), c["name"]
        keep = np.arange(n)[None, :] >= (np.full(B, n) if c["nv"] is None else np.clip(c["nv"], 0, n))[:, None]
        assert same(got[keep], x[keep]), c["name"]  # the padding keeps x's bits, a NaN's included
    free = universal_apply(_place(x, 1), _place(noise, 0)).cpu().numpy()  # no clip range, a new tensor
    assert same_but_nan(free, R.apply(x, noise)) and np.isnan(free[0, 0])
    xt = _place(x)
    with pytest.raises(ValueError, match="out overlaps x"):
        universal_apply(xt, _place(noise), out=xt)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_reduce_equals_the_host_twin_and_the_restatement(cuda, shape):
    from lipasr import _native as N
    from lipasr.universal import universal_reduce

    B, n, P_ = shape
    _, _, g, ref = reference(shape)
    groups = (B + 63) // 64
    for k, c in enumerate(ref):
        o = (k % 2, (k // 2) % 2, 1 - k % 2)
        gt, ot, nt = _place(g, o[0]), _opt(c["offs"], o[1]), _opt(c["nv"], o[0])
        sums = _out((groups, P_), o[2], torch.float64)
        got = universal_reduce(gt, P_, offs=ot, n_valid=nt, sums=sums)
        assert got.data_ptr() == sums.data_ptr()
        got = got.cpu().numpy()
        assert same(got, c["reduce"]), c["name"]
        assert same(got, N.universal_reduce_host(g, P_, offs=c["offs"], n_valid=c["nv"])), c["name"]
        assert np.isfinite(got).all()  # a NaN counts as 0
        again = universal_reduce(gt, P_, offs=ot, n_valid=nt).cpu().numpy()  # a second run, another output: the same bits
        assert same(again, got), c["name"]


def test_reduce_is_the_sum_of_the_rows_and_cuts_at_the_group(cuda):
    from lipasr.universal import universal_reduce

    g = rows(130, 36, 5, 1.0)
    gt = dev(g)
    for P_ in (36, 50):
        want = np.zeros((3, P_))
        for b in range(130):
            want[b // 64, :36] += g[b].astype(np.float64)
        assert same(universal_reduce(gt, P_).cpu().numpy(), want)
    offs, nv = R.shifts(130, 12, 0, 5), np.array(([0, 1, 36, 39, -2, 18, 35] * 19)[:130], dtype=np.int32)
    ot, nt = _place(offs), _place(nv)
    whole = universal_reduce(gt, 12, offs=ot, n_valid=nt).cpu().numpy()
    head = universal_reduce(gt[:64], 12, offs=ot[:64], n_valid=nt[:64]).cpu().numpy()
    tail = universal_reduce(gt[64:], 12, offs=ot[64:], n_valid=nt[64:]).cpu().numpy()
    assert same(whole, np.concatenate([head, tail])) and same(whole, R.reduce(g, 12, offs, nv))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_step_inf_equals_the_host_twin_and_the_restatement(cuda, shape):
    from lipasr import _native as N
    from lipasr.universal import universal_step

    B, n, P_ = shape
    groups = (B + 63) // 64
    sums = np.random.default_rng(8).standard_normal((groups, P_))
    sums[:, ::3] = 0.0
    if P_ > 4:
        sums[0, 1], sums[0, 2], sums[-1, 4] = INF, -INF, math.nan
    if groups > 1 and P_ > 7:
        sums[0, 7], sums[1, 7] = 1.5, -1.5
    noise0 = rows(1, P_, 9, 0.1)[0]
    noise0[0] = -0.0
    k = 0
    for alpha in (0.05, -0.05, 0.0):
        for eps in (0.12, 0.0, INF):
            k += 1
            noise = _place(noise0, k % 2)
            got = universal_step(noise, _place(sums, (k // 2) % 2), np.inf, alpha, eps)
            assert got.data_ptr() == noise.data_ptr()
            got = got.cpu().numpy()
            assert same(got, R.step(noise0, sums, np.inf, alpha, eps)), (alpha, eps)
            assert same(got, N.universal_step_host(noise0.copy(), sums, np.inf, alpha, eps)), (alpha, eps)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_step_2_within_the_float32_yardstick(cuda, shape):
    from lipasr.universal import universal_step

    flip = [0]

    def run(noise, sums, alpha, eps):
        flip[0] += 1
        return universal_step(_place(noise, flip[0] % 2), _place(sums, (flip[0] // 2) % 2), 2, alpha, eps).cpu().numpy()

    err, yard = step2_errors(run, shape)
    print(f"step norm 2 {ids(shape)}: worst error {err:.3e}, float32 restatement {yard:.3e}, ratio of the bound used {err / (8 * yard) if yard else 0:.3f}")
    assert err <= 8 * yard
    # two runs, the same bits; and a sum that is not finite takes no step: the call only projects
    noise, sums, alpha, eps = next(iter(step2_cases(shape)))
    assert same(run(noise, sums, alpha, eps), run(noise, sums, alpha, eps))
    for bad in (INF, math.nan):
        s = sums.copy()
        s[-1, -1] = bad
        assert same(run(noise, s, alpha, INF), noise)
        got = run(noise, s, alpha, 0.05)
        assert np.abs(got.astype(np.float64) - R.step(noise, s, 2, alpha, 0.05)).max() <= 8 * yard


def test_step_2_at_the_largest_period(cuda):
    """P = 2^17: every thread of the one workgroup takes 128 positions, 16 groups of partials."""
    from lipasr.universal import universal_step

    rng = np.random.default_rng(21)
    P_ = 1 << 17
    sums, noise = rng.standard_normal((16, P_)), (0.01 * rng.standard_normal(P_)).astype(np.float32)
    want = R.step(noise, sums, 2, 0.5, 1.0)
    yard = np.abs(R.step(noise, sums, 2, 0.5, 1.0, dtype=np.float32).astype(np.float64) - want).max()
    got = universal_step(dev(noise), torch.as_tensor(sums).cuda(), 2, 0.5, 1.0).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"step norm 2, P = 2^17: error {err:.3e}, float32 restatement {yard:.3e}")
    assert err <= 8 * yard


def test_wrappers_check_their_tensors(cuda):
    from lipasr.universal import universal_apply, universal_reduce, universal_shifts, universal_step

    x, noise = dev(rows(3, 8, 0)), dev(rows(1, 5, 1)[0])
    i32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int32)).cuda()
    for bad in (dict(offs=i32([0, 1])), dict(offs=torch.zeros(3, device="cuda")), dict(n_valid=i32([1, 2, 3, 4])),
                dict(out=torch.empty(3, 9, device="cuda"))):
        with pytest.raises(ValueError):
            universal_apply(x, noise, **bad)
    with pytest.raises(ValueError):
        universal_apply(x.cpu(), noise)
    with pytest.raises(ValueError):
        universal_apply(x, noise.double())
    with pytest.raises(ValueError):
        universal_reduce(x, 5, sums=torch.empty(1, 5, device="cuda"))
    with pytest.raises(ValueError):
        universal_reduce(x, 5, sums=torch.empty(2, 5, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        universal_step(noise, torch.empty(1, 6, dtype=torch.float64, device="cuda"), np.inf, 0.1, 0.1)
    with pytest.raises(ValueError):
        universal_step(noise, torch.empty(1, 5, dtype=torch.float64, device="cuda"), 1, 0.1, 0.1)
    with pytest.raises(ValueError):
        universal_shifts(4, 5, -1, 0)
    assert universal_shifts(0, 5, 0, 0).shape == (0,) and universal_reduce(x[:0], 5).shape == (0, 5)


# =================================================================================================
# 2. UniversalPerturbation against the hand-built chain
# =================================================================================================
@pytest.mark.parametrize("norm,eps,kw", [(np.inf, 0.3, {}), (2, 1.5, {}), (np.inf, 0.3, dict(length=10, random_shift=True)),
                                         (2, 1.5, dict(length=50, random_shift=True, targeted=True))],
                         ids=["inf", "2", "inf-loop-shift", "2-window-shift-targeted"])
def test_generate_equals_the_hand_built_chain(small, norm, eps, kw):
    from lipasr.attacks import UniversalPerturbation
    from lipasr.universal import universal_apply, universal_reduce, universal_shifts, universal_step

    clf, xt = small["clf"], dev(small["x"])
    B, n, bs, epochs, step = 5, 36, 2, 3, eps / 4
    P_, shift, targeted = kw.get("length") or n, kw.get("random_shift", False), kw.get("targeted", False)
    own = clf.predict_device(xt, logits=True).argmax(dim=1)
    y = ((own + 1) % 5) if targeted else None
    atk = UniversalPerturbation(clf, delta=0.0, max_iter=epochs, eps=eps, eps_step=step, norm=norm, batch_size=bs, seed=4, **kw)
    adv = atk.generate_device(xt, y)
    labels = y if targeted else own
    onehot = torch.nn.functional.one_hot(labels, 5).float()
    noise = torch.zeros(P_, device="cuda")
    seed = (UniversalPerturbation._SEED + 4) & 0xFFFFFFFFFFFFFFFF
    done = 0
    for epoch in range(epochs):
        offs = universal_shifts(B, P_, epoch, seed) if shift else None
        for s in range(0, B, bs):
            o = None if offs is None else offs[s:s + bs]
            xa = universal_apply(xt[s:s + bs], noise, offs=o)
            g = clf.loss_gradient_device(xa, onehot[s:s + bs])
            universal_step(noise, universal_reduce(g, P_, offs=o), norm, -step if targeted else step, eps)
        done = epoch + 1
        eo = universal_shifts(B, P_, R.EVAL_IT + epoch, seed) if shift else None
        pred = clf.predict_device(universal_apply(xt, noise, offs=eo), logits=True).argmax(dim=1)
        rate = float(((pred == labels) if targeted else (pred != labels)).double().mean())
        if rate >= 1.0:
            break
    assert same(atk.noise_.cpu().numpy(), noise.cpu().numpy()) and same(atk.noise, noise.cpu().numpy())
    assert atk.epochs_ == done and atk.fooling_rate == rate and atk.converged == (rate >= 1.0)
    assert same(adv.cpu().numpy(), universal_apply(xt, noise).cpu().numpy()) and adv.data_ptr() != xt.data_ptr()
    assert np.abs(atk.noise).max() > 0
    if norm == np.inf:
        assert np.abs(atk.noise).max() <= np.float32(eps)
    else:
        assert np.linalg.norm(atk.noise.astype(np.float64)) <= eps * (1 + 1e-6)
    # NumPy in, NumPy out; labels as indices or one-hot; apply on rows the fit never saw, at shifts of the caller's
    y_np = None if y is None else y.cpu().numpy()
    for yy in ((y_np,) if targeted else (None, own.cpu().numpy(), onehot.cpu().numpy())):
        assert same(atk.generate(small["x"], yy), adv.cpu().numpy())
    other = np.random.default_rng(5).standard_normal((3, 36)).astype(np.float32)
    assert same(atk.apply(other), R.apply(other, atk.noise))
    assert same(atk.apply(other, offs=[1, 0, P_ - 1]), R.apply(other, atk.noise, np.array([1, 0, P_ - 1])))
    with pytest.raises(ValueError):
        atk.generate_device(xt, y, lengths=[36] * 5)
    with pytest.raises(ValueError):
        atk.generate_device(xt[:, :35], y)
    if targeted:
        with pytest.raises(ValueError, match="Target labels"):
            atk.generate_device(xt)


def test_constructor_refusals(small):
    from lipasr.attacks import UniversalPerturbation

    clf = small["clf"]
    for kw in (dict(attacker="deepfool"), dict(delta=1.5), dict(max_iter=0), dict(eps=-1.0), dict(eps_step=-0.1), dict(norm=1), dict(batch_size=0),
               dict(length=0), dict(length=(1 << 17) + 1)):
        with pytest.raises(ValueError):
            UniversalPerturbation(clf, **kw)
    atk = UniversalPerturbation(clf, eps=0.5)
    assert atk.eps_step == 0.05 and atk.clip_values is None and atk.norm == math.inf
    with pytest.raises(RuntimeError):
        atk.apply(small["x"])


# =================================================================================================
# 3. known answers
# =================================================================================================
def test_known_answer_linear_one_class(cuda):
    """tests/test_universal_cpu.py, test_known_answer_linear_one_class, through a one-layer Model."""
    from lipasr.attacks import TensorFlowV2Classifier, UniversalPerturbation

    spec, p, x, w, eps = linear_rows()
    m = build_model(spec)
    load_params(m, p)
    clf = TensorFlowV2Classifier(model=m, nb_classes=2, input_shape=(880,))
    assert (clf.predict(x).argmax(axis=1) == 0).all()
    batches = -(-len(x) // 2)
    atk = UniversalPerturbation(clf, delta=0.0, max_iter=-(-4 // batches) + 1, eps=eps, eps_step=eps / 4, batch_size=2)
    adv = atk.generate(x)
    assert (eps / 4) * batches * atk.epochs_ >= eps and not atk.converged and atk.fooling_rate == 0.0
    nz = w != 0
    assert same(atk.noise[nz], (np.float32(eps) * np.sign(w[nz])).astype(np.float32))
    assert same(adv, R.apply(x, atk.noise))


def test_known_answer_held_out_generalisation(cuda):
    """The fixture of tests/test_universal_cpu.py on the device: the same two assertions, and the bookkeeping of the class.
    Measured on the MI355X: held-out fooling rate 0.78 against a largest random 0.23; cross-entropy 1.51 -> 2.14."""
    from lipasr.attacks import TensorFlowV2Classifier, UniversalPerturbation

    spec, p, fit_rows, held = held_out_case()
    m = build_model(spec, max_batch=64)
    load_params(m, p)
    clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
    predict = lambda a: clf.predict_device(dev(a), logits=True).cpu().numpy()
    own_fit, own_held = predict(fit_rows).argmax(axis=1), predict(held).argmax(axis=1)
    atk = UniversalPerturbation(clf, delta=HELD["delta"], max_iter=HELD["max_iter"], eps=HELD["eps"], eps_step=HELD["eps_step"],
                                batch_size=HELD["batch_size"], clip_values=HELD["clip"])
    adv = atk.generate(fit_rows)
    lo, hi = HELD["clip"]
    assert np.abs(atk.noise).max() <= np.float32(HELD["eps"]) and np.abs(atk.noise).max() > 0  # within the ball
    assert same(adv, atk.apply(fit_rows)) and same(adv, R.apply(fit_rows, atk.noise, lo=lo, hi=hi))
    assert atk.fooling_rate == float((predict(adv).argmax(axis=1) != own_fit).mean())
    rate = float((predict(atk.apply(held)).argmax(axis=1) != own_held).mean())
    random = random_sign_rates(predict, held, own_held)

    def ce(a):
        logp = torch.log_softmax(clf.predict_device(dev(a), logits=True).double(), dim=1).cpu().numpy()
        return float(-logp[np.arange(len(a)), own_fit].mean())

    ce0, ce1 = ce(fit_rows), ce(adv)
    print(f"held-out fooling rate {rate:.3f} against random sign vectors {max(random):.3f} (all: {random}); fitting rows: fooling rate "
          f"{atk.fooling_rate:.3f} after {atk.epochs_} epochs, mean CE {ce0:.3f} -> {ce1:.3f}")
    assert rate > max(random)
    assert ce1 > ce0


# =================================================================================================
# 4. audio with lengths, and through a room
# =================================================================================================
def _ball(noise, eps, norm):
    if norm == np.inf:
        return np.abs(noise).max() <= np.float32(eps)
    return np.linalg.norm(noise.astype(np.float64)) <= eps * (1 + 1e-6)


@pytest.mark.parametrize("shift", [False, True], ids=["fixed", "shift"])
@pytest.mark.parametrize("norm,eps", [(np.inf, 0.02), (2, 0.5)])
def test_attack_over_audio_with_lengths(audio, norm, eps, shift):
    from lipasr.attacks import UniversalPerturbation

    clf, xt, lt = audio["clf"], audio["rows"], audio["lt"]
    x = xt.cpu().numpy()
    assert x.shape == (3, 22050)
    pos = [int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED]
    valid = np.arange(22050)[None, :] < np.array(pos)[:, None]
    atk = UniversalPerturbation(clf, delta=0.0, max_iter=3, eps=eps, norm=norm, batch_size=2, random_shift=shift, seed=3)
    assert atk.clip_values == (-1.0, 1.0)  # the estimator's
    adv = atk.generate_device(xt, lengths=lt).cpu().numpy()
    assert same(adv[~valid], x[~valid]), "padding moved"
    assert adv[valid].min() >= -1.0 and adv[valid].max() <= 1.0
    assert atk.noise.shape == (22050,) and _ball(atk.noise, eps, norm) and (atk.noise != 0).mean() > 0.5  # the noise moved
    assert same(adv, R.apply(x, atk.noise, None, np.array(pos, dtype=np.int32), -1.0, 1.0))
    if norm == np.inf:
        assert np.abs(adv - x)[valid].max() <= np.float32(eps) * (1 + 2.0 ** -23) + np.spacing(np.float32(1.0))
    else:
        assert np.linalg.norm((adv - x).astype(np.float64), axis=1).max() <= eps * (1 + 1e-5)
    print(f"audio 3 x 22050 with lengths, norm {norm}, eps {eps}, shift {shift}: fooling rate {atk.fooling_rate:.2f} after {atk.epochs_} epochs")


def test_through_a_room_that_is_the_identity(audio):
    """OverTheAirClassifier with the bank [[1.0]] hears what the WaveformClassifier hears: the same noise bit for bit."""
    from lipasr.attacks import OverTheAirClassifier, UniversalPerturbation
    from lipasr.room import RoomChannel

    clf, xt, lt = audio["clf"], audio["rows"], audio["lt"]
    air = OverTheAirClassifier(clf, RoomChannel(np.ones((1, 1), dtype=np.float32)))
    noises = []
    for est in (clf, air):
        atk = UniversalPerturbation(est, delta=0.0, max_iter=2, eps=0.02, batch_size=2, length=4000, random_shift=True, seed=1)
        atk.generate_device(xt, lengths=lt)
        noises.append(atk.noise)
    assert same(noises[0], noises[1]) and np.abs(noises[0]).max() > 0


def test_short_window_extractor_without_lengths(cuda):
    from lipasr.attacks import UniversalPerturbation, WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor

    spec = P.sr_constrained_spec()  # 2 020 features (20 x 101 frames of the short window), 20 speakers
    m = build_model(spec, max_batch=16)
    load_params(m, LR.setup_params(spec, 4))
    ex = MfccExtractor(22050, 22050, batch_max=8, n_fft=441, hop=220)
    try:
        clf = WaveformClassifier(m, 20, extractor=ex, utterance_length=101, domain="22k")
        w = np.random.default_rng(2).uniform(-0.5, 0.5, (3, 22050)).astype(np.float32)
        atk = UniversalPerturbation(clf, delta=0.0, max_iter=2, eps=0.01, batch_size=2)
        adv = atk.generate(w)
        assert same(adv, R.apply(w, atk.noise, lo=-1.0, hi=1.0)) and (atk.noise != 0).mean() > 0.5
        with pytest.raises(ValueError):
            atk.generate(w, lengths=[22050] * 3)
    finally:
        ex.close()


# =================================================================================================
# 5. the menu
# =================================================================================================
def test_menu_runs_the_universal_sweep(cuda, tmp_path, capsys):
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
    load_params(m, LR.setup_params(spec, 3))
    h5 = str(tmp_path / "model.h5")
    m.save(h5)
    base = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--attack", "white", "--kind",
            "universal", "--points", "1", "--max-iter", "2"]
    capsys.readouterr()
    for extra, first in (([], 0.01), (["--norm", "2"], 1.0), (["--shift", "--length", "100"], 0.01), (["--over", "audio"], V.AUDIO_SIGMAS[1]),
                         (["--over", "audio", "--norm", "2", "--shift", "--length", "4000"], V.AUDIO_SIGMAS[1]),
                         (["--over", "audio", "--room", "2", "--room-taps", "64"], V.AUDIO_SIGMAS[1])):
        grid, acc, fooled = V.main(base + extra)
        out = capsys.readouterr().out
        assert len(grid) == 1 and np.isclose(grid[0], first) and set(acc) == set(fooled) == {"constrained", "unconstrained"}
        assert all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for d in (acc, fooled) for v in d.values())
        assert "under a universal perturbation: " in out and "under a universal perturbation unconstrained: " in out
        assert "fooling rate on the 2 fitting " in out
    with pytest.raises(ValueError):
        V.main(base + ["--norm", "1"])
    with pytest.raises(ValueError):
        V.main(base + ["--room", "2"])
