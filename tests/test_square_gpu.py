"""Square Attack on the MI355X: lipasr_square_init / lipasr_square_step against their host twins bit for bit (which
tests/test_square_cpu.py pins against the NumPy restatement), at buffer offsets 0 and 1; the window-only invariants; SquareAttack
against a hand-built chain of the calls and across chunk sizes; and the attack's properties on small real models over MFCC rows as
pictures and over audio with ragged lengths.

Bounds: none -- the kernels and the host twins are the same inline functions (integer arithmetic, one fp32 add, two clamps, one
fp32 subtract), so every comparison is of bits."""
import itertools
import math

import numpy as np
import pytest
import torch

import genetic_ref as G
import local_lip_ref as L
import square_ref as R
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P
from test_square_cpu import SHAPES, _logits, _rows, host_state, host_step, ids, same

pytestmark = pytest.mark.gpu


def _place(x, offset=0, dtype=torch.float32, fill=0.0):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation (test_genetic_gpu's idiom)."""
    buf = torch.full((x.size + offset,), fill, device="cuda", dtype=dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _i32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


def _device_chain(shape, seed, eps, iters, offs, n_valid=None, clip=None, restart=1, p=0.3, clip0=0):
    """``iters`` steps of the device kernels next to the host twins, on the logits of test_square_cpu.chain."""
    from lipasr.square import square_init, square_step

    B, height, width = shape
    n = height * width
    x0 = _rows(B, n, seed)
    labels = np.arange(B, dtype=np.int32) % 3
    nv = None if n_valid is None else np.asarray(n_valid, dtype=np.int32)
    lo, hi = (-math.inf, math.inf) if clip is None else clip
    host = host_state(x0, height, width, restart, seed, eps, n_valid=nv, clip0=clip0, clip_lo=lo, clip_hi=hi)
    junk = np.full((B, n), 7.0, dtype=np.float32)
    xt, best, cand = _place(x0, offs[0]), _place(junk, offs[1]), _place(junk, offs[2])
    win, loss, done = _i32(np.full((B, 4), 9)), torch.full((B,), 5.0, device="cuda"), _i32(np.zeros(B))
    nvt, lab = None if nv is None else _i32(nv), _i32(labels)
    kw = dict(x_best=best, x_cand=cand, win=win, n_valid=nvt, clip0=clip0, clip_values=clip)
    square_init(xt, height, width, restart, seed, eps, **kw)
    state = lambda: dict(x_best=best.cpu().numpy(), x_cand=cand.cpu().numpy(), win=win.cpu().numpy(), loss_best=loss.cpu().numpy(),
                         done=done.cpu().numpy())
    got = state()
    for k in ("x_best", "x_cand", "win"):
        assert same(got[k], host[k]), f"{ids(shape)} offsets {offs} init: {k}"
    wh, ww = R.square_window(p, height, width)
    for it in range(iters):
        z = _logits(B, 4, seed + it)
        z[np.arange(B), labels] += 4.0 if it < iters - 3 else 0.0
        last = it + 1 == iters
        host_step(host, z, labels, x0, height, width, wh, ww, R.p_q(p), restart, it, seed, eps, last=last, n_valid=nv, clip0=clip0,
                  clip_lo=lo, clip_hi=hi)
        square_step(dev(z), lab, xt, height, width, wh, ww, R.p_q(p), restart, it, seed, eps, loss_best=loss, done=done, last=last, **kw)
        got = state()
        for k in got:
            assert same(got[k], host[k]), f"{ids(shape)} offsets {offs} step {it}: {k}"
        inside = np.zeros((B, height, width), dtype=bool)
        for b, (r, c, h, w) in enumerate(got["win"]):
            inside[b, r:r + h, c:c + w] = True
        differs = (got["x_best"].view(np.uint32) != got["x_cand"].view(np.uint32)).reshape(inside.shape)
        assert not (differs & ~inside).any(), "x_cand differs from x_best outside win"
        if last:
            assert not differs.any() and not got["win"].any(), "after LAST x_cand is x_best"
    assert same(xt.cpu().numpy(), x0)
    return got


# =================================================================================================
# 1. the kernels against the host twins
# =================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_kernels_equal_the_host_twins_bit_for_bit(cuda, shape):
    seed = 11 + sum(shape)
    for offs in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]:
        _device_chain(shape, seed, 0.1, 10, offs)
    _device_chain(shape, seed, 0.25, 8, (1, 0, 1), clip=(-0.2, 0.35), restart=255, clip0=3)
    if shape[1] == 1:
        n = shape[2]
        values = [0, 1, 5, n - 1, n, n + 3, -2]
        for s, offs in zip(range(0, len(values), shape[0]), itertools.cycle([(0, 0, 0), (1, 1, 1)])):
            _device_chain(shape, 5, 0.1, 8, offs, n_valid=(values[s:] + values)[:shape[0]], p=0.4)


def test_wrappers_refuse_bad_arguments(cuda):
    from lipasr.square import square_init, square_step

    x0 = dev(_rows(2, 21, 0))
    best, cand, win = torch.empty_like(x0), torch.empty_like(x0), torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    loss, done, lab = torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    kw = dict(x_best=best, x_cand=cand, win=win)
    square_init(x0, 3, 7, 0, 0, 0.1, **kw)
    z = dev(_logits(2, 3, 0))
    skw = dict(loss_best=loss, done=done, **kw)
    for bad in (lambda: square_init(x0, 3, 8, 0, 0, 0.1, **kw), lambda: square_init(x0, 3, 7, 256, 0, 0.1, **kw),
                lambda: square_init(x0, 3, 7, 0, 0, -0.1, **kw), lambda: square_init(x0, 3, 7, 0, 0, 0.1, **dict(kw, x_cand=best)),
                lambda: square_init(x0, 3, 7, 0, 0, 0.1, **dict(kw, x_best=x0)), lambda: square_init(x0, 3, 7, 0, 0, 0.1, **dict(kw, win=win[:1])),
                lambda: square_init(x0, 3, 7, 0, 0, 0.1, n_valid=lab, **kw), lambda: square_init(x0.cpu(), 3, 7, 0, 0, 0.1, **kw),
                lambda: square_step(z, lab, x0, 3, 7, 4, 1, 0, 0, 0, 0, 0.1, **skw), lambda: square_step(z, lab, x0, 3, 7, 1, 0, 0, 0, 0, 0, 0.1, **skw),
                lambda: square_step(z, lab, x0, 3, 7, 1, 1, (1 << 24) + 1, 0, 0, 0, 0.1, **skw),
                lambda: square_step(z, lab, x0, 3, 7, 1, 1, 0, 0, 1 << 24, 0, 0.1, **skw),
                lambda: square_step(z[:1], lab, x0, 3, 7, 1, 1, 0, 0, 0, 0, 0.1, **skw),
                lambda: square_step(z, lab.long(), x0, 3, 7, 1, 1, 0, 0, 0, 0, 0.1, **skw),
                lambda: square_step(z, lab, x0, 3, 7, 1, 1, 0, 0, 0, 0, 0.1, clip_values=(1.0, -1.0), **skw),
                lambda: square_step(dev(_logits(2, 33, 0)), lab, x0, 3, 7, 1, 1, 0, 0, 0, 0, 0.1, **skw)):
        with pytest.raises(ValueError):
            bad()
    empty = x0[:0]
    square_init(empty, 3, 7, 0, 0, 0.1, x_best=best[:0], x_cand=cand[:0], win=win[:0])  # nothing to do, nothing written
    torch.cuda.synchronize()


# =================================================================================================
# 2. SquareAttack against the hand-built chain, and across chunks
# =================================================================================================
SMALL = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]


@pytest.fixture(scope="module")
def small(cuda):
    from lipasr.attacks import TensorFlowV2Classifier

    m = build_model(SMALL, max_batch=64)
    load_params(m, L.setup_params(SMALL, 2))
    x = np.random.default_rng(4).standard_normal((7, 36)).astype(np.float32)
    return dict(model=m, x=x, clf=TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,)))


def _hand_chain(clf, xt, labels, shape, eps, seed, max_iter, p_init, restart=0):
    """One restart of SquareAttack spelled out: square_init, then max_iter times predict_device and square_step."""
    from lipasr.square import SquareAttack, square_init, square_p, square_p_q, square_step, square_window

    B, n = xt.shape
    best, cand = torch.empty_like(xt), torch.empty_like(xt)
    win, loss = torch.empty(B, 4, dtype=torch.int32, device="cuda"), torch.empty(B, device="cuda")
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    key = (0x5CA2E00000000000 + seed) & 0xFFFFFFFFFFFFFFFF
    assert SquareAttack(clf, eps=eps, seed=seed).seed == key
    kw = dict(x_best=best, x_cand=cand, win=win)
    square_init(xt, *shape, restart, key, eps, **kw)
    for it in range(max_iter):
        p = square_p(it + 1, max_iter, p_init)
        wh, ww = square_window(p, *shape)
        square_step(clf.predict_device(cand, logits=True), labels, xt, *shape, wh, ww, square_p_q(p), restart, it, key, eps, loss_best=loss,
                    done=done, last=it + 1 == max_iter, **kw)
    return best, loss, done


def test_generate_equals_the_hand_built_chain(small):
    from lipasr.attacks import SquareAttack, TensorFlowV2Classifier

    clf, xt = small["clf"], dev(small["x"])
    B, eps, seed, iters = 7, 0.4, 9, 25
    labels = clf.predict_device(xt, logits=True).argmax(dim=1).to(torch.int32)
    for shape in ((6, 6), None):
        atk = SquareAttack(clf, eps=eps, max_iter=iters, seed=seed, shape=shape, check_every=1000)
        adv = atk.generate_device(xt)
        best, loss, done = _hand_chain(clf, xt, labels, shape or (1, 36), eps, seed, iters, 0.8)
        assert same(adv.cpu().numpy(), best.cpu().numpy()) and adv.data_ptr() != xt.data_ptr()
        assert torch.equal(atk.success_, done != 0) and atk.success_.dtype == torch.bool
        assert torch.equal(atk.queries_, torch.where(done != 0, done, torch.full_like(done, iters)).long()) and atk.queries_.dtype == torch.int64
        assert same(atk.loss_.cpu().numpy(), loss.cpu().numpy()) and atk.loss_.dtype == torch.float32
        print(f"shape {shape}: done {done.tolist()} loss {[round(v, 3) for v in loss.tolist()]}")
        want = best.cpu().numpy()
        # a look at done every iteration stops early and returns the same rows; so do chunks of 3 and of 2 rows
        for kw in (dict(check_every=1), dict(batch_size=3), dict(batch_size=2, check_every=2)):
            other = SquareAttack(clf, eps=eps, max_iter=iters, seed=seed, shape=shape, **kw)
            assert same(other.generate_device(xt).cpu().numpy(), want), kw
            assert torch.equal(other.success_, atk.success_) and torch.equal(other.queries_, atk.queries_) and torch.equal(other.loss_, atk.loss_)
        onehot = np.eye(5, dtype=np.float32)[labels.cpu().numpy()]
        for y in (None, onehot, labels.cpu().numpy()):
            assert same(atk.generate(small["x"], y), want)
        assert not same(SquareAttack(clf, eps=eps, max_iter=iters, seed=seed + 1, shape=shape).generate(small["x"]), want)
    assert atk.success_.any() and not atk.success_.all(), "choose eps so that some rows leave their class and some do not"

    class Limited(TensorFlowV2Classifier):
        batch_limit = 4

    lim = SquareAttack(Limited(model=small["model"], nb_classes=5, input_shape=(36,)), eps=eps, max_iter=iters, seed=seed)
    assert same(lim.generate_device(xt).cpu().numpy(), want)
    # restarts: a fooled row keeps the first restart that fooled it, any other row the lowest loss
    two = SquareAttack(clf, eps=eps, max_iter=iters, seed=seed, nb_restarts=2)
    adv2 = two.generate_device(xt)
    b1, l1, d1 = _hand_chain(clf, xt, labels, (1, 36), eps, seed, iters, 0.8, restart=1)
    first = atk.success_
    take1 = ~first & ((d1 != 0) | (l1 < atk.loss_))
    assert same(adv2.cpu().numpy(), torch.where(take1[:, None], b1, adv).cpu().numpy())
    assert torch.equal(two.success_, first | (d1 != 0)) and same(two.loss_.cpu().numpy(), torch.where(take1, l1, atk.loss_).cpu().numpy())
    assert torch.equal(two.queries_, atk.queries_ + torch.where(first, 0, torch.where(d1 != 0, d1, torch.full_like(d1, iters))).long())
    # a row that is misclassified when clean comes back bit for bit, with no query spent
    wrong = (labels + 1) % 5
    given = SquareAttack(clf, eps=eps, max_iter=5, seed=seed)
    back = given.generate_device(xt[:3], torch.cat([wrong[:1], labels[1:3]]))
    assert same(back[:1].cpu().numpy(), small["x"][:1]) and bool(given.success_[0]) and int(given.queries_[0]) == 0 and float(given.loss_[0]) < 0
    for bad in (dict(norm=2), dict(max_iter=0), dict(eps=-0.1), dict(p_init=0.0), dict(p_init=1.5), dict(nb_restarts=0), dict(nb_restarts=257),
                dict(shape=(5, 7)), dict(check_every=0), dict(batch_size=0), dict(clip_values=(1.0, -1.0))):
        with pytest.raises(ValueError):
            SquareAttack(clf, **bad)
    with pytest.raises(ValueError, match="L2"):
        SquareAttack(clf, norm=2)
    with pytest.raises(ValueError):
        atk.generate_device(xt, lengths=[36] * 7)
    with pytest.raises(ValueError):
        SquareAttack(clf, targeted=True).generate_device(xt)
    assert atk.generate_device(xt[:0]).shape == (0, 36)


# =================================================================================================
# 3. small real models
# =================================================================================================
def _margin(z, labels, targeted=False):
    z = np.asarray(z, dtype=np.float32)
    return np.array([R.margin(z[b], int(labels[b]), targeted) for b in range(len(z))], dtype=np.float32)


def _check_attack(atk, predict_logits, x, adv, labels, eps, clip, valid=None):
    """The properties of the issue on one call: the ball, the clip range, the padding, success_ against a fresh prediction, loss_
    against the margin of the returned row from a fresh prediction bit for bit, queries_."""
    valid = np.ones(x.shape, dtype=bool) if valid is None else valid
    assert same(adv[~valid], x[~valid]), "padding moved"
    assert G.within_ball(np.where(valid, adv, x), x, eps)
    assert adv[valid].min() >= np.float32(clip[0]) and adv[valid].max() <= np.float32(clip[1])
    ok, q, loss = atk.success_.cpu().numpy(), atk.queries_.cpu().numpy(), atk.loss_.cpu().numpy()
    z = predict_logits(adv)
    pred = z.argmax(axis=1)
    np.testing.assert_array_equal(ok, (pred == labels) if atk.targeted else (pred != labels))
    assert same(loss, _margin(z, labels, atk.targeted)), (loss, _margin(z, labels, atk.targeted))
    assert ((loss < 0) == ok).all()
    assert (q[~ok] == atk.max_iter * atk.nb_restarts).all() and ((q[ok] >= 0) & (q[ok] <= atk.max_iter * atk.nb_restarts)).all()
    return ok, q


def test_attack_over_mfcc_pictures_of_a_real_model(cuda):
    from lipasr.attacks import SquareAttack, TensorFlowV2Classifier

    spec = P.vd_unconstrained_spec()
    m = build_model(spec)
    load_params(m, L.setup_params(spec, 3))
    clf = TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
    clip = (-2.0, 2.0)
    x = np.clip(np.random.default_rng(3).standard_normal((8, 880)), *clip).astype(np.float32)
    predict = lambda a: clf.predict_device(dev(a), logits=True).cpu().numpy()
    own = predict(x).argmax(axis=1)
    eps = 0.5
    kw = dict(eps=eps, max_iter=40, seed=1, clip_values=clip, shape=(20, 44), check_every=5)
    assert SquareAttack(clf, eps=eps).clip_values is None  # a TensorFlowV2Classifier has no clip_values
    atk = SquareAttack(clf, **kw)
    adv = atk.generate(x)
    ok, q = _check_attack(atk, predict, x, adv, own, eps, clip)
    print(f"unconstrained 880 -> 10 as 20 x 44, eps {eps}: {int(ok.sum())} of 8 rows left their class, queries {q.tolist()}")
    assert ok.any()
    # every element moved by exactly eps (or sits on the clip range): a point of the search is a sign pattern
    moved = np.abs(adv.astype(np.float64) - x)
    assert ((np.abs(moved - np.float32(eps)) <= np.spacing(np.float32(2.5))) | (np.abs(adv) == 2.0)).all()
    # queries_ counts the start as query 1: with exactly that many queries the first rows to finish finish, and no other
    first = int(q[ok].min())
    short = SquareAttack(clf, **dict(kw, max_iter=first, p_schedule=lambda it, mi, p0: atk.p_schedule(it, 40, p0)))
    adv_short = short.generate(x)
    np.testing.assert_array_equal(short.success_.cpu().numpy(), q == first)
    assert same(adv_short[q == first], adv[q == first])
    target = (own + 1) % 10
    tgt = SquareAttack(clf, targeted=True, **kw)
    adv_t = tgt.generate(x, np.eye(10, dtype=np.float32)[target])
    ok_t, _ = _check_attack(tgt, predict, x, adv_t, target, eps, clip)
    print(f"targeted: {int(ok_t.sum())} of 8 rows reached class own + 1")


RAGGED = [16000, 9000, 37]


@pytest.fixture(scope="module")
def audio(cuda):
    """Three synthetic clips of 16000, 9000 and 37 samples in rows of 16000 at 16 kHz as 22 050 Hz rows, and a WaveformClassifier
    over the unconstrained 880 -> 10 model (the fixture of tests/test_genetic_gpu.py)."""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, L.setup_params(spec, 3))
    ex = MfccExtractor(16000, 16000, batch_max=32)
    w = np.asarray(synth_clips(3, seed=31)[0], dtype=np.float32)
    for r, n in enumerate(RAGGED):
        w[r, n:] = 0
    lt = torch.as_tensor(np.array(RAGGED, dtype=np.int32)).to(cuda)
    rows = ex.resample(torch.as_tensor(w).to(cuda).contiguous(), n_valid=lt)
    yield dict(lt=lt, rows=rows, clf=WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k"))
    ex.close()


def test_attack_over_audio_with_lengths(audio):
    from lipasr.attacks import SquareAttack

    clf, rows, lt = audio["clf"], audio["rows"], audio["lt"]
    x = rows.cpu().numpy()
    assert x.shape == (3, 22050)
    pos = [int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED]
    valid = np.arange(22050)[None, :] < np.array(pos)[:, None]
    predict = lambda a: clf.predict_device(torch.as_tensor(a).cuda(), logits=True, lengths=lt).cpu().numpy()
    own = predict(x).argmax(axis=1)
    eps = 0.05
    atk = SquareAttack(clf, eps=eps, max_iter=16, seed=2, check_every=4)
    assert atk.clip_values == (-1.0, 1.0)  # the estimator's
    adv = atk.generate_device(rows, lengths=lt).cpu().numpy()
    ok, q = _check_attack(atk, predict, x, adv, own, eps, (-1.0, 1.0), valid)
    print(f"audio 3 x 22050 with lengths, eps {eps}: success {ok.tolist()} queries {q.tolist()}")
    assert (adv != x)[valid].mean() > 0.99  # every sample of a clip carries +-eps
    tight = SquareAttack(clf, eps=eps, max_iter=3, seed=2, clip_values=(-0.05, 0.05))
    adv = tight.generate_device(rows, lengths=lt).cpu().numpy()
    assert adv[valid].min() >= np.float32(-0.05) and adv[valid].max() <= np.float32(0.05) and same(adv[~valid], x[~valid])
    with pytest.raises(ValueError, match="strip"):
        SquareAttack(clf, eps=eps, shape=(2, 11025)).generate_device(rows, lengths=lt)
    # no lengths: the whole row is the clip, as a strip or as any picture that multiplies to it
    for shape in (None, (2, 11025)):
        free = SquareAttack(clf, eps=eps, max_iter=3, seed=2, shape=shape)
        adv = free.generate_device(rows).cpu().numpy()
        assert G.within_ball(adv, x, eps) and (adv != x)[~valid].any()


# =================================================================================================
# 4. the menu
# =================================================================================================
def test_menu_runs_the_square_sweep_and_the_ensemble(cuda, tmp_path, capsys):
    import wave

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
    load_params(m, L.setup_params(spec, 3))
    h5 = str(tmp_path / "model.h5")
    m.save(h5)
    common = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--points", "1"]
    base = common + ["--attack", "black", "--kind", "square", "--max-iter", "6"]
    capsys.readouterr()
    grid, acc, queries = V.main(base)
    out = capsys.readouterr().out
    assert len(grid) == 1 and np.isclose(grid[0], 0.01) and set(acc) == set(queries) == {"constrained", "unconstrained"}
    assert all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
    assert "Accuracy on square black-box test examples" in out and "mean queries of those" in out
    grid, acc, queries = V.main(base + ["--over", "audio"])
    out = capsys.readouterr().out
    assert grid == V.GENETIC_AUDIO_EPS[:1] and all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
    assert "Accuracy on square black-box audio test examples unconstrained" in out
    for norm in ("inf", "2"):
        grid, acc = V.main(common + ["--attack", "white", "--kind", "auto", "--norm", norm])
        assert len(grid) == 1 and grid[0] == 1.0 and all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
    with pytest.raises(ValueError):
        V.square_sweep({"constrained": m}, feats[:4], feats[4:8], feats[8:], np.eye(10)[lab[8:12]], over="audio")
