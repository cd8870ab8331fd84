"""The input-transformation defences on the MI355X: lipasr_defence_apply / lipasr_defence_vjp against their host twins bit for bit
(the twins equal the NumPy restatement of tests/defence_ref.py bit for bit, test_defence_cpu.py), the fused chain against its
stages launched one after the other, DefendedClassifier against the plain WaveformClassifier and the hand-composed chain, the
attacks over it, and the detector.

There are no tolerances here: no element's arithmetic depends on the tiling, the batch or the alignment, so every comparison is of
bits.  Outputs are pre-filled with NaN, so that "exactly 0 beyond the clip" is seen; buffers (and taps) sit at element offsets 0
and 1 of their allocations.  The cases are defence_ref.CASES: n on either side of the 1 024-position tile, 1, 3 and 33 clips, each
stage alone, chains of 2, 3 and 4, one of them at the halo cap of 256."""
import functools
import math

import numpy as np
import pytest
import torch

import defence_ref as DR
import local_lip_ref as L
from defence_ref import CASES, ids
from helpers import build_model, load_params
from oracle import mlp_ref as P

import lipasr._native as N

pytestmark = pytest.mark.gpu


def _place(x, offset=0, fill=0.0):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation."""
    x = np.asarray(x)
    buf = torch.full((x.size + offset,), fill, device="cuda", dtype=torch.as_tensor(x[:0]).dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bits(a, b):
    """torch.equal on the bits: a -0 is not a +0."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _i32(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs, lengths and the host twins' results for a case, computed once and left unchanged."""
    name, clips, n = case
    stages = DR.stages_of(name)
    nat = DR.native(stages)
    runs = []
    for levels in (False, True):
        x, g = DR.inputs(clips, n, levels=levels)
        for nv in (None, DR.mixed_lengths(clips, n)):
            runs.append(dict(x=x, g=g, nv=nv, out=N.defence_apply_host(x, nat, n_valid=nv), gx=N.defence_vjp_host(x, g, nat, n_valid=nv)))
    return dict(stages=stages, runs=runs)


def _defence(stages, off=0):
    from lipasr.defences import AudioDefence

    d = AudioDefence([(k, _place(a, off) if k == "fir" else a) for k, a in stages])
    for t in d._taps:
        assert t is None or t.data_ptr() % 8 == (4 if off else 0)
    return d


def _run(d, x, g, nv, off=0, clip=None):
    """apply and vjp on the device (for the one clip ``clip``, launched alone) -> NumPy (out, gx)."""
    if clip is not None:
        x, g, nv = x[clip:clip + 1], g[clip:clip + 1], None if nv is None else nv[clip:clip + 1]
    nvt = _i32(nv)
    poison = np.full(x.shape, np.nan, dtype=np.float32)
    out, gx = _place(poison, off, fill=np.nan), _place(poison, 1 - off, fill=np.nan)
    xt = _place(x, off)
    assert d.apply(xt, nvt, out=out) is out
    assert d.vjp(xt, _place(g, 1 - off), nvt, out=gx) is gx
    return out.cpu().numpy(), gx.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_kernels_equal_their_twins(cuda, case):
    """Bit for bit, apply and vjp; exact zeros beyond the clip over the NaN the outputs held; the same bits on a second run at the
    other buffer offsets."""
    name, clips, n = case
    ref = reference(case)
    for i, r in enumerate(ref["runs"]):
        d = _defence(ref["stages"], i % 2)
        out, gx = _run(d, r["x"], r["g"], r["nv"], i % 2)
        assert same(out, r["out"]), (case, i, "apply", int((out.view(np.uint32) != r["out"].view(np.uint32)).sum()))
        assert same(gx, r["gx"]), (case, i, "vjp", int((gx.view(np.uint32) != r["gx"].view(np.uint32)).sum()))
        beyond = np.arange(n)[None, :] >= DR.clamp_lengths(r["nv"], clips, n)[:, None]
        assert same(out[beyond], np.zeros(int(beyond.sum()), dtype=np.float32)) and same(gx[beyond], np.zeros(int(beyond.sum()), dtype=np.float32))
        again = _run(_defence(ref["stages"], 1 - i % 2), r["x"], r["g"], r["nv"], 1 - i % 2)
        assert same(again[0], out) and same(again[1], gx), (case, i, "two runs, two alignments")


@pytest.mark.parametrize("case", [c for c in CASES if len(DR.CHAINS[c[0]]) > 1], ids=ids)
def test_fused_equals_composed(cuda, case):
    """The chain in one launch against its stages launched one after the other, in both directions: the halo test."""
    ref = reference(case)
    stages = ref["stages"]
    singles = [_defence([st]) for st in stages]
    fused = _defence(stages)
    for r in ref["runs"]:
        x, g, nvt = _place(r["x"]), _place(r["g"]), _i32(r["nv"])
        us = [x]
        for s in singles:
            us.append(s.apply(us[-1], nvt))
        assert bits(fused.apply(x, nvt), us[-1]) and same(us[-1].cpu().numpy(), r["out"])
        gg = g
        for s, u in zip(singles[::-1], us[-2::-1]):
            gg = s.vjp(u, gg, nvt)
        assert bits(fused.vjp(x, g, nvt), gg) and same(gg.cpu().numpy(), r["gx"])


@pytest.mark.parametrize("case", [c for c in CASES if c[1] > 1 and c[2] > 5], ids=ids)
def test_a_clip_has_the_bits_of_its_own_launch(cuda, case):
    name, clips, n = case
    ref = reference(case)
    d = _defence(ref["stages"])
    for r in ref["runs"][1::2]:  # the ragged runs: every kind of length is among the clips
        out, gx = _run(d, r["x"], r["g"], r["nv"])
        for b in sorted({0, 1, 2, 3, 4, 5, clips - 1} & set(range(clips))):
            alone = _run(d, r["x"], r["g"], r["nv"], clip=b)
            assert same(alone[0], out[b:b + 1]) and same(alone[1], gx[b:b + 1]), (case, b)


@pytest.mark.parametrize("name", ["median5", "cap-median15-fir255-fir245-quantize4"])
def test_one_launch_per_direction(cuda, name):
    d = _defence(DR.stages_of(name))
    x, g = (_place(a) for a in DR.inputs(3, 2 * DR.TILE + 3))
    count = lambda: [N.lib.lipasr_debug_defence_launches(k) for k in (0, 1)]
    c0 = count()
    d.apply(x)
    c1 = count()
    d.vjp(x, g)
    c2 = count()
    d.vjp(x, g, backward="identity")
    d.apply(x[:0])  # nothing to do: no launch
    c3 = count()
    assert c1 == [c0[0] + 1, c0[1]] and c2 == [c0[0] + 1, c0[1] + 1] and c3 == c2


def test_defence_checks_its_tensors(cuda):
    from lipasr.defences import AudioDefence

    d = AudioDefence([("median", 5), ("lowpass", np.ones(9, dtype=np.float32) / 9), ("quantize", 8)])
    assert d.halo == 6 and d.stages == [(N.DEFENCE_MEDIAN, 5), (N.DEFENCE_FIR, 9), (N.DEFENCE_QUANTIZE, 8)]
    x = torch.zeros(4, 10, device="cuda")
    assert d.apply(x).shape == (4, 10) and d.vjp(x, x.clone()).shape == (4, 10)
    for bad in (x.double(), x.cpu(), x[:, ::2], x[0]):
        with pytest.raises(ValueError):
            d.apply(bad)
        with pytest.raises(ValueError):
            d.vjp(x, bad)
    with pytest.raises(ValueError):
        d.apply(x, n_valid=torch.zeros(4, device="cuda"))  # not int32
    with pytest.raises(ValueError):
        d.apply(x, out=torch.zeros(4, 11, device="cuda"))
    with pytest.raises(ValueError):
        d.vjp(x, torch.zeros(3, 10, device="cuda"))
    with pytest.raises(ValueError):
        d.vjp(x, x.clone(), backward="bpda")
    big = torch.zeros(70, device="cuda")
    with pytest.raises(ValueError):
        d.apply(big[:40].view(4, 10), out=big[30:].view(4, 10))  # out overlaps x: refused by the library
    for bad in ([], [("median", 4)], [("quantize", 1)], [("fir", np.ones(4))], [("fir", np.ones(255))] * 3):
        with pytest.raises(ValueError):
            AudioDefence(bad)
    # the identity backward: g masked to the clip, whatever the chain
    g = torch.as_tensor(np.random.default_rng(0).standard_normal((4, 10)).astype(np.float32)).cuda()
    nv = _i32([10, 3, 0, 15])
    want = torch.where(torch.arange(10, device="cuda")[None, :] < torch.tensor([10, 3, 0, 10], device="cuda")[:, None], g, torch.zeros_like(g))
    out = torch.full((4, 10), float("nan"), device="cuda")
    assert bits(d.vjp(x, g, nv, backward="identity"), want) and d.vjp(x, g, nv, backward="identity", out=out) is out and bits(out, want)
    assert bits(d.vjp(x, g, backward="identity"), g) and d.vjp(x, g, backward="identity") is not g


# =================================================================================================
# the estimator
# =================================================================================================
RAGGED = [16000, 9000, 37, 0]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def air(cuda):
    """The small WaveformClassifier of test_room_gpu.py, four clips at 22 050 Hz (without -0) and their labels."""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, L.setup_params(spec, 3))
    ex = MfccExtractor(16000, 16000, batch_max=32)
    w = np.asarray(synth_clips(4, seed=31)[0], dtype=np.float32)
    whole = ex.resample(torch.as_tensor(w).to(cuda).contiguous()).clone() + 0.0  # x + 0: a -0 becomes +0
    for r, n in enumerate(RAGGED):
        w[r, n:] = 0
    lt = torch.as_tensor(np.array(RAGGED, dtype=np.int32)).to(cuda)
    cut = ex.resample(torch.as_tensor(w).to(cuda).contiguous(), n_valid=lt).clone() + 0.0
    base = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
    y = torch.eye(10, device=cuda)[torch.tensor([3, 1, 4, 1], device=cuda)].contiguous()
    v = torch.as_tensor(np.random.default_rng(5).standard_normal((4, 10)).astype(np.float32)).to(cuda)
    pos = torch.tensor([int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED], device=cuda)
    yield dict(base=base, cases=[(whole, None, None), (cut, lt, torch.arange(22050, device=cuda)[None, :] < pos[:, None])], y=y, v=v)
    ex.close()


def _chain():
    from lipasr.defences import AudioDefence, lowpass_taps

    return AudioDefence([("median", 5), ("lowpass", lowpass_taps(4000, 22050, 101)), ("quantize", 8)])


def _five(est, x, lt, y, v):
    """The five calls of the estimator surface (predict twice: probabilities and logits)."""
    return dict(probs=est.predict_device(x, lengths=lt), logits=est.predict_device(x, logits=True, lengths=lt),
                own=est.own_labels_device(x, lengths=lt), grad=est.loss_gradient_device(x, y, lengths=lt),
                vjp=est.output_vjp_device(x, v, on_logits=True, lengths=lt), vjp_p=est.output_vjp_device(x, v, lengths=lt),
                jac=est.jacobian_device(x, on_logits=True, lengths=lt).contiguous())


def test_one_tap_is_the_plain_estimator(air):
    """fir [1.0] is the identity on rows without -0 (fma(1, x, 0) = x), forward and backward: the five calls give the base's
    values, compared with torch.equal (a -0 of the base's gradient comes back as +0: the one bit the identity chain may change)."""
    from lipasr.attacks import DefendedClassifier
    from lipasr.defences import AudioDefence

    base = air["base"]
    for backward in ("chain", "identity"):
        est = DefendedClassifier(base, AudioDefence([("fir", np.ones(1, dtype=np.float32))]), backward=backward)
        assert est.batch_limit == base.batch_limit and est.clip_values == base.clip_values and est.input_shape == (22050,)
        assert est.model is base.model and est.extractor is base.extractor and est.domain == base.domain
        for x, lt, _ in air["cases"]:
            nv = None if lt is None else base.clip_positions(lt).contiguous()
            assert bits(est.defence.apply(x, nv), x)
            got, want = _five(est, x, lt, air["y"], air["v"]), _five(base, x, lt, air["y"], air["v"])
            for k in want:
                assert torch.equal(got[k], want[k]), (backward, k, lt)
            assert float(want["grad"].abs().max()) > 0
            assert np.array_equal(est.predict(x.cpu().numpy(), lengths=lt), want["probs"].cpu().numpy())


def test_the_estimator_is_the_composed_chain(air):
    """With a real chain every backward call equals the hand composition defence.vjp(x, base.call(defence.apply(x), ...)) bit for
    bit, with and without lengths, and the gradient is exactly 0 beyond each clip."""
    from lipasr.attacks import DefendedClassifier

    base, d = air["base"], _chain()
    est = DefendedClassifier(base, d)
    y, v = air["y"], air["v"]
    for x, lt, mask in air["cases"]:
        nv = None if lt is None else base.clip_positions(lt).contiguous()
        keep = x.clone()
        tx = d.apply(x, nv)
        assert not bits(tx, x)
        assert bits(est.predict_device(x, lengths=lt), base.predict_device(tx, lengths=lt))
        assert bits(est.predict_device(x, logits=True, lengths=lt), base.predict_device(tx, logits=True, lengths=lt))
        assert bits(est.own_labels_device(x, lengths=lt), base.own_labels_device(tx, lengths=lt))
        got = est.loss_gradient_device(x, y, lengths=lt)
        assert bits(got, d.vjp(x, base.loss_gradient_device(tx, y, lengths=lt), nv)) and float(got.abs().max()) > 0
        out = torch.full_like(x, float("nan"))
        assert est.loss_gradient_device(x, y, out=out, lengths=lt) is out and bits(out, got)
        for on_logits in (True, False):
            assert bits(est.output_vjp_device(x, v, on_logits=on_logits, lengths=lt),
                        d.vjp(x, base.output_vjp_device(tx, v, on_logits=on_logits, lengths=lt), nv))
        jac = est.jacobian_device(x, on_logits=True, lengths=lt)
        jb = base.jacobian_device(tx, on_logits=True, lengths=lt)
        assert jac.shape == (4, 10, 22050)
        for c in range(10):
            assert bits(jac[:, c], d.vjp(x, jb[:, c].contiguous(), nv)), c
            assert bits(jac[:, c], est.output_vjp_device(x, torch.eye(10, device=x.device)[c].expand(4, 10).contiguous(), on_logits=True, lengths=lt)), c
        if mask is not None:
            assert not got[~mask].any() and not jac.permute(1, 0, 2)[:, ~mask].any(), "the gradient is exactly 0 beyond each clip"
        ident = DefendedClassifier(base, d, backward="identity").loss_gradient_device(x, y, lengths=lt)
        gb = base.loss_gradient_device(tx, y, lengths=lt)
        assert bits(ident, gb if mask is None else torch.where(mask, gb, torch.zeros_like(gb))) and not bits(ident, got)
        assert torch.equal(x, keep)


def test_a_defended_classifier_goes_behind_a_room(air):
    from lipasr.attacks import DefendedClassifier, OverTheAirClassifier
    from lipasr.room import RoomChannel, synthetic_rirs

    base, d = air["base"], _chain()
    est = DefendedClassifier(base, d)
    ch = RoomChannel(synthetic_rirs(2, taps=65))
    ota = OverTheAirClassifier(est, ch)
    assert ota.batch_limit == base.batch_limit // 2 and ota.input_shape == (22050,)
    for x, lt, mask in air["cases"]:
        nv = None if lt is None else base.clip_positions(lt).contiguous()
        l2 = None if lt is None else lt.repeat_interleave(2)
        each = ota.predict_each_device(x, lengths=lt)
        assert each.shape == (4, 2, 10) and bits(each.view(8, 10), est.predict_device(ch.apply(x, nv), lengths=l2))  # room, then defence
        assert bits(ota.predict_device(x, lengths=lt), each.mean(dim=1))
        g = ota.loss_gradient_device(x, air["y"], lengths=lt)
        assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        if mask is not None:
            assert not g[~mask].any()
    for bad in ((est, d), (ota, d), (object(), d), (base, None)):
        with pytest.raises(TypeError):
            DefendedClassifier(*bad)
    with pytest.raises(ValueError):
        DefendedClassifier(base, d, backward="bpda")


def test_attacks_run_unchanged(air):
    """ProjectedGradientDescent and SquareAttack over a DefendedClassifier with ragged lengths: the result stays inside the ball and
    clip_values, and the samples beyond each clip are the input's bits."""
    from lipasr.attacks import DefendedClassifier, ProjectedGradientDescent
    from lipasr.square import SquareAttack

    eps = 0.01
    for backward in ("chain", "identity"):
        est = DefendedClassifier(air["base"], _chain(), backward=backward)
        for make in (lambda: ProjectedGradientDescent(est, eps=eps, eps_step=eps / 2, max_iter=3),
                     lambda: SquareAttack(est, eps=eps, max_iter=4, seed=1)):
            for x, lt, mask in air["cases"]:
                keep = x.clone()
                y = est.own_labels_device(x, lengths=lt)  # the estimator's own: no clip is adversarial before the attack starts
                a = make().generate_device(x, y, lengths=lt)
                assert float((a.double() - x.double()).abs().max()) <= eps + U  # adv = fl(x + d), |d| <= eps, |x| <= 1
                assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0 and not torch.equal(a, x) and torch.equal(x, keep)
                if mask is not None:
                    assert bits(a[~mask], x[~mask]), "padding moved"
                assert bits(make().generate_device(x, y, lengths=lt), a), "two runs differ"


def test_detector_scores_and_flags(air):
    from lipasr.defences import AudioDefence, TransformationDetector

    base = air["base"]
    ident = AudioDefence([("fir", np.ones(1, dtype=np.float32))])
    d3, d2 = _chain(), AudioDefence([("quantize", 3)])
    for x, lt, _ in air["cases"]:
        nv = None if lt is None else base.clip_positions(lt).contiguous()
        assert not TransformationDetector(base, [ident]).scores(x, lengths=lt).any()  # T = identity: nothing moves
        p0 = base.predict_device(x, lengths=lt)
        each = [(base.predict_device(d.apply(x, nv), lengths=lt) - p0).abs().sum(dim=1) for d in (d3, d2)]
        det = TransformationDetector(base, [d3, d2])
        s = det.scores(x, lengths=lt)
        assert s.shape == (4,) and bits(s, torch.maximum(*each)) and float(s.max()) > 0 and float(s.max()) <= 2.0 + 4 * U
        assert det.fit(x, fpr=0.25, lengths=lt) is det and det.threshold == float(np.quantile(s.cpu().numpy().astype(np.float64), 0.75))
        flags, s2 = det.detect(x, lengths=lt)
        assert bits(s2, s) and flags.dtype == torch.bool and torch.equal(flags, s > det.threshold) and int(flags.sum()) <= 1


def test_menu_puts_the_defence_under_attack(cuda, tmp_path, capsys):
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
    common = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--points", "2",
              "--over", "audio"]
    defence = ["--defence", "median:5,lowpass:4000:101,quantize:8"]
    capsys.readouterr()
    for extra in (["--attack", "white", "--kind", "pgd"], ["--attack", "white", "--kind", "fgsm", "--defence-backward", "identity"],
                  ["--attack", "black", "--kind", "square", "--max-iter", "3", "--detect-fpr", "0.5"]):
        grid, acc = V.main(common + extra + defence)
        out = capsys.readouterr().out
        assert len(grid) == 2 and set(acc) == {"constrained", "unconstrained"}
        for name, a in acc.items():
            assert set(a) == {"undefended", "static", "adaptive", "detected"}
            assert all(len(v) == 2 and ((0.0 <= v) & (v <= 1.0)).all() for v in a.values())
            if grid[0] == 0:  # strength 0: the clean clips, so the defended model's two accuracies are one
                assert a["static"][0] == a["adaptive"][0]
        for k in ("undefended", "static", "adaptive", "detected"):
            assert np.array_equal(acc["constrained"][k], acc["unconstrained"][k])  # one model twice
        for label in ("Accuracy of the undefended model on adversarial audio", "made against the undefended one (static)",
                      "made against itself (adaptive, backward", "Detector hit rate on the static adversarial audio at false-positive rate"):
            assert out.count(label) == 4, out
    for bad in (["--attack", "black", "--kind", "hsj"], ["--attack", "black", "--kind", "simple"], ["--attack", "lipschitz"],
                ["--attack", "white", "--kind", "pgd", "--room", "2"]):
        with pytest.raises(ValueError):
            V.main(common + bad + defence)
    with pytest.raises(ValueError):
        V.main(common[:-2] + ["--attack", "white", "--kind", "fgsm"] + defence)  # over MFCC rows there is no defence
    with pytest.raises(ValueError):
        V.main(common + ["--attack", "white", "--kind", "fgsm", "--defence", "mp3:64"])
    with pytest.raises(ValueError):
        V.main(common + ["--attack", "white", "--kind", "fgsm", "--detect-fpr", "0.1"])  # goes with --defence
    # without the flag the sweep is the one it was
    grid, acc = V.main(common + ["--attack", "white", "--kind", "fgsm"])
    assert len(grid) == 2 and all(isinstance(v, np.ndarray) for v in acc.values())
    out = capsys.readouterr().out
    assert "defended" not in out and out.count("Accuracy on adversarial audio test examples") == 4
