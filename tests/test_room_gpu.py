"""The over-the-air channel on the MI355X: lipasr_room_apply / lipasr_room_vjp against the float64 restatement of tests/room_ref.py,
and OverTheAirClassifier against the plain WaveformClassifier and against the hand-composed chain.

Kernel bounds.  The device sums an output's taps in another order than the float32 restatement (by position upwards, two taps per
MFMA), so the comparison is with the float64 restatement, bound 8 x the worst error of the float32 restatement against that same
float64 one, the worst taken over the cases of the shape, no floor (the form of test_psycho_gpu.py and test_hsj_gpu.py).  On the CPU,
reversing the tap order or splitting the chain into four interleaved accumulators moved the worst error by factors 0.4 - 1.9 at
33 to 2 048 taps: the factor 8 covers the order of summation and nothing else.  Taps are N(0, 1) and not decaying, so that the loss
of any tap shows; x, g ~ U(-1, 1); outputs are pre-filled with 7.0; buffers sit at element offsets 0 and 1 of their allocations.

The shapes are room_ref.SHAPES: the issue's ten, then one shape on each side of every edge of the one kernel instance there is.

Measured (MI355X): device error / float32 restatement's error per shape 0.73 ... 1.26 for apply (the worst at 32 x 16 x 127 x 1000) and
1.00 for vjp at every shape, whose chain runs in the restatement's (j, k) order.

Estimator bounds.  With the bank [[1.0]] the channel is the identity bit for bit (fma(x, 1, 0) = x), so the five calls give the plain
estimator's values.  With three copies of it every answer is a mean, or for the loss gradient a sum, of three terms, term_j being
what the base answers for room j's row of the expanded batch: the copies' terms are equal up to the base's last bits, so the
first partial sum 2 t is exact and the sum of three has one rounding (2^-24); the scale 1/3 adds its own (2^-25) and the product's
(2^-24): 2.5 * 2^-24 sum_j |term_j| to first order, inside the 3 * 2^-24 sum_j |term_j| asked for (three unequal terms could reach
3.5: the bound is one for copies) -- measured 0.33 (loss gradient) to 0.67 (the vjp's) of that bound.  The terms are taken from the base AT THE TRIPLED ROWS, not from its
answer at the clip alone: the base's own arithmetic depends on the batch it is given (the loss gradient's 1 / rows, the extraction's
tiles), measured up to 1.2e-4 between the two on gradients of size 1e+1, which is the base's business and not the channel's."""
import functools
import math

import numpy as np
import pytest
import torch

import local_lip_ref as L
import room_ref as RR
from helpers import build_model, load_params
from oracle import mlp_ref as P
from room_ref import SHAPES, ids

pytestmark = pytest.mark.gpu

THIRD = 1.0 / 3.0


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


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Inputs, cases and the restatement's results for a shape, computed once and left unchanged."""
    clips, r, taps, n = shape
    x, g, h = RR.inputs(shape)
    cases = []
    for nv in [None] + RR.ragged_lengths(clips, n):
        a64, v64 = RR.apply(x, h, nv), RR.vjp(g, h, nv)
        a32, v32 = RR.apply(x, h, nv, dtype=np.float32), RR.vjp(g, h, nv, dtype=np.float32)
        # the scaled vjp: the same sums times float32(scale), one more rounding in float32
        v64s, v32s = float(np.float32(THIRD)) * v64, np.float32(THIRD) * v32
        cases.append(dict(nv=nv, a64=a64, v64=v64, v64s=v64s, ea=float(np.abs(a32 - a64).max()),
                          ev=max(float(np.abs(v32 - v64).max()), float(np.abs(v32s - v64s).max()))))
    return dict(x=x, g=g, h=h, cases=cases, yard_a=max(c["ea"] for c in cases), yard_v=max(c["ev"] for c in cases))


def _i32(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


def _run(ref, nv, offs=(0, 0, 0), scale=1.0, clip=None):
    """apply and vjp on the device for one case (or for the one clip ``clip`` of it, launched alone) -> NumPy (out, gx)."""
    from lipasr.room import RoomChannel

    x, g, h = ref["x"], ref["g"], ref["h"]
    r = h.shape[0]
    if clip is not None:
        x, g, nv = x[clip:clip + 1], g[clip * r:(clip + 1) * r], None if nv is None else nv[clip:clip + 1]
    ch = RoomChannel(_place(h, offs[2]))
    assert ch.rirs.data_ptr() % 8 == (4 if offs[2] else 0)
    nvt = _i32(nv)
    out = _place(np.full((x.shape[0] * r, x.shape[1]), 7.0, dtype=np.float32), offs[1], fill=7.0)
    gx = _place(np.full(x.shape, 7.0, dtype=np.float32), offs[0], fill=7.0)
    assert ch.apply(_place(x, offs[0]), nvt, out=out) is out
    assert ch.vjp(_place(g, offs[1]), nvt, scale=scale, out=gx) is gx
    return out.cpu().numpy(), gx.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_apply_and_vjp_against_float64(cuda, shape):
    """Accuracy (bound 8 x the float32 restatement's own error), exact zeros from nv on, and equal bits on a second run at the
    other buffer offsets."""
    clips, r, taps, n = shape
    ref = reference(shape)
    worst_a = worst_v = 0.0
    for i, c in enumerate(ref["cases"]):
        nvc = RR.clamp_lengths(c["nv"], clips, n)
        beyond = np.arange(n)[None, :] >= nvc[:, None]
        offs = [(0, 0, 0), (1, 0, 1), (0, 1, 0)][i % 3]
        out, gx = _run(ref, c["nv"], offs)
        _, gxs = _run(ref, c["nv"], offs, scale=THIRD)
        for got, want, yard, what in ((out, c["a64"], ref["yard_a"], "apply"), (gx, c["v64"], ref["yard_v"], "vjp"),
                                      (gxs, c["v64s"], ref["yard_v"], "vjp / 3")):
            err = float(np.abs(got - want).max())
            if what == "apply":
                worst_a = max(worst_a, err)
            else:
                worst_v = max(worst_v, err)
            assert err <= 8 * yard, (shape, c["nv"], what, err, yard)
        assert not out.reshape(clips, r, n)[np.broadcast_to(beyond[:, None], (clips, r, n))].any(), "apply: not 0 beyond the clip"
        assert not gx[beyond].any() and not gxs[beyond].any(), "vjp: not 0 beyond the clip"
        again = _run(ref, c["nv"], tuple(1 - o for o in offs))
        assert same(again[0], out) and same(again[1], gx), (shape, c["nv"], "two runs, two alignments")
    ra = worst_a / ref["yard_a"] if ref["yard_a"] else 0.0
    rv = worst_v / ref["yard_v"] if ref["yard_v"] else 0.0
    print(f"{ids(shape)}: apply device {worst_a:.3e} float32 restatement {ref['yard_a']:.3e} ratio {ra:.2f}; "
          f"vjp device {worst_v:.3e} float32 restatement {ref['yard_v']:.3e} ratio {rv:.2f} (bound: ratio 8)")


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_a_clip_has_the_bits_of_its_own_launch(cuda, shape):
    clips, r, taps, n = shape
    ref = reference(shape)
    some = sorted({b for b in (0, 1, 2, 30, 31, 32, clips - 1) if b < clips})
    for c in ref["cases"]:
        out, gx = _run(ref, c["nv"], scale=THIRD)
        for b in some:
            alone = _run(ref, c["nv"], scale=THIRD, clip=b)
            assert same(alone[0], out[b * r:(b + 1) * r]) and same(alone[1], gx[b:b + 1]), (shape, c["nv"], b)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_device_adjointness(cuda, shape):
    """<apply x, g> = <x, vjp g> up to the two accuracy bounds: |<A x - A64 x, g>| <= ea sum|g| and |<x, V g - V64 g>| <= ev sum|x|
    (the float64 restatement is adjoint to 1e-12, test_room_cpu.py)."""
    ref = reference(shape)
    x, g = ref["x"].astype(np.float64), ref["g"].astype(np.float64)
    for c in ref["cases"]:
        out, gx = _run(ref, c["nv"])
        lhs, rhs = float(np.sum(out.astype(np.float64) * g)), float(np.sum(x * gx.astype(np.float64)))
        bound = 8 * ref["yard_a"] * np.abs(g).sum() + 8 * ref["yard_v"] * np.abs(x).sum()
        assert abs(lhs - rhs) <= bound, (shape, c["nv"], lhs, rhs, bound)


def test_channel_checks_its_tensors(cuda):
    from lipasr.room import RoomChannel

    ch = RoomChannel(np.ones((2, 3), dtype=np.float32))
    x = torch.zeros(4, 10, device="cuda")
    assert ch.subset([1]).count == 1 and ch.subset(slice(0, 2)).count == 2 and ch.apply(x).shape == (8, 10)
    for bad in (x.double(), x.cpu(), x[:, ::2], x[0]):
        with pytest.raises(ValueError):
            ch.apply(bad)
    with pytest.raises(ValueError):
        ch.vjp(torch.zeros(3, 10, device="cuda"))  # not a multiple of R rows
    with pytest.raises(ValueError):
        ch.apply(x, n_valid=torch.zeros(4, device="cuda"))  # not int32
    with pytest.raises(ValueError):
        ch.apply(x, out=torch.zeros(4, 10, device="cuda"))
    big = torch.zeros(45, device="cuda")
    with pytest.raises(ValueError):
        ch.apply(big[:20].view(4, 5), out=big[5:].view(8, 5))  # out overlaps x: refused by the library
    with pytest.raises(ValueError):
        RoomChannel(np.ones((1, 8193), dtype=np.float32))


# =================================================================================================
# the estimator
# =================================================================================================
RAGGED = [16000, 9000, 37, 0]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def air(cuda):
    """The small WaveformClassifier of test_hsj_gpu.py, four clips at 22 050 Hz and their labels."""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, L.setup_params(spec, 3))
    ex = MfccExtractor(16000, 16000, batch_max=32)
    w = np.asarray(synth_clips(4, seed=31)[0], dtype=np.float32)
    whole = ex.resample(torch.as_tensor(w).to(cuda).contiguous()).clone()
    for r, n in enumerate(RAGGED):
        w[r, n:] = 0
    lt = torch.as_tensor(np.array(RAGGED, dtype=np.int32)).to(cuda)
    cut = ex.resample(torch.as_tensor(w).to(cuda).contiguous(), n_valid=lt).clone()
    base = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
    y = torch.eye(10, device=cuda)[torch.tensor([3, 1, 4, 1], device=cuda)].contiguous()
    v = torch.as_tensor(np.random.default_rng(5).standard_normal((4, 10)).astype(np.float32)).to(cuda)
    pos = torch.tensor([int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED], device=cuda)
    yield dict(base=base, cases=[(whole, None, None), (cut, lt, torch.arange(22050, device=cuda)[None, :] < pos[:, None])], y=y, v=v)
    ex.close()


def _ota(air, rirs):
    from lipasr.attacks import OverTheAirClassifier
    from lipasr.room import RoomChannel

    return OverTheAirClassifier(air["base"], RoomChannel(rirs))


def _five(est, x, lt, y, v):
    """The five calls of the estimator surface (predict twice: probabilities and logits)."""
    return dict(probs=est.predict_device(x, lengths=lt), logits=est.predict_device(x, logits=True, lengths=lt),
                own=est.own_labels_device(x, lengths=lt), grad=est.loss_gradient_device(x, y, lengths=lt),
                vjp=est.output_vjp_device(x, v, on_logits=True, lengths=lt), vjp_p=est.output_vjp_device(x, v, lengths=lt),
                jac=est.jacobian_device(x, on_logits=True, lengths=lt).contiguous())


def test_one_tap_is_the_plain_estimator(air):
    est = _ota(air, np.ones((1, 1), dtype=np.float32))
    assert est.batch_limit == air["base"].batch_limit and est.clip_values == air["base"].clip_values and est.input_shape == (22050,)
    for x, lt, _ in air["cases"]:
        got, want = _five(est, x, lt, air["y"], air["v"]), _five(air["base"], x, lt, air["y"], air["v"])
        for k in want:
            assert torch.equal(got[k], want[k]), (k, lt)
        assert float(want["grad"].abs().max()) > 0
        assert torch.equal(est.predict_each_device(x, lengths=lt)[:, 0], want["probs"])


def test_three_copies_agree_with_their_terms(air):
    """Three rooms [1.0]: every answer is the mean (or, for the loss gradient, the sum) of the base's answers at the tripled rows;
    bound 3 * 2^-24 * sum_j |term_j| per element, the terms taken in float64."""
    base = air["base"]
    est = _ota(air, np.ones((3, 1), dtype=np.float32))
    assert est.batch_limit == base.batch_limit // 3
    for x, lt, _ in air["cases"]:
        x3, l3 = x.repeat_interleave(3, dim=0), None if lt is None else lt.repeat_interleave(3)
        y3, v3 = air["y"].repeat_interleave(3, dim=0), air["v"].repeat_interleave(3, dim=0)
        got, terms = _five(est, x, lt, air["y"], air["v"]), _five(base, x3, l3, y3, v3)
        plain = _five(base, x, lt, air["y"], air["v"])
        assert torch.equal(got["own"], plain["own"])  # the dry clip's labels
        for k in ("probs", "logits", "grad", "vjp", "vjp_p", "jac"):
            t = terms[k].double().view(4, 3, *terms[k].shape[1:]) * (1.0 if k == "grad" else 1.0 / 3.0)
            err, bound = (got[k].double() - t.sum(dim=1)).abs(), 3 * U * t.abs().sum(dim=1)
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"three copies, lengths {'given' if lt is not None else 'none'}: {k} worst error / bound {worst:.3f}; "
                  f"against the plain estimator max|d| {float((got[k] - plain[k]).abs().max()):.3e}")
            assert bool((err <= bound).all()), (k, worst)


def test_loss_gradient_is_the_composed_chain(air):
    """The estimator's gradient against the chain made by hand from the same three calls, bound 3 * 2^-24 * sum_j |term_j| with
    term_j the adjoint of room j alone (the one launch over the three rooms continues one fma chain through them, so it is NOT
    compared with the sum of the three launches, whose roundings fall elsewhere)."""
    from lipasr.room import synthetic_rirs

    base = air["base"]
    est = _ota(air, synthetic_rirs(3, taps=257))
    ch = est.channel
    for x, lt, mask in air["cases"]:
        nv = None if lt is None else base.clip_positions(lt).contiguous()
        l3 = None if lt is None else lt.repeat_interleave(3)
        rows = ch.apply(x, nv)
        g3 = base.loss_gradient_device(rows, air["y"].repeat_interleave(3, dim=0), lengths=l3)
        got = est.loss_gradient_device(x, air["y"], lengths=lt)
        terms = torch.stack([ch.subset([j]).vjp(g3[j::3].contiguous(), nv) for j in range(3)]).double()
        err, bound = (got.double() - ch.vjp(g3, nv).double()).abs(), 3 * U * terms.abs().sum(dim=0)
        assert bool((err <= bound).all()) and float(got.abs().max()) > 0
        if mask is not None:
            assert not got[~mask].any(), "the gradient is exactly 0 beyond each clip"
        each = est.predict_each_device(x, lengths=lt)
        assert each.shape == (4, 3, 10)
        assert torch.equal(est.predict_device(x, lengths=lt), each.mean(dim=1))  # the float32 mean over the rooms, as torch takes it
        assert torch.equal(est.predict_device(x, lengths=lt, logits=True), est.predict_each_device(x, lengths=lt, logits=True).mean(dim=1))
        assert torch.equal(each.view(12, 10), base.predict_device(rows, lengths=l3))


def test_attacks_run_through_the_channel(air):
    from lipasr.attacks import AutoProjectedGradientDescent, FastGradientMethod, ProjectedGradientDescent
    from lipasr.room import synthetic_rirs

    est = _ota(air, synthetic_rirs(3, taps=257))
    eps = 0.01
    for x, lt, mask in air["cases"]:
        keep = x.clone()
        g = est.loss_gradient_device(x, air["y"], lengths=lt)
        want = (x + eps * torch.sign(g)).clamp(-1.0, 1.0)
        want = want if mask is None else torch.where(mask, want, x)
        adv = FastGradientMethod(est, eps).generate_device(x, air["y"], lengths=lt)
        assert torch.equal(adv, want) and torch.equal(x, keep) and not torch.equal(adv, x)
        for make in (lambda: ProjectedGradientDescent(est, eps=eps, eps_step=eps / 2, max_iter=3),
                     lambda: AutoProjectedGradientDescent(est, eps=eps, max_iter=3, nb_random_init=1)):
            a = make().generate_device(x, air["y"], lengths=lt)
            assert float((a.double() - x.double()).abs().max()) <= eps + U  # adv = fl(x + d), |d| <= eps, |x| <= 1
            assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0 and not torch.equal(a, x)
            if mask is not None:
                assert torch.equal(a[~mask], x[~mask]), "padding moved"
            assert torch.equal(make().generate_device(x, air["y"], lengths=lt), a), "two runs differ"


def test_estimator_refusals_and_the_short_window(air):
    from lipasr.attacks import OverTheAirClassifier, WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.room import RoomChannel

    base = air["base"]
    with pytest.raises(ValueError):
        _ota(air, np.ones((base.batch_limit + 1, 2), dtype=np.float32))
    with pytest.raises(TypeError):
        OverTheAirClassifier(_ota(air, np.ones((1, 1), dtype=np.float32)), RoomChannel(np.ones((1, 1), dtype=np.float32)))
    with pytest.raises(TypeError):
        OverTheAirClassifier(base, np.ones((1, 1), dtype=np.float32))
    spec = P.sr_constrained_spec()  # 2 020 features (20 x 101 frames of the short window), 20 speakers
    m = build_model(spec, max_batch=16)
    load_params(m, L.setup_params(spec, 4))
    ex = MfccExtractor(22050, 22050, batch_max=8, n_fft=441, hop=220)
    try:
        short = WaveformClassifier(m, 20, extractor=ex, utterance_length=101, domain="22k")
        est = OverTheAirClassifier(short, RoomChannel(np.array([[1.0, 0.5], [1.0, -0.25]], dtype=np.float32)))
        assert est.batch_limit == 4
        x = torch.as_tensor(np.random.default_rng(2).uniform(-0.5, 0.5, (5, 22050)).astype(np.float32)).cuda()
        y = torch.eye(20, device="cuda")[torch.arange(5, device="cuda")].contiguous()
        g = est.loss_gradient_device(x, y)
        assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert est.predict_device(x).shape == (5, 20) and est.predict_each_device(x).shape == (5, 2, 20)
        with pytest.raises(ValueError):
            est.predict_device(x, lengths=[22050, 100, 5, 1, 0])
    finally:
        ex.close()


def test_menu_plays_the_attack_in_a_room(cuda, tmp_path, capsys):
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
    room = ["--room", "2", "--room-taps", "64", "--room-t60", "0.05", "0.1", "--room-seed", "3"]
    capsys.readouterr()
    for extra in (["--attack", "white", "--kind", "fgsm"], ["--attack", "white", "--kind", "pgd", "--norm", "2"],
                  ["--attack", "black", "--kind", "square", "--max-iter", "3"]):
        grid, acc = V.main(common + extra + room)
        out = capsys.readouterr().out
        assert len(grid) == 2 and set(acc) == {"constrained", "unconstrained"}
        for name, a in acc.items():
            assert set(a) == {"clean", "dry", "air"} and all(len(v) == 2 and ((0.0 <= v) & (v <= 1.0)).all() for v in a.values())
            assert a["clean"][0] == a["clean"][1]  # the clean clips do not depend on the grid point
            if grid[0] == 0:
                assert a["dry"][0] == a["air"][0] == a["clean"][0]
        assert np.array_equal(acc["constrained"]["air"], acc["unconstrained"]["air"])  # one model twice
        for label in ("clean audio", "adversarial audio made without the room", "adversarial audio made through the attack rooms"):
            assert out.count(f"Accuracy through 2 held-out rooms on {label}") == 4, out
    for bad in (["--attack", "black", "--kind", "hsj"], ["--attack", "black", "--kind", "simple"], ["--attack", "lipschitz"]):
        with pytest.raises(ValueError):
            V.main(common + bad + room)
    with pytest.raises(ValueError):
        V.main(common[:-2] + ["--attack", "white", "--kind", "fgsm"] + room)  # over MFCC rows there is no room
    # without the flag the sweep is the one it was
    grid, acc = V.main(common + ["--attack", "white", "--kind", "fgsm"])
    assert len(grid) == 2 and all(isinstance(v, np.ndarray) for v in acc.values())
    assert "held-out rooms" not in capsys.readouterr().out
