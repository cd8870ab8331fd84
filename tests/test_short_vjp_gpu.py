"""The native backward pass of the short-window MFCC stage (lipasr_mfcc_plan_vjp_short: the Speaker-recognition features, n_fft =
win_length = 441, hop 220) against the float64 autograd oracle of tests/mfcc_grad_ref.py (n_fft=, hop=), its determinism and edge cases,
and the audio-domain attacks of lipasr.speaker_recognition built on it.

Parity bounds are 8 x the error of the SAME oracle graph evaluated in float32 (computed here, on the CPU), and at most 0.2 % of a
clip's samples may differ in sign from float64: the factor and the cap of tests/test_wave_attacks_gpu.py."""
import wave

import numpy as np
import pytest
import torch

import mfcc_grad_ref as H
from helpers import build_model, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

# batch per shape: 510/510 has 5 rows per clip, 15 clips span three clips per workgroup and leave a partial last workgroup
BATCH = {(441, 220, 22050): 6, (400, 160, 4000): 6, (510, 510, 2040): 15, (64, 32, 1000): 6, (32, 7, 300): 6}


def _lengths(shape):
    T = 1 + shape[2] // shape[1]
    return (101, 98) if shape == (441, 220, 22050) else (T, T - 3, T + 2)


def _short(n_samp, n_fft, hop, batch_max, sr=22050):
    from lipasr.extract_features_construct_dataset import MfccExtractor

    return MfccExtractor(sr, n_samp, batch_max=batch_max, n_fft=n_fft, hop=hop)


def _parity_rows(got, sig, gf, scale, vjp_kw):
    """Per row: (row, device errors, float32-oracle errors against float64 (inf, two), sign mismatches of both, samples whose float64
    gradient is exactly 0, whether the device gives exactly 0 at every one of them)."""
    rows = []
    for i in range(sig.shape[0]):
        row = H.parity_row(got[i], sig[i], gf[i], scale=scale, **vjp_kw)
        g64 = row[4]
        rows.append((i,) + row[:4] + (int((g64 == 0).sum()), bool(np.all(got[i][g64 == 0] == 0))))
    return rows


def _report_and_check(name, rows):
    yard_inf, yard_2 = max(r[1][2][0] for r in rows), max(r[1][2][1] for r in rows)
    for tag, (i, (e_inf, e_2), (y_inf, y_2), sb, sb32, z64, zdev) in rows:
        print(f"{name} {tag} row {i}: device inf {e_inf:.3e} two {e_2:.3e} | float32 oracle inf {y_inf:.3e} two {y_2:.3e} | sign mismatches "
              f"device {100 * sb:.4f}% float32 oracle {100 * sb32:.4f}% | exact zeros in float64 {z64}, all exact on the device: {zdev}")
    print(f"{name}: yardstick (worst float32 oracle) inf {yard_inf:.3e} two {yard_2:.3e}; bounds {8 * yard_inf:.3e} / {8 * yard_2:.3e}; "
          f"worst device inf {max(r[1][1][0] for r in rows):.3e} two {max(r[1][1][1] for r in rows):.3e} "
          f"sign {100 * max(r[1][3] for r in rows):.4f}%")
    for tag, (i, (e_inf, e_2), _, sb, _, _, _) in rows:
        assert e_inf <= 8 * yard_inf, (tag, i, e_inf)
        assert e_2 <= 8 * yard_2, (tag, i, e_2)
        assert sb <= 0.002, (tag, i, sb)  # the L-inf step takes sign(g)


@pytest.mark.parametrize("shape", H.SHORT_SHAPES, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s in H.SHORT_SHAPES])
def test_vjp_short_matches_the_float64_oracle(cuda, shape):
    """MI355X, worst row per shape: see DESIGN.md 3 ("Backward pass", short-window plans) for the recorded figures."""
    n_fft, hop, n = shape
    b = BATCH[shape]
    ex = _short(n, n_fft, hop, b)
    assert ex.n_frames == 1 + n // hop and ex.n_y == n
    sig = H.short_parity_batch(n_fft, hop, n, b)
    st = torch.as_tensor(sig).to(cuda).contiguous()
    rng = np.random.default_rng(n_fft * 1000 + hop)
    rows = []
    for L in _lengths(shape):
        gf = rng.standard_normal((b, 20 * L)).astype(np.float32)
        scale = rng.uniform(0.5, 2.0, 20 * L)
        got = ex.vjp_short(st, torch.as_tensor(gf).to(cuda), L, torch.as_tensor(scale).to(cuda)).double().cpu().numpy()
        assert np.isfinite(got).all()
        rows += [(f"L={L}", r) for r in _parity_rows(got, sig, gf, scale, dict(n_fft=n_fft, hop=hop, utterance_length=L, domain="22k"))]
        for _, r in rows[-b:]:
            assert r[6], r
            if L < ex.n_frames:  # the samples only frames >= L reach receive exactly 0 (441/220, L = 98: 489 of them)
                assert r[5] > 0, r
    _report_and_check(f"vjp_short {shape}", rows)
    ex.close()


@pytest.fixture(scope="module")
def sr_plan(cuda):
    ex = _short(22050, 441, 220, 8)
    sig = torch.as_tensor(H.short_parity_batch(441, 220, 22050, 6)).to(cuda).contiguous()
    rng = np.random.default_rng(9)
    gf = torch.as_tensor(rng.standard_normal((6, 2020)).astype(np.float32)).to(cuda)
    mean = torch.as_tensor(rng.standard_normal(2020)).to(cuda)
    scale = torch.as_tensor(rng.uniform(0.5, 2.0, 2020)).to(cuda)
    return dict(ex=ex, sig=sig, gf=gf, mean=mean, scale=scale)


def test_reuse_forward_and_reruns_give_the_same_bits(sr_plan):
    ex, sig, gf, scale = sr_plan["ex"], sr_plan["sig"], sr_plan["gf"], sr_plan["scale"]
    a = ex.vjp_short(sig, gf, 101, scale).clone()
    b = ex.vjp_short(sig, gf, 101, scale).clone()
    # another batch in between, so that a stale intermediate could not go unnoticed
    ex.vjp_short(sig.flip(0).contiguous()[:4], gf[:4], 101, scale)
    ex.from_22k(sig, 101, sr_plan["mean"], scale)
    c = ex.vjp_short(sig, gf, 101, scale, reuse_forward=True).clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert float(a.abs().max()) > 0


def test_zero_batch_identity_plan_and_unsupported_plans(sr_plan, cuda):
    from lipasr import _native as N
    from lipasr.extract_features_construct_dataset import MfccExtractor

    ex, sig, gf = sr_plan["ex"], sr_plan["sig"], sr_plan["gf"]
    z = ex.vjp_short(torch.zeros(6, 22050, device=cuda), gf, 101)
    assert torch.isfinite(z).all() and float(z.abs().max()) == 0.0
    # 22 050 Hz input: the resampler is the identity, the two domains coincide
    assert torch.equal(ex.vjp_short(sig, gf, 101, domain="input"), ex.vjp_short(sig, gf, 101, domain="22k"))

    def unsupported(fn):
        with pytest.raises(N.LipasrError) as e:
            fn()
        assert e.value.code == N.EUNSUPPORTED

    unsupported(lambda: ex.vjp(sig, gf, 101, domain="22k"))  # lipasr_mfcc_plan_vjp keeps refusing short-window plans
    e2 = MfccExtractor(16000, 16000, batch_max=2)
    unsupported(lambda: e2.vjp_short(torch.zeros(2, 16000, device=cuda), torch.zeros(2, 880, device=cuda), 44, domain="input"))
    with pytest.raises(ValueError):
        ex.vjp_short(sig, gf, 101, domain="mel")
    with pytest.raises(ValueError):
        ex.vjp_short(sig[:, :-1].contiguous(), gf, 101)
    e2.close()


def test_domain_input_at_16_khz_matches_the_oracle_composed_with_the_resampler_adjoint(cuda):
    ex = _short(H.INPUT_SAMPLES, 441, 220, 4, sr=H.INPUT_RATE)
    assert ex.n_y == 22050 and ex.n_frames == 101
    x = H.input_rate_clips()
    rng = np.random.default_rng(21)
    gf = rng.standard_normal((3, 2020)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, 2020)
    got = ex.vjp_short(torch.as_tensor(x).to(cuda), torch.as_tensor(gf).to(cuda), 101, torch.as_tensor(scale).to(cuda), domain="input")
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all()
    rows = [("16 kHz", r) for r in _parity_rows(got, x, gf, scale, dict(n_fft=441, hop=220, utterance_length=101, sr_in=H.INPUT_RATE,
                                                                       domain="input"))]
    _report_and_check("vjp_short domain input", rows)
    ex.close()


@pytest.fixture(scope="module")
def sr_model(cuda):
    """The signed-glorot Speaker-recognition unconstrained classifier (an untrained non-negative network with its own labels has an
    exactly zero gradient) behind a scaler fitted on the windows' features."""
    from lipasr.speaker_recognition import mfcc_windows

    spec = P.sr_unconstrained_spec()
    p = P.init_params(spec, seed=3, nonneg_init=False)
    m = build_model(spec, max_batch=32)
    load_params(m, p)
    t = np.arange(22050) / 22050.0
    rng = np.random.default_rng(12)
    w = np.stack([H.short_parity_batch(441, 220, 22050, 6)[i % 6] * (1.0 - 0.02 * (i // 6)) + 0.002 * rng.standard_normal(22050) +
                  0.05 * np.sin(2 * np.pi * (500.0 + 130.0 * i) * t) for i in range(32)]).astype(np.float32)
    w[:6] = H.short_parity_batch(441, 220, 22050, 6)
    feats = mfcc_windows(w).double().cpu().numpy()
    mean, scale = feats.mean(axis=0), feats.std(axis=0)
    scale[scale == 0.0] = 1.0
    return dict(spec=spec, p=p, model=m, w=w, mean=mean, scale=scale)


def test_waveform_classifier_loss_gradient_matches_the_composed_oracle(sr_model, cuda):
    from lipasr.speaker_recognition import waveform_classifier

    spec, p, m, mean, scale = (sr_model[k] for k in ("spec", "p", "model", "mean", "scale"))
    clf = waveform_classifier(m, mean, scale)
    assert clf.n == 22050 and clf.utterance_length == 101 and clf.nb_classes == 20 and clf.domain == "22k"
    x = sr_model["w"][:6]
    pred = clf.predict(x).argmax(axis=1)
    y = H.onehot((pred + 1 + np.arange(6)) % 20, 20)
    got = clf.loss_gradient(x, y).astype(np.float64)
    assert got.shape == (6, 22050) and np.isfinite(got).all() and np.abs(got).max() > 0
    kw = dict(n_fft=441, hop=220, utterance_length=101, domain="22k")
    f64 = np.stack([H.features(torch.as_tensor(x[i].astype(np.float64)), mean=mean, scale=scale, **kw).numpy() for i in range(6)])
    f32 = np.stack([H.features(torch.as_tensor(x[i].astype(np.float64)), mean=mean, scale=scale, dtype=torch.float32, **kw).numpy() for i in range(6)])
    gf64 = P.input_gradient_infer(spec, p.astype(np.float64), f64, y.astype(np.float64))
    gf32 = P.input_gradient_infer(spec, p.astype(np.float32), f32.astype(np.float32), y.astype(np.float32))
    rows = []
    for i in range(6):
        g64 = H.vjp(x[i], gf64[i], scale=scale, **kw)
        g32 = H.vjp(x[i], gf32[i].astype(np.float64), scale=scale, dtype=torch.float32, **kw)
        rows.append((i, H.errs(got[i], g64), H.errs(g32, g64)))
    yard_inf, yard_2 = max(r[2][0] for r in rows), max(r[2][1] for r in rows)
    for i, (e_inf, e_2), (y_inf, y_2) in rows:
        print(f"loss_gradient window {i}: device inf {e_inf:.3e} two {e_2:.3e} | composed float32 oracle inf {y_inf:.3e} two {y_2:.3e}")
    print(f"loss_gradient: bounds 8 x ({yard_inf:.3e}, {yard_2:.3e}); worst device inf {max(r[1][0] for r in rows):.3e} two {max(r[1][1] for r in rows):.3e}")
    for i, (e_inf, e_2), _ in rows:
        assert e_inf <= 8 * yard_inf, (i, e_inf)
        assert e_2 <= 8 * yard_2, (i, e_2)
    with pytest.raises(ValueError):
        clf.loss_gradient(x, y, lengths=[22050] * 6)
    clf.extractor.close()


def test_pgd_linf_over_the_windows(sr_model, cuda):
    from lipasr import attacks as A
    from lipasr.speaker_recognition import waveform_classifier

    eps = 0.01
    m = sr_model["model"]
    clf = waveform_classifier(m, sr_model["mean"], sr_model["scale"])
    x0 = torch.as_tensor(sr_model["w"]).to(cuda).contiguous()
    keep = x0.clone()
    # a feature-domain attack on the same model before and after: the audio path leaves it untouched
    fx = torch.as_tensor(np.random.default_rng(2).standard_normal((32, 2020)).astype(np.float32)).to(cuda)
    fclf = A.TensorFlowV2Classifier(model=m, nb_classes=20, input_shape=(2020,))
    before = A.ProjectedGradientDescent(estimator=fclf, eps=0.5, eps_step=0.1, max_iter=5).generate_device(fx)
    lab = clf.predict_device(x0).argmax(dim=1).cpu().numpy().astype(np.int64)  # the model's own labels: CE can only be pushed up
    y = torch.as_tensor(H.onehot(lab, 20)).to(cuda)
    adv = A.ProjectedGradientDescent(estimator=clf, eps=eps, eps_step=eps / 4, max_iter=8, batch_size=32).generate_device(x0, y)
    assert torch.equal(x0, keep) and adv.data_ptr() != x0.data_ptr()
    assert float((adv - x0).abs().max()) <= eps + float(np.spacing(np.float32(1.0)))
    assert float(adv.max()) <= 1.0 and float(adv.min()) >= -1.0
    gen = torch.Generator(device="cpu").manual_seed(5)
    noise = (torch.randint(0, 2, x0.shape, generator=gen).float() * 2 - 1).to(cuda) * eps
    res = {}
    for name, x in (("clean", x0), ("noise", (x0 + noise).clamp_(-1.0, 1.0)), ("pgd", adv)):
        res[name] = H.mean_ce(clf.predict_device(x).double().cpu().numpy(), lab)
    print(f"pgd-linf over 32 windows, eps {eps}: " + ", ".join(f"{k}: CE {v:.4f}" for k, v in res.items()))
    assert res["pgd"] > res["clean"] and res["pgd"] > res["noise"]
    after = A.ProjectedGradientDescent(estimator=fclf, eps=0.5, eps_step=0.1, max_iter=5).generate_device(fx)
    assert torch.equal(before, after) and not torch.equal(before, fx)
    clf.extractor.close()


def test_white_box_audio_sweep(sr_model, tmp_path, capsys, cuda):
    from lipasr import attacks as A, speaker_recognition as S

    rng = np.random.default_rng(40)
    files = []
    for i in range(4):  # 4.2 s at 22 050 Hz: two whole windows per file after the first and the last second are dropped
        n = int(22050 * 4.2)
        t = np.arange(n) / 22050.0
        x = 0.3 * np.sin(2 * np.pi * (300.0 + 250.0 * i) * t * (1 + 0.05 * t)) + 0.01 * rng.standard_normal(n)
        path = tmp_path / f"rec_{i}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(22050)
            f.writeframes((np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    m = sr_model["model"]
    feats, _ = S.load_audio_dataset_and_labels(files, [0] * 4)
    assert feats.shape == (8, 2020)
    train, val = feats[:4], feats[4:]
    # the clean accuracy, computed here: the windows through a classifier of our own behind the statistics of (train, val, clean).
    # A file's label is what the (untrained) model says on its first window, so that the clean accuracy is not trivially 0.
    sc = A.StandardScaler().fit(np.concatenate([train, val, feats]))
    windows = np.concatenate([S.split_windows(S._load_22k(f)) for f in files])
    clf = S.waveform_classifier(m, sc.mean_, sc.scale_)
    pred = clf.predict(windows).argmax(axis=1)
    clf.extractor.close()
    labels = [int(pred[2 * i]) for i in range(4)]
    want = float(np.mean(pred == np.repeat(labels, 2)))
    assert want >= 0.5
    models = {"constrained": m, "unconstrained": m}
    grid, acc = S.white_box_audio_sweep(models, train, val, files, labels, kind="pgd", grid=[0, 0.01], eps_step=0.0025, max_iter=4)
    assert grid == [0, 0.01]
    for k in models:
        assert acc[k].shape == (2,)
        assert acc[k][0] == want, (acc[k][0], want)
        assert acc[k][1] <= acc[k][0]
    assert S.white_box_audio_sweep(models, train, val, files, labels, kind="fgsm", points=2)[0] == [0, 0.002]
    with pytest.raises(ValueError):
        S.white_box_audio_sweep(models, train, val, files, labels, kind="jsma")
    assert "Accuracy on adversarial audio test examples" in capsys.readouterr().out
