"""Waveform-domain FGM / PGD: the native backward pass of the MFCC stage (lipasr_mfcc_plan_vjp) against the float64 autograd
oracle of tests/mfcc_grad_ref.py, its determinism and edge cases, and the attacks built on it.

Parity bounds are 8 x the error of the SAME oracle graph evaluated in float32 (computed here, on the CPU): 8 = 2^3 is the ratio
of the forward kernels' 2^-21 per-product error (fp16 two-plane split; the backward reads their dB tile) to fp32's 2^-24."""
import wave

import numpy as np
import pytest
import torch

import mfcc_grad_ref as G
from helpers import build_model, load_params
from oracle import mfcc_ref as M, mlp_ref as P

pytestmark = pytest.mark.gpu

L = 44
DOMAINS = ("22k", "input")


@pytest.fixture(scope="module")
def parity(cuda):
    """The twelve clips, a signed-glorot unconstrained classifier, a scaler fitted on the clips' features and, per clip, a label
    different from the prediction (an untrained non-negative network with its own labels has an exactly zero gradient)."""
    from lipasr import _native as N
    from lipasr.extract_features_construct_dataset import MfccExtractor

    spec = P.vd_unconstrained_spec()
    p = P.init_params(spec, seed=3, nonneg_init=False)
    m = build_model(spec, max_batch=32)
    load_params(m, p)
    ex, x, y22, raw = {}, {}, {}, {}
    for n in G.LENGTHS:
        ex[n] = MfccExtractor(16000, n, batch_max=8)
        x[n] = torch.as_tensor(G.parity_clips(n)).to(cuda).contiguous()
        y22[n] = ex[n].resample(x[n])
        raw[n] = ex[n](x[n], L)
    feats = torch.cat([raw[n] for n in G.LENGTHS]).double().cpu().numpy()
    mean, scale = feats.mean(axis=0), feats.std(axis=0)
    scale[scale == 0.0] = 1.0
    mean_t, scale_t = torch.as_tensor(mean).to(cuda), torch.as_tensor(scale).to(cuda)
    out = dict(spec=spec, p64=p.astype(np.float64), model=m, ex=ex, x=x, y22=y22, mean=mean, scale=scale, mean_t=mean_t, scale_t=scale_t,
               y={}, g_feat={})
    for n in G.LENGTHS:
        f = ex[n](x[n], L, mean_t, scale_t)
        pred = m.predict_device(f).argmax(dim=1).cpu().numpy()
        out["y"][n] = G.onehot((pred + 1 + np.arange(4)) % 10, 10)
        yt = torch.as_tensor(out["y"][n]).to(cuda)
        gf = torch.empty_like(f)
        N.check(N.lib.lipasr_mlp_input_grad(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(f), N.ptr(yt), 4, N.ptr(gf), N.stream_ptr()))
        assert float(gf.abs().max()) > 0
        out["g_feat"][n] = gf
    torch.cuda.synchronize()
    return out


def _sig(parity, n, domain):
    return parity["y22"][n] if domain == "22k" else parity["x"][n]


@pytest.mark.parametrize("domain", DOMAINS)
def test_vjp_matches_the_float64_oracle(parity, domain):
    """MI355X, worst of the twelve clips: see DESIGN.md 3 ("Backward pass") for the recorded figures."""
    rows = []
    for n in G.LENGTHS:
        sig, gf = _sig(parity, n, domain), parity["g_feat"][n]
        got = parity["ex"][n].vjp(sig, gf, L, parity["scale_t"], domain=domain).double().cpu().numpy()
        assert np.isfinite(got).all()
        for i in range(4):
            rows.append((n, i) + G.parity_row(got[i], sig[i].double().cpu().numpy(), gf[i].double().cpu().numpy(), scale=parity["scale"],
                                              domain=domain)[:4])
    yard_inf, yard_2 = max(r[3][0] for r in rows), max(r[3][1] for r in rows)
    for n, i, (e_inf, e_2), (y_inf, y_2), sb, sb32 in rows:
        print(f"vjp {domain} {G.CLIP_NAMES[i]} n={n}: device inf {e_inf:.3e} two {e_2:.3e} | float32 oracle inf {y_inf:.3e} two {y_2:.3e} | "
              f"sign mismatches device {100 * sb:.4f}% float32 oracle {100 * sb32:.4f}%")
    print(f"vjp {domain}: yardstick (worst float32 oracle) inf {yard_inf:.3e} two {yard_2:.3e}; bounds {8 * yard_inf:.3e} / {8 * yard_2:.3e}; "
          f"worst device inf {max(r[2][0] for r in rows):.3e} two {max(r[2][1] for r in rows):.3e}")
    for n, i, (e_inf, e_2), _, sb, _ in rows:
        assert e_inf <= 8 * yard_inf, (n, i, e_inf)
        assert e_2 <= 8 * yard_2, (n, i, e_2)
        assert sb <= 0.002, (n, i, sb)  # the L-inf step takes sign(g)


def test_resampler_adjoint(cuda):
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(17)
    for sr, n in ((16000, 16000), (16000, 12000), (8000, 8000), (22050, 9000)):
        ex = MfccExtractor(sr, n, batch_max=4)
        x = torch.as_tensor(rng.standard_normal((4, n)).astype(np.float32) * 0.3).to(cuda)
        v = torch.as_tensor(rng.standard_normal((4, ex.n_y)).astype(np.float32)).to(cuda)
        rx, rtv = ex.resample(x).double().cpu().numpy(), ex.resample_vjp(v).double().cpu().numpy()
        xd, vd = x.double().cpu().numpy(), v.double().cpu().numpy()
        for i in range(4):
            lhs, rhs = float(rx[i] @ vd[i]), float(xd[i] @ rtv[i])
            bound = 2.0 ** -16 * np.linalg.norm(rx[i]) * np.linalg.norm(vd[i])
            print(f"adjoint sr {sr} n {n} clip {i}: <Rx, v> {lhs:.9e} <x, R^T v> {rhs:.9e} |diff| {abs(lhs - rhs):.3e} bound {bound:.3e}")
            assert abs(lhs - rhs) <= bound
        ex.close()


@pytest.mark.parametrize("domain", DOMAINS)
def test_reuse_forward_and_reruns_give_the_same_bits(parity, domain):
    n = 16000
    ex, sig, gf = parity["ex"][n], _sig(parity, n, domain), parity["g_feat"][n]
    a = ex.vjp(sig, gf, L, parity["scale_t"], domain=domain).clone()
    b = ex.vjp(sig, gf, L, parity["scale_t"], domain=domain).clone()
    # another signal in between, so that a stale intermediate could not go unnoticed
    ex.vjp(_sig(parity, n, domain).flip(0).contiguous(), gf, L, parity["scale_t"], domain=domain)
    if domain == "22k":
        ex.from_22k(sig, L, parity["mean_t"], parity["scale_t"])
    else:
        ex(sig, L, parity["mean_t"], parity["scale_t"])
    c = ex.vjp(sig, gf, L, parity["scale_t"], domain=domain, reuse_forward=True).clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert float(a.abs().max()) > 0


def test_zero_clip_identity_plan_and_unsupported_inputs(cuda):
    from lipasr import _native as N
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(4)
    g = torch.as_tensor(rng.standard_normal((2, 20 * L)).astype(np.float32)).to(cuda)
    ex = MfccExtractor(16000, 16000, batch_max=2)
    for domain, n in (("input", 16000), ("22k", ex.n_y)):
        z = ex.vjp(torch.zeros(2, n, device=cuda), g, L, domain=domain)
        assert torch.isfinite(z).all() and float(z.abs().max()) == 0.0
    # 22 050 Hz input: the resampler is the identity, the two domains coincide
    ei = MfccExtractor(22050, 22050, batch_max=2)
    w = torch.as_tensor(G.parity_clips(22050, sr=22050)[:2]).to(cuda).contiguous()
    assert torch.equal(ei.vjp(w, g, L, domain="input"), ei.vjp(w, g, L, domain="22k"))
    # no backward pass: short-window plans, int16 rows, per-clip lengths, clips shorter than the reflect padding
    def unsupported(fn):
        with pytest.raises(N.LipasrError) as e:
            fn()
        assert e.value.code == N.EUNSUPPORTED

    es = MfccExtractor(22050, 22050, batch_max=2, n_fft=441, hop=220)
    unsupported(lambda: es.vjp(w, torch.zeros(2, 20 * 101, device=cuda), 101, domain="22k"))
    x = torch.zeros(2, 16000, device=cuda)
    unsupported(lambda: ex.vjp(torch.zeros(2, 16000, dtype=torch.int16, device=cuda), g, L))
    unsupported(lambda: ex.vjp(x, g, L, n_valid=torch.full((2,), 12000, dtype=torch.int32, device=cuda)))
    et = MfccExtractor(16000, 1000, batch_max=2)
    unsupported(lambda: et.vjp(torch.zeros(2, 1000, device=cuda), g, L))
    with pytest.raises(ValueError):
        ex.vjp(x, g, L, domain="mel")
    for e in (ex, ei, es, et):
        e.close()


@pytest.mark.parametrize("domain", DOMAINS)
def test_fgm_l2_step_matches_the_composed_oracle(parity, domain):
    """x_adv - x0 against eps g64 / |g64|_2, g64 from restatement -> mlp_ref.input_gradient_infer -> autograd."""
    from lipasr import attacks as A

    eps = 0.5
    rows = []
    for n in G.LENGTHS:
        clf = A.WaveformClassifier(parity["model"], 10, extractor=parity["ex"][n], utterance_length=L, mean=parity["mean"], scale=parity["scale"],
                                   domain=domain)
        x0 = _sig(parity, n, domain)
        keep = x0.clone()
        adv = A.FastGradientMethod(estimator=clf, eps=eps, norm=2, batch_size=32).generate_device(x0, torch.as_tensor(parity["y"][n]).to(x0.device))
        assert torch.equal(x0, keep) and adv.data_ptr() != x0.data_ptr()
        delta = (adv.double() - x0.double()).cpu().numpy()
        for i in range(4):
            s64 = x0[i].double().cpu().numpy()
            f64 = G.features(torch.as_tensor(s64), mean=parity["mean"], scale=parity["scale"], domain=domain).numpy()
            gfeat = P.input_gradient_infer(parity["spec"], parity["p64"], f64[None, :], parity["y"][n][i:i + 1].astype(np.float64))[0]
            g64 = G.vjp(s64, gfeat, scale=parity["scale"], domain=domain)
            g32 = G.vjp(s64, gfeat, scale=parity["scale"], domain=domain, dtype=torch.float32)
            u64 = g64 / np.linalg.norm(g64)
            rows.append((n, i, float(np.linalg.norm(delta[i] - eps * u64) / eps), float(np.linalg.norm(g32 / np.linalg.norm(g32) - u64))))
    yard = max(r[3] for r in rows)
    for n, i, e, y in rows:
        print(f"fgm-l2 {domain} {G.CLIP_NAMES[i]} n={n}: |delta - eps u64| / eps = {e:.3e} (float32 oracle direction error {y:.3e})")
    print(f"fgm-l2 {domain}: bound 8 x {yard:.3e} = {8 * yard:.3e}; worst device {max(r[2] for r in rows):.3e}")
    for n, i, e, _ in rows:
        assert e <= 8 * yard, (n, i, e)


@pytest.fixture(scope="module")
def trained(cuda):
    """A classifier trained for a few epochs on MFCCs of synthetic clips, with the scaler it was trained behind."""
    from lipasr import attacks as A, keras as K
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.synth import synth_clips

    waves, labels = synth_clips(448, seed=31)
    ex = MfccExtractor(16000, 16000, batch_max=64)
    w = torch.as_tensor(waves).to(cuda)
    feats = torch.cat([ex(w[s:s + 64].contiguous(), L) for s in range(0, 448, 64)])
    sc = A.StandardScaler().fit(feats[:320])
    K.reset_layer_names()
    m = build_model(P.vd_unconstrained_spec(), max_batch=64)
    tr = sc.transform_device(feats[:320]).cpu().numpy()
    m.fit(K.Dataset.from_tensor_slices((tr, K.to_categorical(labels[:320], 10))).batch(64), epochs=10, verbose=0)
    return dict(model=m, ex=ex, sc=sc, waves=waves, w=w, labels=labels, feats=feats)


@pytest.mark.parametrize("domain", DOMAINS)
def test_pgd_linf_over_audio(trained, domain, cuda):
    from lipasr import attack_eval as V, attacks as A

    eps = V.AUDIO_SIGMAS[3]  # 0.01
    m, ex, sc = trained["model"], trained["ex"], trained["sc"]
    clf = A.WaveformClassifier(m, 10, extractor=ex, utterance_length=L, mean=sc.mean_, scale=sc.scale_, domain=domain)
    w = trained["w"][320:448].contiguous()
    lab = trained["labels"][320:448].astype(np.int64)
    x0 = torch.cat([ex.resample(w[s:s + 64]) for s in (0, 64)]) if domain == "22k" else w
    keep = x0.clone()
    y = torch.as_tensor(G.onehot(lab, 10)).to(cuda)
    adv = A.ProjectedGradientDescent(estimator=clf, eps=eps, eps_step=eps / 4, max_iter=10, batch_size=64).generate_device(x0, y)
    assert torch.equal(x0, keep)
    assert float((adv - x0).abs().max()) <= eps + float(np.spacing(np.float32(1.0)))
    assert float(adv.max()) <= 1.0 and float(adv.min()) >= -1.0
    gen = torch.Generator(device="cpu").manual_seed(5)
    noise = (torch.randint(0, 2, x0.shape, generator=gen).float() * 2 - 1).to(cuda) * eps
    noisy = (x0 + noise).clamp_(-1.0, 1.0)
    res = {}
    for name, x in (("clean", x0), ("noise", noisy), ("pgd", adv)):
        prob = clf.predict_device(x).double().cpu().numpy()
        res[name] = (G.mean_ce(prob, lab), float((prob.argmax(axis=1) == lab).mean()))
    print(f"pgd-linf over audio, domain {domain}, eps {eps}: " + ", ".join(f"{k}: CE {v[0]:.4f} accuracy {v[1]:.4f}" for k, v in res.items()))
    assert res["pgd"][0] > res["clean"][0] and res["pgd"][0] > res["noise"][0]
    assert res["pgd"][1] <= res["noise"][1]
    # y=None: the model's own clean predictions; random starts stay in the ball and in [-1, 1]
    adv2 = A.ProjectedGradientDescent(estimator=clf, eps=eps, eps_step=eps / 2, max_iter=3, batch_size=64, num_random_init=2).generate_device(x0[:64])
    assert float((adv2 - x0[:64]).abs().max()) <= eps + float(np.spacing(np.float32(1.0)))
    assert float(adv2.abs().max()) <= 1.0
    # NumPy in, NumPy out
    g = clf.loss_gradient(x0[:4].cpu().numpy(), G.onehot(lab[:4], 10))
    assert g.shape == (4, x0.shape[1]) and np.isfinite(g).all() and np.abs(g).max() > 0


def test_feature_domain_attacks_are_untouched(trained, cuda):
    """With a TensorFlowV2Classifier the estimator check is the only new code on the path: same result, call after call."""
    from lipasr import attacks as A

    m, sc = trained["model"], trained["sc"]
    x = sc.transform_device(trained["feats"][320:384])
    clf = A.TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))
    for kw in (dict(), dict(norm=2)):
        a = A.ProjectedGradientDescent(estimator=clf, eps=0.5, eps_step=0.1, max_iter=5, **kw).generate_device(x)
        b = A.ProjectedGradientDescent(estimator=clf, eps=0.5, eps_step=0.1, max_iter=5, **kw).generate_device(x)
        assert torch.equal(a, b) and not torch.equal(a, x)


def test_white_box_audio_sweep_anchors_on_the_black_box_sweep(trained, tmp_path, capsys):
    from lipasr import attack_eval as V
    from lipasr.extract_features_construct_dataset import compute_mfcc_all_files

    files = []
    for i in range(48):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(trained["waves"][i], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = compute_mfcc_all_files(files)
    labels = G.onehot(trained["labels"][32:48].astype(np.int64), 10)
    models = {"constrained": trained["model"], "unconstrained": trained["model"]}
    args = (models, feats[:24], feats[24:32], feats[32:48], labels)
    _, black = V.black_box_sweep(*args, kind="simple", over="audio", test_filenames=files[32:48], grid=[0])
    for domain in DOMAINS:
        grid, white = V.white_box_sweep(*args, kind="pgd", over="audio", test_filenames=files[32:48], domain=domain, grid=[0, 0.01],
                                        eps_step=0.0025, max_iter=5)
        assert grid == [0, 0.01]
        for k in models:
            assert white[k][0] == black[k][0]
            assert white[k][1] <= white[k][0]
    assert V.white_box_sweep(*args, kind="fgsm", over="audio", test_filenames=files[32:48], points=2)[0] == V.AUDIO_SIGMAS[:2]
    with pytest.raises(ValueError):
        V.white_box_sweep(*args, kind="jsma", over="audio", test_filenames=files[32:48])
    assert "Accuracy on adversarial audio test examples" in capsys.readouterr().out
