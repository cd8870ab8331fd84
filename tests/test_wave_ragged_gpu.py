"""Clips of different lengths in one launch of the MFCC backward pass (lipasr_mfcc_plan_vjp_ragged) and of the attacks over
audio (lengths=): parity against the float64 oracle of tests/mfcc_grad_ref.py on each clip alone, the same bits as the
one-length call where that exists, determinism, the edges, int16 rows, the split forward, the attacks and the sweep.

One plan of 20 000-sample rows serves every test.  Parity bounds follow tests/test_wave_attacks_gpu.py: 8 x the error of the SAME
oracle graph evaluated in float32, the yardstick recomputed here among the four clips of a row's own length."""
import math
import wave

import numpy as np
import pytest
import torch

import mfcc_grad_ref as G
from helpers import build_model, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu

L = 44
N_ROW = 20000
DOMAINS = ("22k", "input")
SAME_BITS = (3000, 7000, 12000, 16000, 20000)  # multiples of 4 with n_y > 2048: the one-length call exists for the clip alone


def _n22(n):
    return int(math.ceil(n * (22050.0 / 16000.0)))


def _end(n, domain):
    """where clip of n samples ends in a row of the given domain"""
    return n if domain == "input" else _n22(n)


def _i32(v, dev):
    return torch.as_tensor(np.asarray(v, dtype=np.int32)).to(dev)


def _fill_tails(t, ends, rng, amp):
    for u, e in enumerate(ends):
        t[u, e:] = torch.as_tensor((amp * rng.standard_normal(t.shape[1] - e)).astype(np.float32)).to(t.device)
    return t


@pytest.fixture(scope="module")
def rag(cuda):
    """The forty parity clips side by side in rows of 20 000 samples (tails: 10 x noise, which nothing may read), a signed-glorot
    classifier, a scaler fitted on the clips' features and a cotangent from a label different from the prediction."""
    from lipasr import _native as N
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(77)
    spec = P.vd_unconstrained_spec()
    p = P.init_params(spec, seed=3, nonneg_init=False)
    m = build_model(spec, max_batch=48)
    load_params(m, p)
    ex = MfccExtractor(16000, N_ROW, batch_max=48)
    lens = [n for n in G.RAGGED_LENGTHS for _ in range(4)]
    x = torch.zeros(len(lens), N_ROW, device=cuda)
    for k, n in enumerate(G.RAGGED_LENGTHS):
        x[4 * k:4 * k + 4, :n] = torch.as_tensor(G.parity_clips(n)).to(cuda)
    _fill_tails(x, lens, rng, 10.0)
    lt = _i32(lens, cuda)
    y22 = _fill_tails(ex.resample(x, n_valid=lt).clone(), [_n22(n) for n in lens], rng, 10.0)
    feats = ex(x, L, n_valid=lt).double().cpu().numpy()
    mean, scale = feats.mean(axis=0), feats.std(axis=0)
    scale[scale == 0.0] = 1.0
    mean_t, scale_t = torch.as_tensor(mean).to(cuda), torch.as_tensor(scale).to(cuda)
    f = ex(x, L, mean_t, scale_t, n_valid=lt)
    pred = m.predict_device(f).argmax(dim=1).cpu().numpy()
    y = G.onehot((pred + 1 + np.arange(len(lens)) % 4) % 10, 10)
    gf = torch.empty_like(f)
    N.check(N.lib.lipasr_mlp_input_grad(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(f), N.ptr(torch.as_tensor(y).to(cuda)), len(lens),
                                        N.ptr(gf), N.stream_ptr()))
    assert float(gf.abs().max()) > 0
    torch.cuda.synchronize()
    return dict(model=m, ex=ex, lens=lens, lt=lt, x=x, y22=y22, mean=mean, scale=scale, mean_t=mean_t, scale_t=scale_t, y=y, g_feat=gf)


def _sig(rag, domain):
    return rag["y22"] if domain == "22k" else rag["x"]


@pytest.mark.parametrize("domain", DOMAINS)
def test_ragged_vjp_matches_the_float64_oracle_on_each_clip_alone(rag, domain):
    """Per row: inf- and 2-norm error relative to the float64 gradient's, bound 8 x the worst float32-oracle error among the four
    clips of the row's length.  The sign criterion (<= 0.2 % mismatches) is asserted from 12 000 samples up; below, one sample is
    >= 0.01 % of a clip and the float32 oracle itself reaches 0.2 %: printed.  MI355X figures: DESIGN.md 3 ("K1 backward"); no row
    above 0.40 of its bound."""
    sig, gf, lens = _sig(rag, domain), rag["g_feat"], rag["lens"]
    got = rag["ex"].vjp_ragged(sig, gf, rag["lt"], L, rag["scale_t"], domain=domain).double().cpu().numpy()
    assert np.isfinite(got).all()
    rows = []
    for u, n in enumerate(lens):
        e = _end(n, domain)
        row = G.parity_row(got[u, :e], sig[u, :e].double().cpu().numpy(), gf[u].double().cpu().numpy(), scale=rag["scale"], domain=domain)
        rows.append((u, n) + row[:4] + (float(np.abs(got[u, e:]).max()) if e < got.shape[1] else 0.0,))
    yard = {n: (max(r[3][0] for r in rows if r[1] == n), max(r[3][1] for r in rows if r[1] == n)) for n in G.RAGGED_LENGTHS}
    for u, n, (e_inf, e_2), (y_inf, y_2), sb, sb32, tail in rows:
        print(f"ragged vjp {domain} {G.CLIP_NAMES[u % 4]} n={n}: device inf {e_inf:.3e} two {e_2:.3e} | float32 oracle inf {y_inf:.3e} two "
              f"{y_2:.3e} | bounds {8 * yard[n][0]:.3e} / {8 * yard[n][1]:.3e} | sign mismatches device {100 * sb:.4f}% float32 oracle "
              f"{100 * sb32:.4f}% | max |g| past the end {tail:.1e}")
    for u, n, (e_inf, e_2), _, sb, _, tail in rows:
        assert e_inf <= 8 * yard[n][0], (n, u, e_inf)
        assert e_2 <= 8 * yard[n][1], (n, u, e_2)
        if n >= 12000:
            assert sb <= 0.002, (n, u, sb)  # the L-inf step takes sign(g)
        assert tail == 0.0, (n, u, tail)


@pytest.mark.parametrize("domain", DOMAINS)
def test_ragged_rows_have_the_bits_of_the_one_length_call(rag, domain, cuda):
    from lipasr.extract_features_construct_dataset import MfccExtractor

    ex, sig, gf = rag["ex"], _sig(rag, domain), rag["g_feat"]
    got = ex.vjp_ragged(sig, gf, rag["lt"], L, rag["scale_t"], domain=domain).clone()
    for n in SAME_BITS:
        rows = [u for u, m in enumerate(rag["lens"]) if m == n]
        e = _end(n, domain)
        one = MfccExtractor(16000, n, batch_max=4)
        assert one.n_y == _n22(n)
        alone = one.vjp(sig[rows, :e].contiguous(), gf[rows].contiguous(), L, rag["scale_t"], domain=domain)
        assert float(alone.abs().max()) > 0
        assert torch.equal(got[rows, :e], alone), n
        one.close()
    # every length equal to the row length: the one-length call on the same plan
    full = [u for u, m in enumerate(rag["lens"]) if m == N_ROW]
    xs = rag["x"][full].contiguous()
    s = ex.resample(xs) if domain == "22k" else xs
    a = ex.vjp_ragged(s, gf[full].contiguous(), _i32([N_ROW] * len(full), cuda), L, rag["scale_t"], domain=domain).clone()
    b = ex.vjp(s, gf[full].contiguous(), L, rag["scale_t"], domain=domain)
    assert torch.equal(a, b) and float(a.abs().max()) > 0


@pytest.mark.parametrize("domain", DOMAINS)
def test_ragged_reruns_and_reuse_forward_give_the_same_bits(rag, domain):
    ex, sig, gf, lt = rag["ex"], _sig(rag, domain), rag["g_feat"], rag["lt"]
    a = ex.vjp_ragged(sig, gf, lt, L, rag["scale_t"], domain=domain).clone()
    b = ex.vjp_ragged(sig, gf, lt, L, rag["scale_t"], domain=domain).clone()
    # another batch in between, so that a stale intermediate could not go unnoticed
    ex.vjp_ragged(sig.flip(0).contiguous(), gf, lt.flip(0).contiguous(), L, rag["scale_t"], domain=domain)
    if domain == "22k":
        ex.from_22k(sig, L, rag["mean_t"], rag["scale_t"], n_valid=lt)
    else:
        ex(sig, L, rag["mean_t"], rag["scale_t"], n_valid=lt)
    c = ex.vjp_ragged(sig, gf, lt, L, rag["scale_t"], domain=domain, reuse_forward=True).clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert float(a.abs().max()) > 0


@pytest.mark.parametrize("domain", DOMAINS)
def test_ragged_edges(rag, domain, cuda):
    """Clips of 0, 1, 2 and 37 samples: finite, zeros past the end (all zeros for the empty clip), and deaf to the tail."""
    ex = rag["ex"]
    rng = np.random.default_rng(5)
    lens = [0, 1, 2, 37]
    lt = _i32(lens, cuda)
    x = torch.as_tensor((0.1 * rng.standard_normal((4, N_ROW))).astype(np.float32)).to(cuda)
    sig = ex.resample(x, n_valid=lt).clone() if domain == "22k" else x
    ends = [_end(n, domain) for n in lens]
    gf = torch.as_tensor(rng.standard_normal((4, 20 * L)).astype(np.float32)).to(cuda)
    a = ex.vjp_ragged(_fill_tails(sig.clone(), ends, rng, 10.0), gf, lt, L, rag["scale_t"], domain=domain).clone()
    b = ex.vjp_ragged(_fill_tails(sig.clone(), ends, rng, 3.0), gf, lt, L, rag["scale_t"], domain=domain).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert float(a[0].abs().max()) == 0.0
    for u, e in enumerate(ends):
        assert float(a[u, e:].abs().max()) == 0.0
    assert float(a[3].abs().max()) > 0


def test_int16_rows_and_unsupported_plans(rag, cuda):
    from lipasr import _native as N
    from lipasr.extract_features_construct_dataset import MfccExtractor

    ex, gf, lt, lens = rag["ex"], rag["g_feat"], rag["lt"], rag["lens"]
    rng = np.random.default_rng(9)
    pcm = torch.as_tensor(rng.integers(-32768, 32768, size=(len(lens), N_ROW)).astype(np.int16)).to(cuda)
    for u, n in enumerate(lens):
        pcm[u, :n] = (rag["x"][u, :n] * 32767.0).to(torch.int16)
    a = ex.vjp_ragged(pcm, gf, lt, L, rag["scale_t"]).clone()
    b = ex.vjp_ragged((pcm.float() / 32768.0).contiguous(), gf, lt, L, rag["scale_t"])
    assert a.dtype == torch.float32 and torch.equal(a, b) and float(a.abs().max()) > 0

    def unsupported(fn):
        with pytest.raises(N.LipasrError) as e:
            fn()
        assert e.value.code == N.EUNSUPPORTED

    g2, l2 = gf[:2].contiguous(), _i32([9000, 12000], cuda)
    unsupported(lambda: ex.vjp_ragged(torch.zeros(2, ex.n_y, dtype=torch.int16, device=cuda), g2, l2, L, domain="22k"))
    e22 = MfccExtractor(22050, N_ROW, batch_max=2)
    unsupported(lambda: e22.vjp_ragged(torch.zeros(2, N_ROW, device=cuda), g2, l2, L))
    unsupported(lambda: e22.vjp_ragged(torch.zeros(2, N_ROW, device=cuda), g2, l2, L, domain="22k"))
    es = MfccExtractor(16000, 16000, batch_max=2, n_fft=441, hop=220)
    unsupported(lambda: es.vjp_ragged(torch.zeros(2, 16000, device=cuda), torch.zeros(2, 20 * 101, device=cuda), l2, 101))
    eo = MfccExtractor(16000, 15998, batch_max=2)
    unsupported(lambda: eo.vjp_ragged(torch.zeros(2, 15998, device=cuda), g2, l2, L))
    unsupported(lambda: eo.vjp_ragged(torch.zeros(2, eo.n_y, device=cuda), g2, l2, L, domain="22k"))
    with pytest.raises(ValueError):
        ex.vjp_ragged(rag["x"][:2].contiguous(), g2, l2.long(), L)
    for e in (e22, es, eo):
        e.close()


def test_ragged_resample_and_from_22k_compose_to_the_extraction(rag):
    ex, x, lt, lens = rag["ex"], rag["x"], rag["lt"], rag["lens"]
    y = ex.resample(x, n_valid=lt)
    for u, n in enumerate(lens):
        assert float(y[u, int(n * (22050.0 / 16000.0)):].abs().max()) == 0.0, n
    assert float(y.abs().max()) > 0
    whole = ex(x, L, rag["mean_t"], rag["scale_t"], n_valid=lt).clone()
    assert torch.equal(ex.from_22k(y, L, rag["mean_t"], rag["scale_t"], n_valid=lt), whole)


ATTACK_LENGTHS = (8000, 12000, 16000, 20000)


@pytest.mark.parametrize("domain", DOMAINS)
def test_attacks_with_lengths_equal_the_attack_on_each_clip_alone(rag, domain, cuda):
    """Row k of the ragged batch is clip k of length ATTACK_LENGTHS[k]; alone, it is row k of the four clips of that length through a
    one-length classifier (same batch size and row, so that the classifier's own arithmetic is the same)."""
    from lipasr import attacks as A
    from lipasr.extract_features_construct_dataset import MfccExtractor

    rng = np.random.default_rng(21)
    ex, m = rag["ex"], rag["model"]
    lt = _i32(ATTACK_LENGTHS, cuda)
    clips = {n: torch.as_tensor(G.parity_clips(n)).to(cuda).contiguous() for n in ATTACK_LENGTHS}
    x = torch.zeros(4, N_ROW, device=cuda)
    for k, n in enumerate(ATTACK_LENGTHS):
        x[k, :n] = clips[n][k]
    ends = [_end(n, domain) for n in ATTACK_LENGTHS]
    x0 = _fill_tails((ex.resample(x, n_valid=lt).clone() if domain == "22k" else x), ends, rng, 2.0)  # tails outside [-1, 1] too
    keep = x0.clone()
    clf = A.WaveformClassifier(m, 10, extractor=ex, utterance_length=L, mean=rag["mean"], scale=rag["scale"], domain=domain)
    pred = clf.predict_device(x0, lengths=lt).argmax(dim=1).cpu().numpy()
    y = torch.as_tensor(G.onehot((pred + 1 + np.arange(4)) % 10, 10)).to(cuda)
    eps = 0.01
    attacks = {"pgd": lambda c: A.ProjectedGradientDescent(estimator=c, eps=eps, eps_step=eps / 4, max_iter=5, batch_size=32),
               "fgm": lambda c: A.FastGradientMethod(estimator=c, eps=eps, batch_size=32)}
    adv = {k: mk(clf).generate_device(x0, y, lengths=lt) for k, mk in attacks.items()}
    assert torch.equal(x0, keep)
    for name, a in adv.items():
        for k, e in enumerate(ends):
            assert torch.equal(a[k, e:], x0[k, e:]), (name, k)
            assert float((a[k, :e] - x0[k, :e]).abs().max()) > 0.5 * eps, (name, k)
    for k, n in enumerate(ATTACK_LENGTHS):
        one = MfccExtractor(16000, n, batch_max=4)
        c1 = A.WaveformClassifier(m, 10, extractor=one, utterance_length=L, mean=rag["mean"], scale=rag["scale"], domain=domain)
        s = one.resample(clips[n]) if domain == "22k" else clips[n]
        assert torch.equal(s[k], x0[k, :ends[k]])
        # domain "22k", n * 22050 / 16000 not an integer (12 000, 20 000): position int(n r) of the row is the zero fix_length
        # appends.  The forward with per-clip lengths reads it as zero whatever the row holds; the one-length classifier reads
        # what is there -- and a first step has moved it, since the backward (as the one-length call, bit for bit) hands that
        # position its gradient.  From the second step on the two classifiers see different signals: only a single step (FGM)
        # can agree there.  At the input rate, and where n r is an integer, every step agrees.
        exact = domain == "input" or (n * 22050) % 16000 == 0
        for name, mk in attacks.items():
            if name == "pgd" and not exact:
                continue
            alone = mk(c1).generate_device(s, y)
            assert torch.equal(adv[name][k, :ends[k]], alone[k]), (name, n)
        one.close()
    # norm 2 with random starts: inside the ball, tail untouched
    a2 = A.ProjectedGradientDescent(estimator=clf, eps=0.5, eps_step=0.2, max_iter=3, norm=2, num_random_init=2,
                                    batch_size=32).generate_device(x0, y, lengths=lt)
    d = (a2.double() - x0.double())
    for k, e in enumerate(ends):
        assert torch.equal(a2[k, e:], x0[k, e:])
        nrm = float(d[k].norm())
        print(f"pgd-l2 {domain} n={ATTACK_LENGTHS[k]}: |delta|_2 = {nrm:.6f} (eps 0.5)")
        assert 0 < nrm <= 0.5 * (1 + 1e-6)
    # NumPy in / NumPy out
    g = clf.loss_gradient(x0.cpu().numpy(), y.cpu().numpy(), lengths=list(ATTACK_LENGTHS))
    assert g.shape == tuple(x0.shape) and np.isfinite(g).all() and all(np.abs(g[k, e:]).max() == 0 for k, e in enumerate(ends) if e < g.shape[1])


def test_white_box_audio_sweep_over_files_of_different_lengths(tmp_path, cuda, capsys):
    """Four lengths, one of them 1000 samples (62 ms: no one-length backward pass exists for it): one extractor for the rate, and
    at eps = 0 the accuracies of the black-box sweep at sigma = 0."""
    from lipasr import attack_eval as V, attacks as A, keras as K
    from lipasr import extract_features_construct_dataset as X
    from lipasr.synth import synth_clips

    waves, labels = synth_clips(112, seed=31)
    cut = (16000, 12000, 8000, 1000)
    files = []
    for i in range(112):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(waves[i][:cut[i % 4]], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats = X.compute_mfcc_all_files(files)
    sc = A.StandardScaler().fit(feats[:96])
    K.reset_layer_names()
    m = build_model(P.vd_unconstrained_spec(), max_batch=16)
    m.fit(K.Dataset.from_tensor_slices((sc.transform(feats[:80]).astype(np.float32), K.to_categorical(labels[:80], 10))).batch(16), epochs=6,
          verbose=0)
    test = files[96:112]
    onehot = G.onehot(labels[96:112].astype(np.int64), 10)
    models = {"constrained": m, "unconstrained": m}
    args = (models, feats[:80], feats[80:96], feats[96:112], onehot)
    _, black = V.black_box_sweep(*args, kind="simple", over="audio", test_filenames=test, grid=[0])
    for domain in DOMAINS:
        before = dict(X._extractors)
        grid, white = V.white_box_sweep(*args, kind="pgd", over="audio", test_filenames=test, domain=domain, grid=[0, 0.01], eps_step=0.0025,
                                        max_iter=3)
        made = [k for k, v in X._extractors.items() if before.get(k) is not v]
        assert len(made) <= 1 and all(k[:2] == (16000, 16000) for k in made), made
        assert (16000, 16000, torch.cuda.current_device()) in X._extractors
        assert grid == [0, 0.01]
        for k in models:
            assert white[k][0] == black[k][0]
            assert white[k][1] <= white[k][0]
    assert "Accuracy on adversarial audio test examples" in capsys.readouterr().out
