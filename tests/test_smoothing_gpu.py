"""Randomized smoothing on the MI355X: lipasr_smooth_expand and lipasr_smooth_vote against the float64 restatement of
tests/smoothing_ref.py on the same arrays, their conventions (include/lipasr.h), lipasr.smoothing.Smooth against a hand-built chain
of the same calls, CERTIFY end to end where the answer is known, and the read-outs built on it.

Bounds.  expand: |out - (x + sigma z_ref)| <= 1e-5 sigma + half a unit in the last place of out -- the 1e-5 is the bound of the
noise table (test_smoothing_cpu.test_noise_table_matches_the_restatement derives it: about 5e-6 from fp32 logf / sincosf), the
half unit is the one rounding of the fused multiply-add.  vote: exact.  Smooth.counts_device against the hand-built chain: exact,
the same kernels on the same chunk."""
import math
import time
import wave
from statistics import NormalDist

import numpy as np
import pytest
import torch

import deepfool_ref as D
import local_lip_ref as R
import smoothing_ref as S
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P

pytestmark = pytest.mark.gpu


def _place(x, offset=0, dtype=torch.float32):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation."""
    buf = torch.zeros(x.size + offset, device="cuda", dtype=dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _expand(x, draws, sigma, seed, n_valid=None, clip=None, clip0=0, draw0=0, x_off=0, out_off=0):
    """One lipasr_smooth_expand -> NumPy float32 [B * draws, n]."""
    from lipasr.smoothing import smooth_expand

    B, n = x.shape
    xt = _place(np.asarray(x, dtype=np.float32), x_off)
    out = torch.full((B * draws * n + out_off,), 7.0, device="cuda")[out_off:].view(B * draws, n)
    nv = None if n_valid is None else torch.as_tensor(np.asarray(n_valid, dtype=np.int32)).cuda()
    got = smooth_expand(xt, draws, sigma, seed, clip0=clip0, draw0=draw0, n_valid=nv, clip_values=clip, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _check_expand(got, x, draws, sigma, seed, what, n_valid=None, clip=None, **kw):
    lo, hi = (-np.inf, np.inf) if clip is None else clip
    want, valid = S.expand(x, draws, sigma, seed, n_valid=n_valid, lo=lo, hi=hi, **kw)
    xr = np.repeat(x, draws, axis=0)
    assert got[~valid].tobytes() == xr[~valid].tobytes(), f"{what}: padding moved"
    err = np.abs(got.astype(np.float64) - want)
    bound = 1e-5 * sigma + 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = (err[valid] / sigma).max() if valid.any() and sigma > 0 else 0.0
    print(f"{what}: worst |out - (x + sigma z_ref)| / sigma {worst:.2e} (bound 1e-5 + half a unit in the last place of out)")
    assert (err[valid] <= bound[valid]).all(), what


# =================================================================================================
# 1. expand
# =================================================================================================
SHAPES = [(1, 1, 1), (3, 5, 880), (2, 3, 881), (2, 4, 2020), (2, 2, 22050), (4, 2, 67)]
SIGMA = 0.05


def _rows(B, n, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((B, n))).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_expand_matches_float64(cuda, shape):
    B, draws, n = shape
    seed = sum(shape)
    x = _rows(B, n, seed)
    base = None
    for x_off in (0, 1):
        for out_off in (0, 1):
            got = _expand(x, draws, SIGMA, seed, x_off=x_off, out_off=out_off)
            _check_expand(got, x, draws, SIGMA, seed, f"{shape} x + {x_off} out + {out_off}")
            # the alignment picks the loads and stores, never a value
            base = got if base is None else base
            assert got.tobytes() == base.tobytes()
    # every n_valid of the issue, cycled over the rows; the padding keeps the bits of x
    values = [0, 1, 5, n - 1, n, n + 3, -2]
    for s in range(0, len(values), B):
        nv = (values[s:] + values)[:B]
        for off in (0, 1):
            got = _expand(x, draws, SIGMA, seed, n_valid=nv, x_off=off, out_off=off)
            _check_expand(got, x, draws, SIGMA, seed, f"{shape} n_valid {nv} offset {off}", n_valid=nv)
            valid = np.repeat(np.clip(nv, 0, n), draws)[:, None] > np.arange(n)[None, :]
            assert np.array_equal(got[valid], base[valid])  # the valid part is what the call without lengths wrote


def test_expand_clips_the_valid_part_only(cuda):
    x = _rows(3, 881, 5)  # |x| up to ~1: most of it outside [-0.01, 0.01]
    nv = [881, 400, 0]
    got = _expand(x, 4, SIGMA, 9, n_valid=nv, clip=(-0.01, 0.01))
    _check_expand(got, x, 4, SIGMA, 9, "clip", n_valid=nv, clip=(-0.01, 0.01))
    valid = np.repeat(nv, 4)[:, None] > np.arange(881)[None, :]
    assert got[valid].min() >= -0.01 and got[valid].max() <= 0.01 and (got[valid] == np.float32(0.01)).any()
    assert np.abs(got[~valid]).max() > 0.5  # the padding is not clamped


def test_expand_draws_do_not_depend_on_the_chunk(cuda):
    x = _rows(3, 881, 6)
    whole = _expand(x, 5, SIGMA, 11)
    a, b = _expand(x, 3, SIGMA, 11, draw0=0), _expand(x, 2, SIGMA, 11, draw0=3)
    glued = np.concatenate([np.concatenate([a[3 * r:3 * r + 3], b[2 * r:2 * r + 2]]) for r in range(3)])
    assert glued.tobytes() == whole.tobytes()
    single = np.concatenate([_expand(x[r:r + 1], 5, SIGMA, 11, clip0=r) for r in range(3)])
    assert single.tobytes() == whole.tobytes()
    assert _expand(x, 5, SIGMA, 11).tobytes() == whole.tobytes()  # two runs, the same bits
    assert np.abs(_expand(x, 5, SIGMA, 12) - whole).max() > SIGMA  # another seed, other draws
    zero = _expand(x, 2, 0.0, 11)
    assert np.array_equal(zero, np.repeat(x, 2, axis=0))


def test_one_draw_is_the_white_noise_attack(cuda):
    """draws = 1, clip0 = draw0 = 0 carry the counters of lipasr_add_noise_f32 mode 0: add_white_noise(x, sigma, seed) to one unit
    in the last place (x + sigma z there, one fused multiply-add here)."""
    from lipasr.attacks import add_white_noise

    for n in (880, 881, 22050):
        x = _rows(3, n, n)
        got, want = _expand(x, 1, SIGMA, 21), add_white_noise(x, SIGMA, seed=21)
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
        assert np.abs(got - x).max() > SIGMA


def test_expand_argument_checks(cuda):
    from lipasr import _native as N
    from lipasr.smoothing import smooth_expand

    x = torch.zeros(2, 8, device="cuda")
    for kw in (dict(sigma=-1.0), dict(sigma=math.inf), dict(sigma=math.nan), dict(sigma=0.1, clip_values=(1.0, -1.0))):
        with pytest.raises(ValueError):
            smooth_expand(x, 3, kw.pop("sigma"), 0, **kw)
    with pytest.raises(ValueError):
        smooth_expand(x, 3, 0.1, 0, n_valid=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        smooth_expand(x.t(), 3, 0.1, 0)
    assert smooth_expand(x, 0, 0.1, 0).shape == (0, 8) and smooth_expand(x[:0], 3, 0.1, 0).shape == (0, 8)
    h = N.get_handle(0)
    assert N.lib.lipasr_smooth_expand(h.h, None, None, 0, 8, 3, 0, 0, 0.1, 0, -np.inf, np.inf, None, N.stream_ptr()) == N.OK
    assert N.lib.lipasr_smooth_expand(h.h, None, None, 2, 8, 3, 0, 0, 0.1, 0, -np.inf, np.inf, None, N.stream_ptr()) == N.EINVAL


# =================================================================================================
# 2. vote
# =================================================================================================
def _vote(logits, batch, counts=None, offset=0):
    from lipasr.smoothing import smooth_vote

    lt = _place(np.asarray(logits, dtype=np.float32), offset)
    C_ = logits.shape[1]
    ct = torch.zeros(batch, C_ + 1, dtype=torch.int32, device="cuda") if counts is None else counts
    smooth_vote(lt, batch, ct)
    torch.cuda.synchronize()
    return ct


def _logits(batch, draws, C_, seed):
    """Random logits with exact ties, +inf (alone and twice in a row), -inf rows and NaN rows mixed in."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((batch * draws, C_)).astype(np.float32)
    rows = z.shape[0]
    kind = rng.integers(0, 8, rows)
    for r in range(rows):
        if kind[r] == 1 and C_ > 1:  # a tie of the maximum: the lowest index wins
            i, j = rng.choice(C_, 2, replace=False)
            z[r, i] = z[r, j] = z[r].max() + 1
        elif kind[r] == 2:
            z[r, rng.integers(C_)] = np.inf
        elif kind[r] == 3 and C_ > 1:
            i, j = rng.choice(C_, 2, replace=False)
            z[r, i] = z[r, j] = np.inf
        elif kind[r] == 4:
            z[r, rng.integers(C_)] = np.nan
        elif kind[r] == 5:
            z[r, :] = -np.inf
        elif kind[r] == 6 and C_ > 1:  # a NaN next to an inf still goes to the extra bin
            i, j = rng.choice(C_, 2, replace=False)
            z[r, i], z[r, j] = np.nan, np.inf
    return z


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("C_", [1, 2, 10, 20, 32])
def test_vote_matches_numpy(cuda, C_, batch):
    for draws in (1, 63, 64, 65, 257, 1024):
        z = _logits(batch, draws, C_, seed=1000 * C_ + draws + batch)
        want = S.vote(z, batch)
        assert (want.sum(axis=1) == draws).all()
        got = _vote(z, batch)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"C {C_} draws {draws} batch {batch}")
        np.testing.assert_array_equal(_vote(z, batch, offset=1).cpu().numpy(), want)
        # a second call accumulates; two runs give the same bits
        z2 = _logits(batch, draws, C_, seed=7 + draws)
        np.testing.assert_array_equal(_vote(z2, batch, counts=got).cpu().numpy(), want + S.vote(z2, batch))


def test_vote_conventions(cuda):
    z = np.array([[1.0, 3.0, 3.0], [np.inf, 2.0, np.inf], [np.nan, 9.0, 1.0], [-np.inf, -np.inf, -np.inf], [0.0, 0.0, 5.0], [1.0, 0.0, 0.0]],
                 dtype=np.float32)
    np.testing.assert_array_equal(_vote(z, 2).cpu().numpy(), [[1, 1, 0, 1], [2, 0, 1, 0]])
    # counts of other clips are untouched: the call owns rows 1 and 2 of a [4, C + 1] array
    counts = torch.full((4, 4), 5, dtype=torch.int32, device="cuda")
    _vote(z, 2, counts=counts[1:3])
    np.testing.assert_array_equal(counts.cpu().numpy(), [[5, 5, 5, 5], [6, 6, 5, 6], [7, 5, 6, 5], [5, 5, 5, 5]])
    from lipasr.smoothing import smooth_vote

    with pytest.raises(ValueError, match="33 classes"):
        smooth_vote(torch.zeros(4, 33, device="cuda"), 2, torch.zeros(2, 34, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        smooth_vote(torch.zeros(5, 3, device="cuda"), 2, torch.zeros(2, 4, dtype=torch.int32, device="cuda"))
    empty = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    smooth_vote(torch.zeros(0, 3, device="cuda"), 2, empty)
    assert not empty.any()


# =================================================================================================
# 3. Smooth.counts_device against the hand-built chain
# =================================================================================================
FEATURE_CASES = {"vd": P.vd_constrained_spec, "sr": P.sr_constrained_spec}


def _feature_case(name):
    """The oracle models with setup_params(spec, 7) and 16 rows of np.random.default_rng(3).standard_normal: the inputs of
    tests/test_deepfool_*."""
    from lipasr.attacks import TensorFlowV2Classifier

    spec = FEATURE_CASES[name]()
    p = R.setup_params(spec, 7)
    m = build_model(spec)
    load_params(m, p)
    n, C_ = spec[0].n_in, spec[-1].n_out
    x = np.random.default_rng(3).standard_normal((16, n)).astype(np.float32)
    return dict(name=name, spec=spec, p64=p.astype(np.float64), model=m, x=x, n=n, C=C_,
                clf=TensorFlowV2Classifier(model=m, nb_classes=C_, input_shape=(n,)))


@pytest.fixture(scope="module")
def feats(cuda):
    cases = {}
    return lambda name: cases.setdefault(name, _feature_case(name))


def _bincount(z, batch, C_):
    am = torch.argmax(z, dim=1).view(batch, -1)
    return torch.stack([torch.bincount(row, minlength=C_) for row in am]).cpu().numpy()


@pytest.mark.parametrize("name", sorted(FEATURE_CASES))
def test_counts_over_features_equal_the_hand_built_chain(feats, name):
    from lipasr.smoothing import Smooth, smooth_expand

    case = feats(name)
    clf, C_ = case["clf"], case["C"]
    xt = dev(case["x"][:4])
    sigma = 2.0  # the float64 oracle's largest vote shares there: 199 or 200 of 200 (880 -> 10), 67 .. 91 of 200 (2020 -> 20)
    sm = Smooth(clf, sigma, seed=3)
    assert 4 * 200 <= clf.batch_limit  # one chunk
    got = sm.counts_device(xt, 200, draw0=7).cpu().numpy()
    noisy = smooth_expand(xt, 200, sigma, 3, draw0=7)
    z = clf.model.predict_device(noisy, logits=True)
    want = _bincount(z, 4, C_)
    print(f"{name}: votes of 200 draws at sigma {sigma} (largest class per row) {want.max(axis=1).tolist()}")
    assert got.shape == (4, C_ + 1) and got.dtype == np.int32
    np.testing.assert_array_equal(got[:, :C_], want)
    assert not got[:, C_].any() and (got.sum(axis=1) == 200).all()


RAGGED = [16000, 9000, 37]


@pytest.fixture(scope="module")
def audio(cuda):
    """Three synthetic clips of 16000, 9000 and 37 samples in rows of 16000 at 16 kHz, one extractor, a WaveformClassifier per
    domain over the unconstrained 880 -> 10 model."""
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
    wt = torch.as_tensor(w).to(cuda).contiguous()
    rows = {"input": wt, "22k": ex.resample(wt, n_valid=lt)}
    clfs = {d: WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain=d) for d in rows}
    yield dict(model=m, ex=ex, lt=lt, rows=rows, clfs=clfs)
    ex.close()


@pytest.mark.parametrize("domain", ["22k", "input"])
def test_counts_over_ragged_audio_equal_the_hand_built_chain(audio, domain):
    from lipasr.smoothing import Smooth, smooth_expand

    clf, rows, lt = audio["clfs"][domain], audio["rows"][domain], audio["lt"]
    d, sigma = 8, 0.02
    assert 3 * d <= clf.batch_limit  # one chunk
    pos = [int(math.ceil(n * 22050.0 / 16000.0)) if domain == "22k" else n for n in RAGGED]
    sm = Smooth(clf, sigma, seed=5, clip_values=clf.clip_values)
    got = sm.counts_device(rows, d, lengths=lt).cpu().numpy()
    noisy = smooth_expand(rows, d, sigma, 5, n_valid=torch.as_tensor(np.array(pos, dtype=np.int32)).cuda(), clip_values=clf.clip_values)
    z = clf.predict_device(noisy, logits=True, lengths=lt.repeat_interleave(d))
    np.testing.assert_array_equal(got[:, :10], _bincount(z, 3, 10))
    assert (got.sum(axis=1) == d).all() and not got[:, 10].any()
    nz, x = noisy.cpu().numpy(), rows.cpu().numpy()
    for r, p in enumerate(pos):  # the noise stays inside each clip
        assert nz[r * d:(r + 1) * d, p:].tobytes() == np.repeat(x[r:r + 1, p:], d, axis=0).tobytes()
        assert np.abs(nz[r * d:(r + 1) * d, :p] - x[r, :p]).max() > sigma
    # lists and arrays are taken as the classifier takes them; without lengths every position is the clip's
    np.testing.assert_array_equal(sm.counts_device(rows, d, lengths=RAGGED).cpu().numpy(), got)
    assert (sm.counts_device(rows, d).cpu().numpy().sum(axis=1) == d).all()


def test_short_window_extractor_works_without_lengths(cuda):
    import mfcc_grad_ref as G
    from lipasr.smoothing import Smooth
    from lipasr.speaker_recognition import waveform_classifier

    spec = P.sr_unconstrained_spec()
    m = build_model(spec, max_batch=8)
    load_params(m, R.setup_params(spec, 3))
    w = G.short_parity_clips(441, 220, 22050)[:2]
    clf = waveform_classifier(m, np.zeros(2020), np.ones(2020), batch_max=4)
    try:
        sm = Smooth(clf, 0.01, seed=1)
        counts = sm.counts_device(torch.as_tensor(w).to(cuda), 6).cpu().numpy()  # two chunks per clip
        assert counts.shape == (2, 21) and (counts.sum(axis=1) == 6).all()
        with pytest.raises(ValueError):
            sm.counts_device(torch.as_tensor(w).to(cuda), 6, lengths=[22050, 22050])
    finally:
        clf.extractor.close()


def test_counts_over_several_chunks(cuda):
    from lipasr.attacks import TensorFlowV2Classifier
    from lipasr.smoothing import Smooth

    spec = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
    m = build_model(spec, max_batch=4)
    load_params(m, R.setup_params(spec, 2))
    clf = TensorFlowV2Classifier(model=m, nb_classes=5, input_shape=(36,))
    x = np.random.default_rng(4).standard_normal((3, 36)).astype(np.float32)
    clean = clf.predict(x).argmax(axis=1)
    counts = Smooth(clf, 0.0).counts_device(dev(x), 10).cpu().numpy()  # 4 + 4 + 2 draws per row, one row per chunk
    np.testing.assert_array_equal(counts, np.eye(6, dtype=np.int32)[clean] * 10)
    noisy = Smooth(clf, 1.0, seed=2).counts_device(dev(x), 10).cpu().numpy()
    assert (noisy.sum(axis=1) == 10).all()
    # two rows per chunk (draws 2 <= the limit 4) and a start inside the sequence: the same votes as draw by draw
    sm = Smooth(clf, 1.0, seed=2)
    by_two = sum(sm.counts_device(dev(x), 2, draw0=j).cpu().numpy() for j in range(0, 10, 2))
    np.testing.assert_array_equal(by_two, noisy)
    alone = sm.counts_device(dev(x[1:2]), 10).cpu().numpy()  # clip0 is the row index: row 1 alone is row 0 of its call
    np.testing.assert_array_equal(alone, Smooth(clf, 1.0, seed=2).counts_device(dev(np.stack([x[1], x[0]])), 10).cpu().numpy()[:1])
    assert Smooth(clf, 1.0).counts_device(dev(x[:0]), 10).shape == (0, 6) and not Smooth(clf, 1.0).counts_device(dev(x), 0).any()
    with pytest.raises(ValueError):
        sm.counts_device(dev(x), 10, lengths=[36, 36, 36])
    with pytest.raises(ValueError):
        sm.counts_device(dev(x[:, :35]), 10)
    with pytest.raises(ValueError):
        Smooth(clf, -0.1)
    # PREDICT: no noise, no doubt; one vote is never significant at alpha = 0.001
    np.testing.assert_array_equal(Smooth(clf, 0.0).predict(x, n=64), clean)
    assert (Smooth(clf, 0.0).predict(x, n=1) == -1).all()


# =================================================================================================
# 4. CERTIFY end to end
# =================================================================================================
def test_certify_on_a_linear_classifier(cuda):
    """The case of test_smoothing_cpu.test_oracle_certify_on_a_linear_classifier on the device: the same seed, the same
    inequalities (the smoothed classifier's exact radius is the distance d to the boundary)."""
    from lipasr.attacks import TensorFlowV2Classifier
    from lipasr.smoothing import Smooth

    W, bias, x, d, cls = S.linear_case(S.LINEAR_SEED, S.LINEAR_SIGMA)
    spec = [P.LayerSpec(880, 2, False, 0.0, False)]
    m = build_model(spec)
    p = P.Params(W=[W], b=[bias], gamma=[None], beta=[None], mov_mean=[None], mov_var=[None])
    load_params(m, p)
    clf = TensorFlowV2Classifier(model=m, nb_classes=2, input_shape=(880,))
    res = Smooth(clf, S.LINEAR_SIGMA, seed=S.LINEAR_SEED).certify(x, **S.LINEAR)
    S.check_linear(res["class"], res["radius"], d, cls, what="device")
    assert (res["counts"].sum(axis=1) == S.LINEAR["n"]).all() and (res["counts_select"].sum(axis=1) == S.LINEAR["n0"]).all()
    assert not res["invalid"].any()
    np.testing.assert_allclose(res["radius"], S.LINEAR_SIGMA * np.array([NormalDist().inv_cdf(q) for q in res["p_lower"]]), rtol=1e-12)
    for b in range(6):
        assert abs(res["p_lower"][b] - S.cp_lower(int(res["counts"][b, cls[b]]), S.LINEAR["n"], S.LINEAR["alpha"])) <= 1e-9
    # PREDICT agrees where it does not abstain; far from the boundary it never abstains
    pred = Smooth(clf, S.LINEAR_SIGMA, seed=S.LINEAR_SEED).predict(x, n=1000)
    assert ((pred == cls) | (pred == -1)).all() and (pred[2:] == cls[2:]).all()


def test_the_cap_and_the_two_certificates(feats):
    """On the rows of the constrained 880 -> 10 model.  The cap: with sigma = 1e-6 every vote goes to the clean class and the radius
    is sigma Phi^-1(alpha^(1/n)).  The two certificates: with sigma (sqrt(880) + 6) below the radius margin / (sqrt(2) L) that the
    Lipschitz bound certifies, no draw with ||z|| <= sqrt(880) + 6 (all but e^-18 of them) can leave the class: all 1024 vote for
    it.  The CPU restatement (deepfool_ref.lipschitz_bound, margin) gives certified radii of 3.0e-4 .. 8.7e-4 on the 16 rows: the
    largest admissible sigma is 8.3e-6 .. 2.4e-5, above 1e-6 on every row, and half the smallest one is used."""
    from lipasr.smoothing import Smooth

    case = feats("vd")
    clf, x, n = case["clf"], case["x"], 1024
    z = P.forward_infer(case["spec"], case["p64"], x.astype(np.float64), return_logits=True)
    clean = z.argmax(axis=1)
    certified = D.margin(z, clean) / (math.sqrt(2.0) * D.lipschitz_bound(case["spec"], case["p64"]))
    admissible = certified / (math.sqrt(880.0) + 6.0)
    print(f"certified radius {certified.min():.3e} .. {certified.max():.3e}; largest admissible sigma {admissible.min():.3e} .. {admissible.max():.3e}")
    assert (admissible > 1e-6).all()
    res = Smooth(clf, 1e-6, seed=1).certify(x, n0=16, n=n, alpha=0.001)
    np.testing.assert_array_equal(res["class"], clean)
    np.testing.assert_array_equal(res["counts"], np.eye(10, dtype=np.int64)[clean] * n)
    np.testing.assert_allclose(res["radius"], 1e-6 * NormalDist().inv_cdf(0.001 ** (1.0 / n)), rtol=1e-12)
    sigma = 0.5 * float(admissible.min())
    assert sigma * (math.sqrt(880.0) + 6.0) < certified.min()
    counts = Smooth(clf, sigma, seed=2).counts_device(dev(x), n).cpu().numpy()
    np.testing.assert_array_equal(counts[:, :10], np.eye(10, dtype=np.int64)[clean] * n)


# =================================================================================================
# 5. the read-outs
# =================================================================================================
BASE_KEYS = {"margin", "certified", "linear", "found", "flipped"}


def test_robustness_radius_with_smoothing(feats, audio):
    from lipasr.extract_features_construct_dataset import get_robustness_radius

    case = feats("vd")
    x = case["x"][:4]
    assert set(get_robustness_radius(case["clf"], x, norm=2, max_iter=10)) == BASE_KEYS
    r = get_robustness_radius(case["clf"], x, norm=2, max_iter=10, smoothing=dict(sigma=0.05, n0=16, n=256, alpha=0.01))
    assert set(r) == BASE_KEYS | {"smoothed_radius", "smoothed_class"}
    assert r["smoothed_radius"].dtype == np.float64 and r["smoothed_radius"].shape == (4,) and r["smoothed_class"].shape == (4,)
    assert ((r["smoothed_radius"] > 0) == (r["smoothed_class"] >= 0)).all()
    assert (r["smoothed_radius"] <= 0.05 * NormalDist().inv_cdf(0.01 ** (1.0 / 256)) * (1 + 1e-12)).all()
    with pytest.raises(ValueError):
        get_robustness_radius(case["clf"], x, max_iter=1, smoothing=dict(n=16))
    clf, rows, lt = audio["clfs"]["22k"], audio["rows"]["22k"], audio["lt"]
    assert set(get_robustness_radius(clf, rows, lengths=lt, max_iter=1)) == BASE_KEYS
    r = get_robustness_radius(clf, rows, lengths=lt, max_iter=1, smoothing=dict(sigma=1e-4, n0=8, n=24, alpha=0.01))
    assert set(r) == BASE_KEYS | {"smoothed_radius", "smoothed_class"} and r["certified"] is None
    assert r["smoothed_radius"].shape == (3,) and (r["smoothed_radius"] >= 0).all()


def test_smooth_report(cuda, tmp_path, capsys):
    from lipasr import attack_eval as V
    from lipasr.extract_features_construct_dataset import compute_mfcc_all_files
    from lipasr.keras import to_categorical
    from lipasr.synth import synth_clips

    waves, _ = synth_clips(12, seed=31)
    files = []
    for i in range(12):
        path = tmp_path / f"clip_{i:03d}.wav"
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((np.clip(waves[i], -1, 1) * 32767.0).astype("<i2").tobytes())
        files.append(str(path))
    feats_ = compute_mfcc_all_files(files)
    spec = P.vd_unconstrained_spec()
    m = build_model(spec, max_batch=64)
    load_params(m, R.setup_params(spec, 3))
    models = {"constrained": m, "unconstrained": m}
    train, val, test = feats_[:4], feats_[4:8], feats_[8:12]
    xs = V.A.standardize_dataset(train, val, test)[2]
    labels = to_categorical(m.predict(xs).argmax(axis=1), 10)  # the model's own classes: at most the abstentions are missing at radius 0
    capsys.readouterr()
    rep = V.smooth_report(models, train, val, test, labels, 1e-3, n0=8, n=64, alpha=0.01, over="mfcc")
    out = capsys.readouterr().out
    for name in models:
        r = rep[name]
        assert r["radius"].shape == (4,) and r["class"].shape == (4,) and len(r["certified_accuracy"]) == len(r["radii"]) == len(V.SMOOTH_RADII)
        assert (np.diff(r["certified_accuracy"]) <= 0).all() and r["certified_accuracy"][0] <= 1.0 - r["abstained"]
        assert r["certified_accuracy"][-1] == 0.0  # 4 sigma is above the cap sigma Phi^-1(0.01^(1/64)) = 1.47 sigma
    assert rep["constrained"]["lipschitz_median"] > 0 and rep["unconstrained"]["lipschitz_median"] is None
    assert "Certified accuracy of the smoothed classifier (sigma 0.001) over 4 test rows at L2 radius 0.0:" in out
    assert "Share of 4 test rows on which the smoothed classifier abstains unconstrained:" in out
    assert "Median radius the Lipschitz bound certifies for the base classifier over 4 test rows:" in out
    rep = V.smooth_report(models, train, val, test, labels, 1e-4, n0=4, n=16, alpha=0.05, over="audio", test_filenames=files[8:12], limit=3)
    out = capsys.readouterr().out
    r = rep["unconstrained"]
    assert r["radius"].shape == (3,) and r["lipschitz_median"] is None and "over 3 test files unconstrained at L2 radius" in out
    with pytest.raises(ValueError):
        V.smooth_report(models, train, val, test, labels, 1e-3, over="audio")
    with pytest.raises(ValueError):
        V.smooth_report(models, train, val, test, labels, -1.0)


# =================================================================================================
# 6. measured, not asserted
# =================================================================================================
def _median_spread(ms):
    ms = np.sort(np.asarray(ms))
    return f"median {np.median(ms) * 1e3:.1f} us (min {ms[0] * 1e3:.1f}, 90th percentile {ms[int(0.9 * (len(ms) - 1))] * 1e3:.1f})"


def _time_chunks(sm, rows, features, predict, C_, what, reps=60):
    """Device events around every stage of one chunk of 1024 noisy rows, ``reps`` chunks after a warm-up of the same shapes."""
    from lipasr import _native as N
    from lipasr.smoothing import smooth_expand, smooth_vote

    b, d = rows.shape[0], 1024 // rows.shape[0]
    counts = torch.zeros(b, C_ + 1, dtype=torch.int32, device="cuda")
    buf = torch.empty(b * d, rows.shape[1], device="cuda")
    stages = ["expand"] + (["extraction"] if features else []) + ["predict", "vote"]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)] for _ in range(reps)]
    for it in range(-5, reps):
        e = ev[max(it, 0)]
        e[0].record()
        noisy = smooth_expand(rows, d, sm.sigma, sm.seed, draw0=max(it, 0) * d, out=buf)
        e[1].record()
        k = 1
        if features:
            noisy = features(noisy)
            k += 1
            e[k].record()
        z = predict(noisy)
        e[k + 1].record()
        smooth_vote(z, b, counts)
        e[k + 2].record()
    torch.cuda.synchronize()
    for i, s in enumerate(stages):
        print(f"{what}: {s:10s} {_median_spread([e[i].elapsed_time(e[i + 1]) for e in ev])}")
    # the wall time of a chunk inside Smooth.counts_device, host loop included
    sm.counts_device(rows, 5 * d)
    torch.cuda.synchronize()
    walls = []
    for it in range(5):
        t0 = time.perf_counter()
        sm.counts_device(rows, 12 * d, draw0=it)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / 12 * 1e3)
    print(f"{what}: wall time per chunk in counts_device, 5 runs of 12 chunks: {_median_spread(walls)}")
    # the nearest existing yardstick for expand: lipasr_add_noise_f32 in place on a buffer of the same size
    h = N.get_handle(0)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for it in range(-5, reps):
        e = ev[max(it, 0)]
        e[0].record()
        N.check(N.lib.lipasr_add_noise_f32(h.h, N.ptr(buf), buf.shape[0], buf.shape[1], 0, sm.sigma, 0.0, it + 10, N.stream_ptr()))
        e[1].record()
    torch.cuda.synchronize()
    print(f"{what}: lipasr_add_noise_f32 on {buf.shape[0]} x {buf.shape[1]} in place: {_median_spread([e[0].elapsed_time(e[1]) for e in ev])}")


def test_print_chunk_times(feats, cuda):
    """Prints (asserts nothing about time: nothing at the parent commit does this work) the device time of every stage of a chunk
    of 1024 noisy rows, over features (n = 880) and over audio (n = 22050, domain "22k")."""
    from lipasr.attacks import WaveformClassifier
    from lipasr.extract_features_construct_dataset import MfccExtractor
    from lipasr.smoothing import Smooth

    case = feats("vd")
    clf, m = case["clf"], case["model"]
    _time_chunks(Smooth(clf, 0.25, seed=1), dev(case["x"][:4]), None, lambda t: m.predict_device(t, logits=True), 10, "features 1024 x 880")
    ex = MfccExtractor(16000, 16000, batch_max=1024)
    try:
        wc = WaveformClassifier(m, 10, extractor=ex, utterance_length=44, domain="22k")
        assert wc.batch_limit == 1024
        rows = (0.1 * torch.randn(4, wc.n, device=cuda, generator=torch.Generator(device=cuda).manual_seed(0))).contiguous()
        _time_chunks(Smooth(wc, 0.01, seed=1), rows, wc.features_device, lambda t: m.predict_device(t, logits=True), 10, "audio 1024 x 22050")
    finally:
        ex.close()
