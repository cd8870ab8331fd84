"""Auto-PGD on the MI355X: lipasr_apgd_loss and lipasr_apgd_step against the float64 oracle of tests/apgd_ref.py, the attack class
against a hand-built chain of the same calls and across chunks, and the attack end to end where the answer is known, on a small real
model against the oracle's run, over audio with per-clip lengths and through the evaluation menu.

Bounds.  Loss kernel: hit, the positions of the non-zero gradient entries and the NaN convention exact; f and dz within 2 units in the
last place of the float64 value rounded to fp32 (the kernel computes in fp64 and rounds once: half a unit, plus the libm's exp / log1p).
Step kernel: the state, the copies into x_best / g_best / x_adv, x_prev and the padding exact; x as derived in
test_step_matches_the_oracle."""
import itertools
import math
import wave

import numpy as np
import pytest
import torch

import apgd_ref as A
import genetic_ref as G
import local_lip_ref as R
from helpers import build_model, dev, load_params
from oracle import mlp_ref as P
from test_apgd_cpu import BOUNDARIES, LOSSES, REAL, REAL_CASES, linear_model, real_case, real_oracle
from test_genetic_gpu import RAGGED, SMALL, audio, small  # noqa: F401  (the fixtures of the genetic tests)

pytestmark = pytest.mark.gpu


def _place(x, offset=0, dtype=torch.float32):
    """NumPy [..] -> a contiguous device view that starts ``offset`` elements into its allocation."""
    buf = torch.zeros(x.size + offset, device="cuda", dtype=dtype)
    view = buf[offset:].view(*x.shape)
    view.copy_(torch.as_tensor(x))
    return view


def _ulps(got, want32):
    """|got - want| in units in the last place of want (float32 arrays, finite entries)."""
    return np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


# =================================================================================================
# 1. the loss kernel
# =================================================================================================
def _loss_rows(C_, rng, targeted):
    B = 24
    z = (2.0 * rng.standard_normal((B, C_))).astype(np.float32)
    labels = rng.integers(0, C_, B).astype(np.int32)
    if C_ >= 3:
        z[0, :3] = z[0].max() + 1.0          # an exact tie among the top three
        z[1, C_ - 3:] = z[1].max() + 0.5     # ... at the highest indices
        z[2, [0, C_ - 1]] = z[2].max() + 2.0  # a tie of two, a third below
        labels[0], labels[1], labels[2] = 1, C_ - 1, 0
    z[3, C_ - 1] = np.nan                    # a NaN member
    z[4] = np.nan                            # nothing but NaN
    z[5, 0] = np.inf                         # +inf
    labels[6], labels[7] = -1, C_            # labels outside the classes
    labels[8] = z[8].argmax()                # the label is the prediction ...
    labels[9] = (z[9].argmax() + 1) % C_     # ... and is not
    return z, labels


@pytest.mark.parametrize("loss_type,targeted,C_", [(0, t, c) for t in (False, True) for c in (1, 2, 3, 4, 10, 32)]
                         + [(1, False, c) for c in (3, 4, 10, 32)])
def test_loss_matches_float64(cuda, loss_type, targeted, C_):
    from lipasr.apgd import apgd_loss

    rng = np.random.default_rng(100 * C_ + 10 * loss_type + int(targeted))
    z, labels = _loss_rows(C_, rng, targeted)
    ref = A.loss(z, labels, loss_type, targeted)
    zt, lt = _place(z), torch.as_tensor(labels).cuda()
    f, dz, hit = apgd_loss(zt, lt, loss_type, targeted)
    torch.cuda.synchronize()
    f, dz, hit = f.cpu().numpy(), dz.cpu().numpy(), hit.cpu().numpy()
    bad = ref["bad"]
    assert bad[[3, 4, 5, 6, 7]].all() and not bad[8:].any()
    np.testing.assert_array_equal(hit, ref["hit"])
    assert np.isnan(f[bad]).all() and not np.isnan(f[~bad]).any() and not dz[bad].any() and not hit[bad].any()
    want_f, want_dz = ref["f"][~bad].astype(np.float32), ref["dz"][~bad].astype(np.float32)
    np.testing.assert_array_equal(dz[~bad] != 0, want_dz != 0)  # the chosen indices: where the gradient is not zero
    uf, ud = _ulps(f[~bad], want_f), _ulps(dz[~bad], want_dz)
    ud = np.where(want_dz == 0, 0.0, ud)
    uf = np.where(want_f == 0, np.abs(f[~bad]) > 0, uf)
    print(f"loss {loss_type} targeted {targeted} classes {C_}: f within {uf.max():.2f} ulp, dz within {ud.max():.2f} ulp")
    assert uf.max() <= 2.0 and ud.max() <= 2.0
    # into given tensors, twice: the same bits
    f2, dz2, hit2 = torch.empty_like(torch.as_tensor(f)).cuda(), torch.empty(24, C_, device="cuda"), torch.empty(24, dtype=torch.int32, device="cuda")
    out = apgd_loss(zt, lt, loss_type, targeted, f=f2, dz=dz2, hit=hit2)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == f2.data_ptr()
    assert f2.cpu().numpy().tobytes() == f.tobytes() and dz2.cpu().numpy().tobytes() == dz.tobytes() and hit2.cpu().numpy().tobytes() == hit.tobytes()


def test_loss_argument_checks(cuda):
    from lipasr.apgd import apgd_loss

    z, lab = torch.zeros(4, 5, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    apgd_loss(z, lab)
    for bad in (dict(loss_type="hinge"), dict(loss_type=1, targeted=True), dict(labels=lab.long()), dict(logits=z.t()),
                dict(logits=torch.zeros(4, 33, device="cuda")), dict(logits=torch.zeros(4, 2, device="cuda"), loss_type="difference_logits_ratio"),
                dict(f=torch.zeros(5, device="cuda"))):
        a = dict(dict(logits=z, labels=lab, loss_type=0, targeted=False), **bad)
        with pytest.raises(ValueError):
            apgd_loss(a.pop("logits"), a.pop("labels"), **a)
    assert apgd_loss(z[:0], lab[:0])[1].shape == (0, 5)


# =================================================================================================
# 2. the step kernel
# =================================================================================================
FLAG_CASES = ("first", "plain", "halve-1", "halve-2", "keep", "last")
WIDTHS = [1, 3, 37, 880, 881, 2020] + [w for b in BOUNDARIES for w in (b, b + 1)] + [22050]


def _step_inputs(rows, n, case, rng, eps, eta, with_nv):
    x0 = rng.standard_normal((rows, n)).astype(np.float32)
    near = lambda: (x0 + 0.5 * eps / math.sqrt(n) * rng.standard_normal((rows, n))).astype(np.float32)
    a = dict(x=near(), x_prev=near(), x0=x0, g=rng.standard_normal((rows, n)).astype(np.float32), x_best=near(),
             g_best=rng.standard_normal((rows, n)).astype(np.float32), x_adv=near())
    a["g"][0, 0] = np.nan
    a["g_best"][rows - 1, n - 1] = np.nan
    f = rng.standard_normal(rows).astype(np.float32)
    up = rng.random(rows) < 0.5
    st = dict(eta=np.full(rows, eta, dtype=np.float32) * np.where(rng.random(rows) < 0.5, 1.0, 0.5).astype(np.float32),
              f_prev=(f + np.where(rng.random(rows) < 0.5, 0.5, -0.5)).astype(np.float32),  # away from ties
              f_best=(f + np.where(up, -0.25, 0.75)).astype(np.float32), improved=rng.integers(0, 2, rows).astype(np.int32),
              reduced_last=np.ones(rows, dtype=np.int32), fooled=rng.integers(0, 2, rows).astype(np.int32),
              halvings=rng.integers(0, 5, rows).astype(np.int32))
    st["f_best_ckpt"] = (st["f_best"] - 0.125).astype(np.float32)
    ckpt = 0
    if case == "halve-1":    # improved <= 2 < 0.75 * 4; condition 2 is off (reduced_last = 1)
        ckpt = 4
    elif case == "halve-2":  # improved >= 4; not reduced at the last checkpoint, the best loss as it was then (no row improves on it)
        ckpt = 4
        st["improved"] += 4
        st["reduced_last"][:] = 0
        st["f_best"] = (f + 0.75).astype(np.float32)
        st["f_best_ckpt"] = st["f_best"].copy()
        if rows > 1:         # ... but one: its best loss moves, so it does not halve
            st["f_best"][1] = st["f_best_ckpt"][1] = f[1] - np.float32(0.25)
    elif case == "keep":     # improved >= 4, reduced at the last checkpoint
        ckpt = 4
        st["improved"] += 4
    elif case == "first":    # nothing of the state is read
        st = dict(eta=np.full(rows, np.nan, dtype=np.float32), f_prev=np.full(rows, np.nan, dtype=np.float32),
                  f_best=np.full(rows, np.nan, dtype=np.float32), f_best_ckpt=np.full(rows, np.nan, dtype=np.float32),
                  improved=np.full(rows, 77, dtype=np.int32), reduced_last=np.full(rows, 77, dtype=np.int32),
                  fooled=np.full(rows, 77, dtype=np.int32), halvings=np.full(rows, 77, dtype=np.int32))
        a["x_prev"][:] = np.nan
        if rows > 2:
            f[2] = np.nan    # stored as -inf
    hit = rng.integers(0, 2, rows).astype(np.int32)
    nv = None
    if with_nv:
        values = [0, 1, 5, n - 1, n, n + 3, -2]
        shift = int(rng.integers(0, 7))
        nv = np.array([values[(shift + r) % 7] for r in range(rows)], dtype=np.int32)
    return a, f, hit, st, ckpt, nv


def _run_step(a, f, hit, st, nv, offset, **kw):
    from lipasr.apgd import apgd_step

    t = {k: _place(v, offset) for k, v in a.items()}
    s = {k: torch.as_tensor(v).cuda() for k, v in st.items()}
    nvt = None if nv is None else torch.as_tensor(nv).cuda()
    got = apgd_step(t["x"], t["x_prev"], t["x0"], t["g"], t["x_best"], t["g_best"], t["x_adv"], torch.as_tensor(f).cuda(),
                    torch.as_tensor(hit).cuda(), s, n_valid=nvt, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == t["x"].data_ptr()
    return {k: v.cpu().numpy() for k, v in t.items()}, {k: v.cpu().numpy() for k, v in s.items()}


@pytest.mark.parametrize("n", WIDTHS)
def test_step_matches_the_oracle(cuda, n):
    """One launch against the oracle from the same fp32 inputs, for 1, 5 and 33 rows, both norms and the six flag cases; n_valid,
    the clip range and the alignment of the array bases vary from combination to combination.

    The tolerance on x.  The kernel converts its fp32 inputs to fp64, does every element-wise operation and every norm in fp64 and
    rounds x_new to fp32 ONCE; the oracle does the same in NumPy.  Norm inf: the two fp64 values differ by the ~20 fp64 operations
    between input and output, 20 x 2^-53 relative -- 2^-24 of an fp32 unit -- so the rounded results differ only where that moves a
    value across a rounding boundary: ONE rounded fp32 operation, one unit in the last place of the largest intermediate,
    max |x0| + 2 eta.  Norm 2: the three norms are sums of n squares in another order (n x 2^-53 relative) under a square root, far
    inside the 1e-6 relative tests/test_lp_attacks_gpu.py grants lipasr_lp_step's norms; each scales a vector no longer than
    eta (the direction), 2 eta + eps (the first projection's argument) and 2 eta + 2 eps (the second's), so 1e-6 (5 eta + 3 eps) is added."""
    eps, eta0 = 0.3, 0.6
    checked = {c: 0 for c in FLAG_CASES}
    for i, (rows, norm, case) in enumerate(itertools.product((1, 5, 33), (math.inf, 2.0), FLAG_CASES)):
        rng = np.random.default_rng(1000 * n + i)
        clip = (-1.25, 1.5) if i % 2 else None
        offset = (i // 2) % 2
        a, f, hit, st, ckpt, nv = _step_inputs(rows, n, case, rng, eps, eta0, with_nv=i % 3 != 0)
        kw = dict(norm=norm, eps=eps, eta0=eta0, first=case == "first", last=case == "last", ckpt_len=ckpt)
        ref = A.step(a["x"], a["x_prev"], a["x0"], a["g"], a["x_best"], a["g_best"], a["x_adv"], f, hit, st, clip=clip, n_valid=nv, **kw)
        got, gst = _run_step(a, f, hit, st, nv, offset, clip_values=clip, **kw)
        what = f"n {n} rows {rows} norm {norm} {case} clip {clip} offset {offset} n_valid {None if nv is None else nv.tolist()}"
        for k in A.STATE:
            assert gst[k].tobytes() == ref["state"][k].tobytes(), f"{what}: state {k}: {gst[k]} != {ref['state'][k]}"
        for k in ("x_best", "g_best", "x_adv"):
            assert got[k].tobytes() == ref[k].tobytes(), f"{what}: {k}"
        assert got["x0"].tobytes() == a["x0"].tobytes() and got["g"].tobytes() == a["g"].tobytes()
        moved = ref["moved"]
        if case in ("halve-1",):
            assert ref["restart"][moved].all(), what
        if case == "halve-2":
            assert ref["restart"][moved & (np.arange(rows) != 1)].all() and not (rows > 1 and ref["restart"][1]), what
        if case in ("keep", "plain", "first", "last"):
            assert not ref["restart"].any(), what
        if not moved.any():
            assert got["x"].tobytes() == a["x"].tobytes() and got["x_prev"].tobytes() == a["x_prev"].tobytes(), f"{what}: x moved"
        else:
            keep = ~moved
            assert got["x"][keep].tobytes() == a["x"][keep].tobytes() and got["x_prev"][keep].tobytes() == a["x_prev"][keep].tobytes(), what
            assert got["x_prev"][moved].tobytes() == ref["x_prev"][moved].astype(np.float32).tobytes(), f"{what}: x_prev"
            eta = ref["state"]["eta"].astype(np.float64).max()
            tol = float(np.spacing(np.float32(np.abs(a["x0"]).max() + 2 * eta)))
            if norm == 2.0:
                tol += 1e-6 * (5 * eta + 3 * eps)
            err = np.abs(got["x"][moved].astype(np.float64) - ref["x"][moved]).max()
            assert err <= tol, f"{what}: x off by {err:.3e}, bound {tol:.3e}"
            nvv = np.full(rows, n) if nv is None else np.clip(nv, 0, n)
            pad = (np.arange(n)[None, :] >= nvv[:, None]) & moved[:, None]
            assert got["x"][pad].tobytes() == a["x0"][pad].tobytes() and got["x_prev"][pad].tobytes() == a["x0"][pad].tobytes(), f"{what}: padding"
            inside = ~pad & moved[:, None]
            assert A.within_ball(np.where(inside, got["x"], a["x0"]), a["x0"], eps, norm), f"{what}: outside the ball"
        again, ast = _run_step(a, f, hit, st, nv, offset, clip_values=clip, **kw)
        assert all(again[k].tobytes() == got[k].tobytes() for k in got) and all(ast[k].tobytes() == gst[k].tobytes() for k in gst), f"{what}: two runs"
        if offset == 0:  # the other alignment: the same bits
            other, ost = _run_step(a, f, hit, st, nv, 1, clip_values=clip, **kw)
            assert all(other[k].tobytes() == got[k].tobytes() for k in got) and all(ost[k].tobytes() == gst[k].tobytes() for k in gst), f"{what}: alignment"
        checked[case] += 1
    assert all(v == 6 for v in checked.values())


def test_step_refuses_bad_arguments_and_overlap(cuda):
    from lipasr.apgd import apgd_state, apgd_step

    rows, n = 3, 16
    buf = torch.zeros(8 * rows * n, device="cuda")
    arr = [buf[k * rows * n:(k + 1) * rows * n].view(rows, n) for k in range(7)]
    f, hit, st = torch.zeros(rows, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda"), apgd_state(rows, "cuda")
    kw = dict(norm=math.inf, eps=0.1, eta0=0.2, first=True)
    apgd_step(*arr, f, hit, st, **kw)
    for bad in (dict(norm=1), dict(norm=3.0), dict(eps=-0.1), dict(eps=math.inf), dict(clip_values=(1.0, -1.0)), dict(ckpt_len=3),
                dict(momentum=2.0), dict(n_valid=torch.zeros(rows, device="cuda"))):
        with pytest.raises(ValueError):
            apgd_step(*arr, f, hit, st, **dict(kw, **bad))
    with pytest.raises(ValueError, match="overlaps"):
        apgd_step(arr[0], buf[1:1 + rows * n].view(rows, n), *arr[2:], f, hit, st, **kw)
    with pytest.raises(ValueError, match="overlaps"):
        apgd_step(*arr[:4], arr[0], *arr[5:], f, hit, st, **kw)
    with pytest.raises(ValueError, match="overlaps"):
        apgd_step(*arr, f, hit, dict(st, f_prev=st["f_best"]), **kw)
    with pytest.raises(ValueError):
        apgd_step(arr[0].t(), *arr[1:], f, hit, st, **kw)
    with pytest.raises(ValueError):
        apgd_step(*arr, f, hit, {k: v for k, v in st.items() if k != "eta"}, **kw)
    empty = [t[:0] for t in arr]
    assert apgd_step(*empty, f[:0], hit[:0], apgd_state(0, "cuda"), **kw).shape == (0, n)


# =================================================================================================
# 3. the class against the hand-built chain, and across chunks
# =================================================================================================
@pytest.mark.parametrize("loss_name", sorted(LOSSES))
@pytest.mark.parametrize("norm", [np.inf, 2])
def test_generate_equals_the_hand_built_chain(small, loss_name, norm):
    from lipasr.apgd import apgd_checkpoints, apgd_loss, apgd_state, apgd_step
    from lipasr.attacks import AutoProjectedGradientDescent, TensorFlowV2Classifier

    clf, xt = small["clf"], dev(small["x"])
    eps = 0.3 if norm == np.inf else 1.0
    atk = AutoProjectedGradientDescent(clf, norm=norm, eps=eps, max_iter=10, nb_random_init=0, loss_type=loss_name)
    adv = atk.generate_device(xt)
    labels = clf.predict_device(xt, logits=True).argmax(dim=1).to(torch.int32)
    x, x_prev, x_best, g_best, x_adv = xt.clone(), xt.clone(), xt.clone(), torch.zeros_like(xt), xt.clone()
    st, ck, prev = apgd_state(5, "cuda"), {}, 0
    for w in apgd_checkpoints(10):
        ck[w], prev = w - prev, w
    assert ck == {3: 3, 5: 2, 6: 1, 7: 1, 8: 1, 9: 1}
    kw = dict(norm=float(norm), eps=eps, eta0=2 * eps)
    for k in range(10):
        f, dz, hit = apgd_loss(clf.predict_device(x, logits=True), labels, loss_name)
        g = clf.output_vjp_device(x, dz, on_logits=True)
        apgd_step(x, x_prev, xt, g, x_best, g_best, x_adv, f, hit, st, first=k == 0, ckpt_len=ck.get(k, 0), **kw)
    f, dz, hit = apgd_loss(clf.predict_device(x, logits=True), labels, loss_name)
    apgd_step(x, x_prev, xt, g, x_best, g_best, x_adv, f, hit, st, last=True, **kw)
    fooled = st["fooled"] != 0
    want = torch.where(fooled[:, None], x_adv, x_best)
    assert adv.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() and adv.data_ptr() != xt.data_ptr()
    assert torch.equal(atk.success_, fooled) and atk.success_.dtype == torch.bool
    assert atk.loss_.cpu().numpy().tobytes() == st["f_best"].cpu().numpy().tobytes() and atk.loss_.dtype == torch.float32
    assert torch.equal(atk.halvings_, st["halvings"]) and atk.halvings_.dtype == torch.int32
    assert A.within_ball(adv.cpu().numpy(), small["x"], eps, norm)
    print(f"{loss_name} norm {norm}: success {atk.success_.tolist()} halvings {atk.halvings_.tolist()}")
    # labels given as one-hot or as indices are the labels found above; NumPy in, NumPy out
    lab = labels.cpu().numpy()
    for y in (None, np.eye(5, dtype=np.float32)[lab], lab):
        assert atk.generate(small["x"], y).tobytes() == want.cpu().numpy().tobytes()

    # the results do not depend on the chunks: five rows at once against chunks of two
    class Limited(TensorFlowV2Classifier):
        batch_limit = 2

    lim = Limited(model=small["model"], nb_classes=5, input_shape=(36,))
    parts = AutoProjectedGradientDescent(lim, norm=norm, eps=eps, max_iter=10, nb_random_init=0, loss_type=loss_name)
    assert parts.generate_device(xt).cpu().numpy().tobytes() == adv.cpu().numpy().tobytes()
    assert torch.equal(parts.success_, atk.success_) and torch.equal(parts.halvings_, atk.halvings_)
    assert parts.loss_.cpu().numpy().tobytes() == atk.loss_.cpu().numpy().tobytes()


def test_constructor_and_call_checks(small):
    from lipasr.attacks import AutoProjectedGradientDescent

    clf, xt = small["clf"], dev(small["x"])
    for bad in (dict(norm=1), dict(norm=3), dict(eps=-0.1), dict(eps=math.inf), dict(max_iter=0), dict(nb_random_init=-1), dict(batch_size=0),
                dict(loss_type="hinge"), dict(loss_type="difference_logits_ratio", targeted=True), dict(clip_values=(1.0, -1.0))):
        with pytest.raises(ValueError):
            AutoProjectedGradientDescent(clf, **bad)
    with pytest.raises(TypeError):
        AutoProjectedGradientDescent(small["model"])
    m2 = build_model([P.LayerSpec(36, 2, False, 0.0, False)])
    from lipasr.attacks import TensorFlowV2Classifier
    with pytest.raises(ValueError, match="3 classes"):
        AutoProjectedGradientDescent(TensorFlowV2Classifier(model=m2, nb_classes=2, input_shape=(36,)), loss_type="difference_logits_ratio")
    atk = AutoProjectedGradientDescent(clf, eps=0.1, max_iter=2)
    assert atk.eps_step == 0.2 and atk.clip_values is None and atk.nb_random_init == 5
    with pytest.raises(ValueError):
        AutoProjectedGradientDescent(clf, eps=0.1, targeted=True).generate_device(xt)
    with pytest.raises(ValueError):
        atk.generate_device(xt, lengths=[36] * 5)
    with pytest.raises(ValueError):
        atk.generate_device(xt[:, :35])
    assert atk.generate_device(xt[:0]).shape == (0, 36)
    # targeted: where it succeeds it lands on the target
    target = (clf.predict_device(xt, logits=True).argmax(dim=1) + 1) % 5
    tgt = AutoProjectedGradientDescent(clf, eps=1.0, max_iter=10, targeted=True, nb_random_init=2)
    adv = tgt.generate_device(xt, target)
    assert torch.equal(clf.predict_device(adv, logits=True).argmax(dim=1) == target, tgt.success_)


# =================================================================================================
# 4. the linear known answers
# =================================================================================================
@pytest.mark.parametrize("norm", ["inf", "2"])
def test_linear_known_answer_on_the_device(cuda, norm):
    """tests/test_apgd_cpu.py::test_known_answer_on_a_linear_classifier through a one-layer Model."""
    from lipasr.attacks import AutoProjectedGradientDescent, TensorFlowV2Classifier

    spec, p, x, cls, w, d_inf, d2 = linear_model()
    m = build_model(spec)
    load_params(m, p)
    clf = TensorFlowV2Classifier(model=m, nb_classes=2, input_shape=(880,))
    np.testing.assert_array_equal(clf.predict(x).argmax(axis=1), cls)
    d = d_inf if norm == "inf" else d2
    for factor, pick, want_success in ((0.9, d.min(), False), (1.1, d.max(), True)):
        eps = factor * pick
        atk = AutoProjectedGradientDescent(clf, norm=np.inf if norm == "inf" else 2, eps=eps, max_iter=20, nb_random_init=0)
        adv = atk.generate(x)
        if norm == "inf":
            want = np.float32(x) + np.float32(eps) * np.sign(w).astype(np.float32)
            assert adv.tobytes() == want.tobytes(), f"{int((adv != want).sum())} elements differ"
        else:
            want = x.astype(np.float64) + float(np.float32(eps)) * w / np.linalg.norm(w, axis=1, keepdims=True)
            err = np.abs(adv.astype(np.float64) - want).max()
            print(f"norm 2, eps {eps:.4f}: max |adv - (x0 + eps w/|w|)| = {err:.3e} (bound {1e-6 * eps:.3e})")
            assert err <= 1e-6 * eps
        assert (atk.success_.cpu().numpy() == want_success).all() and (atk.halvings_ > 0).all()
        assert ((clf.predict(adv).argmax(axis=1) != cls) == want_success).all()


# =================================================================================================
# 5. a real model against the oracle's run
# =================================================================================================
@pytest.fixture(scope="module")
def real_model(cuda):
    from lipasr.attacks import TensorFlowV2Classifier

    spec = P.vd_unconstrained_spec()
    m = build_model(spec)
    load_params(m, R.setup_params(spec, REAL["param_seed"]))
    return TensorFlowV2Classifier(model=m, nb_classes=10, input_shape=(880,))


@pytest.mark.parametrize("name", sorted(REAL_CASES))
def test_real_model_against_the_oracle(real_model, name):
    from lipasr.apgd import apgd_loss
    from lipasr.attacks import AutoProjectedGradientDescent

    clf, case = real_model, REAL_CASES[name]
    spec, p, x, own = real_case(name)
    ref = real_oracle(name)
    assert ref["ambiguous"].sum() <= REAL["rows"] // 4  # tests/test_apgd_cpu.py asserts it too: the cap on the rows left out below
    np.testing.assert_array_equal(clf.predict(x).argmax(axis=1), own)
    norm, eps, clip = (np.inf if case["norm"] == "inf" else 2), case["eps"], REAL["clip"]
    kw = dict(norm=norm, eps=eps, max_iter=REAL["max_iter"], loss_type=case["loss"], clip_values=clip)
    atk = AutoProjectedGradientDescent(clf, nb_random_init=0, **kw)
    adv = atk.generate(x)
    ok, loss_, halv = atk.success_.cpu().numpy(), atk.loss_.cpu().numpy(), atk.halvings_.cpu().numpy()
    assert A.within_ball(adv, x, eps, norm) and adv.min() >= np.float32(clip[0]) and adv.max() <= np.float32(clip[1])
    np.testing.assert_array_equal(ok, clf.predict(adv).argmax(axis=1) != own)
    f0 = apgd_loss(clf.predict_device(dev(x), logits=True), torch.as_tensor(own.astype(np.int32)).cuda(), case["loss"])[0].cpu().numpy()
    assert (loss_ >= f0).all()
    clear = ~ref["ambiguous"]
    err = np.abs(adv.astype(np.float64) - ref["adv"].astype(np.float64)).max(axis=1)
    print(f"{name}: success {ok.tolist()} (oracle {ref['success'].tolist()}), halvings {halv.tolist()} (oracle {ref['halvings'].tolist()}), "
          f"ambiguous {ref['ambiguous'].tolist()}, max |adv - oracle| per row / eps {['%.1e' % (e / eps) for e in err]}")
    assert (err[clear] <= 1e-3 * eps).all()
    np.testing.assert_array_equal(halv[clear], ref["halvings"][clear])
    np.testing.assert_array_equal(ok[clear], ref["success"][clear])
    # restarts never un-fool a row: restart 0 of two is the run of one (the draws are keyed by the restart)
    one = AutoProjectedGradientDescent(clf, nb_random_init=1, seed=7, **kw)
    adv1 = one.generate(x)
    two = AutoProjectedGradientDescent(clf, nb_random_init=2, seed=7, **kw)
    adv2 = two.generate(x)
    ok1, ok2 = one.success_.cpu().numpy(), two.success_.cpu().numpy()
    assert (ok2 >= ok1).all() and adv2[ok1].tobytes() == adv1[ok1].tobytes()
    assert (two.loss_.cpu().numpy()[~ok2] >= one.loss_.cpu().numpy()[~ok2]).all()
    assert A.within_ball(adv2, x, eps, norm) and adv2.min() >= np.float32(clip[0]) and adv2.max() <= np.float32(clip[1])
    np.testing.assert_array_equal(ok2, clf.predict(adv2).argmax(axis=1) != own)


# =================================================================================================
# 6. audio with lengths
# =================================================================================================
@pytest.mark.parametrize("norm,eps", [(np.inf, 0.02), (2, 0.5)])
def test_attack_over_audio_with_lengths(audio, norm, eps):
    from lipasr.attacks import AutoProjectedGradientDescent

    clf, rows, lt = audio["clf"], audio["rows"], audio["lt"]
    x = rows.cpu().numpy()
    assert x.shape == (3, 22050)
    pos = [int(math.ceil(n * 22050.0 / 16000.0)) for n in RAGGED]
    valid = np.arange(22050)[None, :] < np.array(pos)[:, None]
    own = clf.predict_device(rows, lengths=lt).argmax(dim=1).cpu().numpy()
    atk = AutoProjectedGradientDescent(clf, norm=norm, eps=eps, max_iter=5, nb_random_init=2, seed=3)
    assert atk.clip_values == (-1.0, 1.0)  # the estimator's
    adv = atk.generate_device(rows, lengths=lt).cpu().numpy()
    assert adv[~valid].tobytes() == x[~valid].tobytes(), "padding moved"
    assert A.within_ball(adv, x, eps, norm, valid) and adv[valid].min() >= -1.0 and adv[valid].max() <= 1.0
    pred = clf.predict_device(torch.as_tensor(adv).cuda(), logits=True, lengths=lt).argmax(dim=1).cpu().numpy()
    ok = atk.success_.cpu().numpy()
    print(f"audio 3 x 22050 with lengths, norm {norm}, eps {eps}: success {ok.tolist()}, halvings {atk.halvings_.tolist()}, loss {atk.loss_.tolist()}")
    np.testing.assert_array_equal(ok, pred != own)
    assert (np.abs(adv - x)[valid] > 0).mean() > 0.1  # the clips did move


# =================================================================================================
# 7. the menu
# =================================================================================================
def test_menu_runs_the_apgd_sweep(cuda, tmp_path, capsys):
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
    base = ["--path", str(data) + "/", "--noise-dir", str(noise), "--constrained", h5, "--unconstrained", h5, "--attack", "white", "--kind",
            "apgd", "--points", "1", "--max-iter", "3"]
    capsys.readouterr()
    for extra in ([], ["--loss", "dlr", "--norm", "2"]):
        grid, acc = V.main(base + extra)
        out = capsys.readouterr().out
        assert len(grid) == 1 and np.isclose(grid[0], 1.0) and set(acc) == {"constrained", "unconstrained"}
        assert all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
        assert "Accuracy on adversarial test examples: " in out and "Accuracy on adversarial test examples unconstrained: " in out
    grid, acc = V.main(base + ["--over", "audio"])
    out = capsys.readouterr().out
    assert grid == V.AUDIO_SIGMAS[:1] and all(len(v) == 1 and 0.0 <= v[0] <= 1.0 for v in acc.values())
    assert "Accuracy on adversarial audio test examples unconstrained" in out
    # the audio grid starts at 0, where nothing is attacked: a second point runs the attack itself
    grid, acc = V.main(base[:-3] + ["2", "--max-iter", "3", "--over", "audio"])
    out = capsys.readouterr().out
    assert grid == V.AUDIO_SIGMAS[:2] and all(len(v) == 2 and 0.0 <= a <= 1.0 for v in acc.values() for a in v)
    assert "Accuracy on adversarial audio test examples unconstrained" in out
    with pytest.raises(ValueError):
        V.main(base + ["--norm", "1"])
