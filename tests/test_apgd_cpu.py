"""Auto-PGD without a GPU: the ABI and the bindings, the checkpoint schedule, the selector's boundaries, and the float64 oracle of
tests/apgd_ref.py held to what is known -- its gradient against central differences, the maximiser of the cross-entropy on the ball
of a linear classifier, the monotonicity of the best loss -- and the choice of the real-model fixtures of tests/test_apgd_gpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

import apgd_ref as A
import genetic_ref as G
import lp_attacks_ref as LP
import local_lip_ref as R
from oracle import mlp_ref as P

# the selector of lipasr_apgd_step: the last width of every instance (include/lipasr.h, lipasr_debug_apgd_path)
BOUNDARIES = [256, 512, 1024, 2048, 8192, 16384, 22528]

# the real-model fixtures of tests/test_apgd_gpu.py: the unconstrained 880 -> 10 model of the genetic tests (parameter seed 3), 8 rows
# clipped to [-2, 2], 20 iterations, no random start.  The data seeds and radii were picked on the ORACLE alone, out of seeds 3 .. 14
# and three radii per norm, as the first whose run has at most two ambiguous rows (test_real_model_fixture_has_few_ambiguous_rows):
# a loss that has converged moves by less than 1e-4 relative per iteration, and a DLR loss saturates at exactly 1 once the label
# is third, so most candidates have more.
REAL = dict(param_seed=3, rows=8, max_iter=20, clip=(-2.0, 2.0))
REAL_CASES = {"ce-inf": dict(loss="cross_entropy", norm="inf", x_seed=4, eps=0.05),
              "dlr-inf": dict(loss="difference_logits_ratio", norm="inf", x_seed=5, eps=0.02),
              "dlr-2": dict(loss="difference_logits_ratio", norm="2", x_seed=10, eps=1.0)}
LOSSES = {"cross_entropy": 0, "difference_logits_ratio": 1}


def real_case(name):
    spec = P.vd_unconstrained_spec()
    p = R.setup_params(spec, REAL["param_seed"])
    x = np.clip(np.random.default_rng(REAL_CASES[name]["x_seed"]).standard_normal((REAL["rows"], 880)), *REAL["clip"]).astype(np.float32)
    own = P.forward_infer(spec, p.astype(np.float64), x.astype(np.float64), return_logits=True).argmax(axis=1)
    return spec, p, x, own


_real_runs = {}


def real_oracle(name):
    """The oracle's run of one real-model fixture, computed once and shared."""
    if name not in _real_runs:
        spec, p, x, own = real_case(name)
        c = REAL_CASES[name]
        _real_runs[name] = A.attack(spec, p, x, own, c["eps"], norm=np.inf if c["norm"] == "inf" else 2, max_iter=REAL["max_iter"],
                                    loss_type=LOSSES[c["loss"]], clip=REAL["clip"])
    return _real_runs[name]


def linear_model():
    W, bias, x, d, cls = G.linear_case_inf()
    spec = [P.LayerSpec(880, 2, False, 0.0, False)]
    p = P.Params(W=[W], b=[bias], gamma=[None], beta=[None], mov_mean=[None], mov_var=[None])
    w = W[:, 1 - cls].T.astype(np.float64) - W[:, cls].T.astype(np.float64)  # [6, 880]: w_o - w_y per row
    c = (bias[1 - cls] - bias[cls]).astype(np.float64)
    d2 = np.abs((x.astype(np.float64) * w).sum(axis=1) + c) / np.linalg.norm(w, axis=1)
    return spec, p, x, cls, w, d, d2


# =================================================================================================
# ABI and bindings
# =================================================================================================
def test_abi_and_bindings():
    import lipasr._native as N

    assert N.lib.lipasr_version() >= 650
    for s in ("lipasr_apgd_loss", "lipasr_apgd_step", "lipasr_debug_apgd_path"):
        assert s in N.PROTOTYPES and N.has(s) and hasattr(N.lib, s)
        assert getattr(N.lib, s).argtypes == N.PROTOTYPES[s][1]


def _step_args(**kw):
    a = dict(h=C.c_void_p(8), arrays=[C.c_void_p(4096 * (i + 1)) for i in range(18)], rows=2, n=16, norm=math.inf, eps=0.1, eta0=0.2,
             lo=-math.inf, hi=math.inf, momentum=0.75, rho=0.75, flags=0, ckpt_len=0)
    a.update(kw)
    return (a["h"], *a["arrays"], a["rows"], a["n"], a["norm"], a["eps"], a["eta0"], a["lo"], a["hi"], a["momentum"], a["rho"], a["flags"],
            a["ckpt_len"], None)


def test_refusals_without_a_device():
    """Every refusal below happens before a pointer is followed or a device is touched: the pointers are made up."""
    import lipasr._native as N

    h, q = C.c_void_p(8), C.c_void_p(4096)
    loss = N.lib.lipasr_apgd_loss
    assert loss(h, None, q, 2, 10, 0, 0, q, q, q, None) == N.EINVAL and "null pointer" in N.last_error()
    assert loss(h, q, q, 2, 10, 0, 0, q, None, q, None) == N.EINVAL and "null pointer" in N.last_error()
    assert loss(None, q, q, 2, 10, 0, 0, q, q, q, None) == N.EINVAL and "null handle" in N.last_error()
    assert loss(h, q, q, 2, 10, 1, 1, q, q, q, None) == N.EINVAL and "untargeted" in N.last_error()
    assert loss(h, q, q, 2, 2, 1, 0, q, q, q, None) == N.EINVAL and "at least 3 classes" in N.last_error()
    assert loss(h, q, q, 2, 33, 0, 0, q, q, q, None) == N.EINVAL and loss(h, q, q, 2, 0, 0, 0, q, q, q, None) == N.EINVAL
    assert loss(h, q, q, 2, 10, 2, 0, q, q, q, None) == N.EINVAL and "loss_type" in N.last_error()
    assert loss(h, None, None, 0, 10, 0, 0, None, None, None, None) == N.OK  # batch == 0
    step = N.lib.lipasr_apgd_step
    for norm in (1.0, 3.0, -math.inf, math.nan):
        assert step(*_step_args(norm=norm)) == N.EINVAL and "norm" in N.last_error()
    for i in range(18):
        arrays = [C.c_void_p(4096 * (k + 1)) for k in range(18)]
        if i == 9:  # n_valid may be NULL: the call would go on to the device, so it is not made here
            continue
        arrays[i] = None
        rc = step(*_step_args(arrays=arrays))
        assert rc == N.EINVAL and "null pointer" in N.last_error(), i
    assert step(*_step_args(h=None)) == N.EINVAL and "null handle" in N.last_error()
    for bad in (dict(eps=-1.0), dict(eps=math.inf), dict(lo=1.0, hi=-1.0), dict(flags=4), dict(flags=1, ckpt_len=3), dict(ckpt_len=-1),
                dict(momentum=1.5), dict(rows=-1)):
        assert step(*_step_args(**bad)) == N.EINVAL, bad
    arrays = [C.c_void_p(4096 * (k + 1)) for k in range(18)]
    arrays[4] = C.c_void_p(4096 + 64)  # x_best inside x
    assert step(*_step_args(arrays=arrays)) == N.EINVAL and "overlaps" in N.last_error()
    assert step(*_step_args(arrays=[None] * 18, rows=0)) == N.OK and step(*_step_args(arrays=[None] * 18, n=0)) == N.OK


def test_step_names_the_arrays_that_overlap():
    """A written array that shares a byte with any other is refused by name, the earlier argument first; made-up pointers."""
    import lipasr._native as N

    step = N.lib.lipasr_apgd_step
    names = ["x", "x_prev", "x0", "g", "x_best", "g_best", "x_adv", "f", "hit", "n_valid", "eta", "f_best", "f_prev", "f_best_ckpt",
             "improved", "reduced_last", "fooled", "halvings"]
    row_bytes, state_bytes = 2 * 16 * 4, 2 * 4
    for i, j, shift in ((0, 4, 64), (0, 1, row_bytes - 4), (2, 6, 0), (3, 5, -4), (7, 10, 4), (9, 10, 0), (11, 12, 0), (8, 17, state_bytes - 4)):
        arrays = [C.c_void_p(4096 * (k + 1)) for k in range(18)]
        arrays[j] = C.c_void_p(4096 * (i + 1) + shift)
        assert step(*_step_args(arrays=arrays)) == N.EINVAL
        assert N.last_error() == f"lipasr_apgd_step: {names[i]} overlaps {names[j]}", (i, j, N.last_error())


def test_checkpoints():
    from lipasr.apgd import apgd_checkpoints

    assert apgd_checkpoints(100) == [22, 41, 57, 70, 80, 87, 93, 99]
    assert apgd_checkpoints(10) == [3, 5, 6, 7, 8, 9]
    for m in (1, 2, 10, 100, 1000):
        got = apgd_checkpoints(m)
        assert got == A.checkpoints(m) and got == sorted(set(got)) and all(1 <= w <= m - 1 for w in got)
    assert apgd_checkpoints(1) == [] and apgd_checkpoints(2) == [1]
    assert apgd_checkpoints(1000) == [220, 410, 570, 700, 800, 870, 930, 990]
    with pytest.raises(ValueError):
        apgd_checkpoints(0)


def test_selector_boundaries():
    import lipasr._native as N
    from lipasr.apgd import apgd_path

    path = N.lib.lipasr_debug_apgd_path
    assert path(0, 1) == -1 and path(-3, 0) == -1
    for inst, last in enumerate(BOUNDARIES):
        assert apgd_path(last)[0] == inst and apgd_path(last + 1)[0] == inst + 1, last
        assert apgd_path(last, aligned=False) == (inst, False) and apgd_path(last, aligned=True) == (inst, True)  # every boundary is a multiple of 4
    assert apgd_path(1) == (0, False) and apgd_path(1 << 30)[0] == 7
    # the project's rows: 880 and 2 020 features in a wavefront, 16 000 and 22 050 samples in a workgroup
    assert [apgd_path(n)[0] for n in (880, 2020, 16000, 22050)] == [2, 3, 5, 6]
    assert apgd_path(22050) == (6, False) and apgd_path(880) == (2, True) and apgd_path(880, aligned=False) == (2, False)


# =================================================================================================
# the oracle
# =================================================================================================
@pytest.mark.parametrize("loss_type,targeted", [(0, False), (0, True), (1, False)])
def test_oracle_gradient_against_central_differences(loss_type, targeted):
    rng = np.random.default_rng(5 + loss_type)
    for C_ in (3, 4, 10, 32):
        z = (2.0 * rng.standard_normal((64, C_))).astype(np.float32)
        srt = np.sort(z, axis=1)[:, ::-1][:, :5]
        # away from ties: the five largest 0.02 apart (the DLR loss is not differentiable where their order changes) and its
        # denominator z_pi1 - z_pi3 above 0.5, so that the third derivative ~ N / D^4 keeps the difference quotient honest
        z = z[((-np.diff(srt, axis=1)).min(axis=1) > 0.02) & (srt[:, 0] - srt[:, 2] > 0.5)]
        assert len(z) >= 8
        labels = rng.integers(0, C_, len(z))
        L = A.loss(z, labels, loss_type, targeted)
        h = 2.0 ** -13  # exact in float32 next to |z| < 16
        for c in range(C_):
            e = np.zeros_like(z)
            e[:, c] = h
            fd = (A.loss(z + e, labels, loss_type, targeted)["f"] - A.loss(z - e, labels, loss_type, targeted)["f"]) / (2 * h)
            np.testing.assert_allclose(L["dz"][:, c], fd, rtol=0, atol=2e-5 * max(1.0, np.abs(L["dz"]).max()))
    # the conventions at the edges: hit, the NaN row, a label outside the classes
    z = np.array([[1.0, 1.0, 0.0], [0.0, np.nan, 1.0], [3.0, 2.0, 1.0], [3.0, 2.0, 1.0]], dtype=np.float32)
    L = A.loss(z, [1, 0, 0, 3], 0, False)
    assert L["hit"].tolist() == [1, 0, 0, 0] and L["bad"].tolist() == [False, True, False, True]
    assert np.isnan(L["f"][[1, 3]]).all() and not L["dz"][[1, 3]].any()


@pytest.mark.parametrize("norm", ["inf", "2"])
def test_known_answer_on_a_linear_classifier(norm):
    """One linear layer, two classes, cross-entropy, no clipping: the maximiser of the loss on the ball is x0 + eps sign(w_o - w_y)
    (norm inf) or x0 + eps w / ||w||_2 (norm 2), and Auto-PGD is there after its first step (eta = 2 eps) and stays."""
    spec, p, x, cls, w, d_inf, d2 = linear_model()
    d = d_inf if norm == "inf" else d2
    nrm = np.inf if norm == "inf" else 2
    for factor, pick, want_success in ((0.9, d.min(), False), (1.1, d.max(), True)):
        eps = factor * pick
        if norm == "inf":
            want = np.float32(x) + np.float32(eps) * np.sign(w).astype(np.float32)
        else:
            want = x.astype(np.float64) + float(np.float32(eps)) * w / np.linalg.norm(w, axis=1, keepdims=True)
        for iters in (1, 2, 20):
            r = A.attack(spec, p, x, cls, eps, norm=nrm, max_iter=iters)
            if norm == "inf":
                assert r["adv"].tobytes() == want.tobytes(), (factor, iters)
            else:
                err = np.abs(r["adv"].astype(np.float64) - want).max()
                print(f"norm 2, eps {eps:.4f}, {iters} iterations: max |adv - (x0 + eps w/|w|)| = {err:.3e} (bound {1e-6 * eps:.3e})")
                assert err <= 1e-6 * eps
            assert (r["success"] == want_success).all(), (factor, iters, r["success"])
        assert (r["halvings"] > 0).all()
        assert (r["loss"] >= r["f_start"]).all()


@pytest.mark.parametrize("loss_name", sorted(LOSSES))
@pytest.mark.parametrize("norm", ["inf", "2"])
def test_monotone_and_inside_on_a_small_model(loss_name, norm):
    """f_best only ever grows from f(x_start) (a theorem of the bookkeeping), and the result lies in the ball and the clip range."""
    spec = [P.LayerSpec(36, 16, True, 0.0, False), P.LayerSpec(16, 5, False, 0.0, False)]
    p = R.setup_params(spec, 2)
    clip = (-1.5, 1.5)
    x = np.clip(np.random.default_rng(4).standard_normal((12, 36)), *clip).astype(np.float32)
    own = P.forward_infer(spec, p.astype(np.float64), x.astype(np.float64), return_logits=True).argmax(axis=1)
    eps = 0.2 if norm == "inf" else 0.8
    nrm = np.inf if norm == "inf" else 2
    r = A.attack(spec, p, x, own, eps, norm=nrm, max_iter=25, loss_type=LOSSES[loss_name], clip=clip)
    assert (r["loss"].astype(np.float64) >= r["f_start"].astype(np.float32)).all()
    assert A.within_ball(r["adv"], x, eps, nrm) and r["adv"].min() >= clip[0] and r["adv"].max() <= clip[1]
    again = P.forward_infer(spec, p.astype(np.float64), r["adv"].astype(np.float64), return_logits=True).argmax(axis=1)
    assert ((again != own) == r["success"]).all()
    # printed, not asserted: rows fooled against fixed-step PGD at the same budget
    onehot = np.eye(5)[own]
    pgd = LP.pgd(spec, p.astype(np.float64), x, eps, eps_step=eps / 4, max_iter=25, norm=nrm, y=onehot)
    pgd = np.clip(pgd, *clip)
    pgd_ok = P.forward_infer(spec, p.astype(np.float64), pgd, return_logits=True).argmax(axis=1) != own
    print(f"{loss_name}, norm {norm}, eps {eps}: Auto-PGD fooled {int(r['success'].sum())} of 12 rows, PGD (eps_step eps/4) {int(pgd_ok.sum())}; "
          f"halvings {r['halvings'].tolist()}")


@pytest.mark.parametrize("name", sorted(REAL_CASES))
def test_real_model_fixture_has_few_ambiguous_rows(name):
    """The cap on the rows tests/test_apgd_gpu.py may leave out of its comparison with the oracle: at most a quarter of the rows of
    each fixture make a comparison closer than 1e-4 relative."""
    r = real_oracle(name)
    closest = [min((abs(a - b) / max(abs(a), abs(b), 1e-300) for a, b in rec if np.isfinite(a) and np.isfinite(b)), default=np.inf)
               for rec in r["comparisons"]]
    print(f"{name}: ambiguous {r['ambiguous'].tolist()}, closest comparison per row {['%.1e' % c for c in closest]}, "
          f"success {r['success'].tolist()}, halvings {r['halvings'].tolist()}")
    assert r["ambiguous"].sum() <= REAL["rows"] // 4
