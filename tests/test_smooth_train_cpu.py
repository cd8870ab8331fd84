"""CPU suite of training for randomized smoothing (lipasr_version 770): the ABI, Phi^-1, the float64 restatement against central
differences of its own loss, and the host twin lipasr_smooth_loss_host against the restatement (tests/smooth_loss_ref.py)."""
import os
import re
from statistics import NormalDist

import numpy as np
import pytest

import lipasr._native as N
import smooth_loss_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lipasr_mlp_train_fwd", "lipasr_mlp_train_bwd", "lipasr_smooth_loss", "lipasr_smooth_loss_host", "lipasr_smooth_probit_host",
         "lipasr_debug_smooth_loss_launches")
# (clips, draws, classes) and the logit scales of the issue; every case is run at every scale
SHAPES = ((1, 1, 2), (4, 7, 3), (3, 16, 10), (5, 64, 32), (2, 16, 1))
SCALES = (0.1, 3.0, 40.0)
SIGMA, LAM, GAMMA, BETA = 0.5, 12.0, 8.0, 16.0
EPS22 = 2.0 ** -22


def case(shape, zscale, seed):
    """logits N(0, 1) * zscale with the label's column raised by one zscale on half the clips (float32), labels, scale = 1 / clips"""
    clips, draws, classes = shape
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((clips, draws, classes)) * zscale
    y = rng.integers(0, classes, clips)
    for b in range(0, clips, 2):
        z[b, :, y[b]] += zscale
    return z.reshape(clips * draws, classes).astype(np.float32), y.astype(np.int32), float(np.float32(1.0 / clips))


# seeds at which the restatement finds no clip within 1e-9 of a decision (at scale 40 softmax(beta z) is one-hot and q a multiple of
# 1 / draws: most seeds tie two classes exactly there); chosen by the restatement alone, before the code under test ran
SEEDS = {((4, 7, 3), 40.0): 4102, ((5, 64, 32), 40.0): 2302}


def all_cases():
    for i, shape in enumerate(SHAPES):
        for j, zs in enumerate(SCALES):
            yield shape, zs, SEEDS.get((shape, zs), 100 * i + j)


def check_against_ref(got, ref, tag=""):
    """the issue's bounds: dz element-wise 2^-22 (|classification term| + |robust term|) (both already times scale), loss and radius
    2^-22 |ref|, correct exactly.  The 2^-24 of one fp32 rounding that the bound is built on holds for normal numbers; below 2^-126
    the store rounds to a multiple of 2^-149 (saturated softmaxes at logit scale 40 put entries of dz there, 1e-46 among them), so
    the bound has that one subnormal step as its floor."""
    bound = EPS22 * (np.abs(ref["dz_c"]) + np.abs(ref["dz_r"])) + 2.0 ** -149
    err = np.abs(got["dz"].astype(np.float64) - ref["dz"])
    assert (err <= bound).all(), (tag, float((err - bound).max()), int((err > bound).sum()))
    for k in ("loss", "radius"):
        r = ref[k]
        fin = np.isfinite(r)
        assert np.array_equal(got[k][~fin].astype(np.float64), r[~fin]), (tag, k)
        assert (np.abs(got[k][fin] - r[fin]) <= EPS22 * np.abs(r[fin])).all(), (tag, k, got[k], r)
    assert np.array_equal(got["correct"], ref["correct"].astype(np.float32)), (tag, "correct")


def test_abi_770():
    header = open(os.path.join(ROOT, "include", "lipasr.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert N.lib.lipasr_version() >= 770
    for n in NAMES:
        assert N.has(n) and hasattr(N.lib, n) and N.SINCE[n] == 770 and n in N.PROTOTYPES, n
        assert re.search(r"\b" + n + r"\s*\(", decl), n
    assert "770: training for randomized smoothing" in header
    hook = N.lib.lipasr_debug_smooth_loss_launches
    assert hook(-1) == -1 and hook(len(N.SMOOTH_LOSS_KERNELS)) == -1 and hook(1000) == -1
    assert [k for k in range(16) if hook(k) >= 0] == list(range(len(N.SMOOTH_LOSS_KERNELS)))


def test_refusals_without_a_device():
    z, y, sc = case((2, 4, 3), 1.0, 1)
    ok = dict(draws=4, sigma=SIGMA, lam=LAM, gamma=GAMMA, beta=BETA, scale=sc)
    N.smooth_loss_host(z, y, **ok)
    bad = [dict(sigma=-0.1), dict(lam=-1.0), dict(gamma=0.0), dict(beta=0.0), dict(beta=-2.0), dict(sigma=float("inf")), dict(lam=float("nan")),
           dict(gamma=float("inf")), dict(beta=float("nan")), dict(scale=float("inf")), dict(scale=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError, match="lipasr_smooth_loss_host"):
            N.smooth_loss_host(z, y, **{**ok, **kw})
    vp = lambda a: a.ctypes.data_as(N.C.c_void_p)
    out = np.zeros(64, dtype=np.float32)
    for clips, draws, classes in ((1, 1, 0), (1, 1, 33), (1, 0, 3), (1, 65, 3), (-1, 1, 3)):
        for fn, lead, tail in ((N.lib.lipasr_smooth_loss_host, (), ()), (N.lib.lipasr_smooth_loss, (None,), (None,))):
            # the device entry point refuses the same things before it looks at its (null) handle
            assert fn(*lead, vp(z), vp(y), clips, draws, classes, SIGMA, LAM, GAMMA, BETA, 1.0, vp(out), vp(out), None, None, *tail) == N.EINVAL
    assert N.lib.lipasr_smooth_loss(None, vp(z), vp(y), 2, 4, 3, SIGMA, LAM, GAMMA, BETA, 1.0, vp(out), vp(out), None, None, None) == N.EINVAL
    assert "null handle" in N.last_error()
    assert N.lib.lipasr_smooth_loss_host(vp(z), vp(y), 0, 4, 3, SIGMA, LAM, GAMMA, BETA, 1.0, None, None, None, None) == N.OK  # clips == 0
    assert N.lib.lipasr_smooth_loss_host(None, vp(y), 2, 4, 3, SIGMA, LAM, GAMMA, BETA, 1.0, vp(out), vp(out), None, None) == N.EINVAL
    assert N.lib.lipasr_smooth_probit_host(None, 3, None) == N.EINVAL and N.lib.lipasr_smooth_probit_host(None, -1, None) == N.EINVAL
    # the seam's entry points refuse a null plan before they touch a device
    assert N.lib.lipasr_mlp_train_fwd(None, None, None, None, 1, None, None, None) == N.EINVAL and "null plan" in N.last_error()
    assert N.lib.lipasr_mlp_train_bwd(None, None, None, None, 1, 1.0, None, None, None) == N.EINVAL and "null plan" in N.last_error()


def test_probit_against_normaldist():
    inv = NormalDist().inv_cdf
    q = np.concatenate([10.0 ** np.arange(-300, 0, 1.0), 10.0 ** -np.linspace(0.01, 16, 400), 1.0 - 10.0 ** -np.linspace(0.3, 16, 400),
                        np.linspace(0.01, 0.99, 197), [0.075, 0.925, 0.5 - 1e-9, 0.5 + 1e-9, 1e-300, 1 - 1e-16]])
    q = q[(q > 0) & (q < 1)]
    got = N.smooth_probit(q)
    want = np.array([inv(float(v)) for v in q])
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    assert N.smooth_probit([0.5])[0] == 0.0
    edge = N.smooth_probit([0.0, 1.0, -0.1, 1.1, float("nan")])
    assert edge[0] == -np.inf and edge[1] == np.inf and np.isnan(edge[2:]).all()


@pytest.mark.parametrize("shape,zscale", [((1, 1, 2), 0.1), ((4, 7, 3), 3.0), ((3, 16, 10), 1.0), ((2, 5, 4), 3.0), ((3, 4, 6), 0.1)])
def test_restatement_dz_is_the_derivative_of_its_loss(shape, zscale):
    """guards the formulas independently of the code under test: central differences (step 1e-6) of the restatement's loss in
    float64, logit scale <= 3, 1e-5 relative to the largest entry of the clip's gradient"""
    z32, y, _ = case(shape, zscale, 7)
    z = z32.astype(np.float64)
    ref = SR.smooth_loss_ref(z32, y, shape[1], SIGMA, LAM, GAMMA, BETA, 1.0)
    assert ref["margin"].min() > 2e-5  # no decision within reach of the step (q moves by at most beta h = 1.6e-5)
    h = 1e-6
    num = np.zeros_like(z)
    for i in range(z.shape[0]):
        for c in range(z.shape[1]):
            zp, zm = z.copy(), z.copy()
            zp[i, c] += h
            zm[i, c] -= h
            num[i, c] = (SR.loss_only(zp, y, shape[1], SIGMA, LAM, GAMMA, BETA) - SR.loss_only(zm, y, shape[1], SIGMA, LAM, GAMMA, BETA)) / (2 * h)
    per_clip = np.abs(ref["dz"]).reshape(shape[0], -1).max(axis=1).repeat(shape[1])[:, None]
    assert (np.abs(num - ref["dz"]) <= 1e-5 * per_clip + 1e-9).all(), float(np.abs(num - ref["dz"]).max())


def test_host_twin_against_the_restatement():
    seen = {"active": 0, "top_inactive": 0, "top_not_y": 0}
    for shape, zs, seed in all_cases():
        z, y, sc = case(shape, zs, seed)
        ref = SR.smooth_loss_ref(z, y, shape[1], SIGMA, LAM, GAMMA, BETA, sc)
        assert ref["margin"].min() > 1e-9, (shape, zs, "the seed puts a clip on a decision")
        got = N.smooth_loss_host(z, y, shape[1], SIGMA, LAM, GAMMA, BETA, sc)
        check_against_ref(got, ref, (shape, zs))
        seen["active"] += int(ref["active"].sum())
        seen["top_inactive"] += int(((ref["top_is_y"] == 1) & (ref["active"] == 0)).sum())
        seen["top_not_y"] += int((ref["top_is_y"] == 0).sum())
    assert all(v > 0 for v in seen.values()), seen


def test_plain_cross_entropy_is_the_special_case():
    """lam = 0, draws = 1: dz = (p - y) scale and loss the row's cross-entropy; classes = 1: inactive, dz = 0, loss 0"""
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((9, 6)) * 3).astype(np.float32)
    y = rng.integers(0, 6, 9).astype(np.int32)
    sc = float(np.float32(1 / 9))
    got = N.smooth_loss_host(z, y, 1, 0.0, 0.0, GAMMA, BETA, sc)
    z64 = z.astype(np.float64)
    lse = z64.max(1) + np.log(np.exp(z64 - z64.max(1, keepdims=True)).sum(1))
    p = np.exp(z64 - lse[:, None])
    onehot = np.eye(6)[y]
    want = (p - onehot) * sc
    assert (np.abs(got["dz"] - want) <= EPS22 * np.abs(want)).all()
    ce = lse - z64[np.arange(9), y]
    assert (np.abs(got["loss"] - ce) <= EPS22 * np.abs(ce)).all()
    assert np.array_equal(got["correct"], (p.argmax(1) == y).astype(np.float32)) and not got["radius"].any()
    z1 = (rng.standard_normal((2 * 16, 1)) * 3).astype(np.float32)
    one = N.smooth_loss_host(z1, np.zeros(2, dtype=np.int32), 16, SIGMA, LAM, GAMMA, BETA, 0.5)
    assert not one["dz"].any() and not one["loss"].any() and (one["correct"] == 1).all() and np.isinf(one["radius"]).all()


def test_a_nan_poisons_its_own_clip_only():
    z, y, sc = case((4, 7, 3), 3.0, 11)
    clean = N.smooth_loss_host(z, y, 7, SIGMA, LAM, GAMMA, BETA, sc)
    zb, yb = z.copy(), y.copy()
    zb[1 * 7 + 3, 2] = np.nan
    zb[2 * 7 + 0, 0] = np.inf
    yb[3] = 3  # outside [0, classes)
    got = N.smooth_loss_host(zb, yb, 7, SIGMA, LAM, GAMMA, BETA, sc)
    assert np.array_equal(got["dz"][:7], clean["dz"][:7]) and got["loss"][0] == clean["loss"][0]
    assert got["correct"][0] == clean["correct"][0] and got["radius"][0] == clean["radius"][0]
    assert np.isnan(got["dz"][7:]).all() and np.isnan(got["loss"][1:]).all()
    assert not got["correct"][1:].any() and not got["radius"][1:].any()
    ref = SR.smooth_loss_ref(zb, yb, 7, SIGMA, LAM, GAMMA, BETA, sc)
    assert np.isnan(ref["loss"][1:]).all() and np.isfinite(ref["loss"][0])
