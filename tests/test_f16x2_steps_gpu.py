"""Arithmetic mode 2 over more than one step: the gradient scales are state, and that state against float64.

In mode 2 the scale of every dz_l is derived at run time: the forward GEMM of layer l clears the words of max |dz_l| (amax_zero), the
kernel that writes dz_l folds its maximum into them (amax_publish: bn_apply_bwd_kernel on the launch chain, the EPI_DH_BNX epilogue
with the exchange), and every GEMM that multiplies with dz_l reads them (sa_dyn / sb_dyn -> scale_from_amax).  Each tile family has
its own copy of the clear and of the read.  One step on a fresh plan cannot see a word that is not cleared (atomicMax only grows:
the scale stays too small for every later, smaller gradient) or a NaN that sticks; these tests take further steps on ONE plan.

Cases: one per implementation, from PLAN_CASES of test_gemm_instances_gpu.py at their shapes (f16x2_steps.STEP_CASES); problems,
knobs, launch counters, the float64 reference and the bounds (_fp32_bound, the same as exact fp32) are that module's.

  * swing: three steps with inv_batch = 1/B, 2^-S/B, 1/B on the same parameters, inputs and masks, no Adam step between them.
    Gradients are linear in inv_batch, so each step is held to the one oracle run, scaled; loss rows, correct rows and the moving
    statistics (k steps of the momentum recurrence) too.  Steps 1 and 3 give the same bits, the case's claimed instances ran on
    every step, no exchange gave up.  S = 27 (f16x2_steps.S): on the oracle with two-plane operands a scale left over from step 1
    puts a weight gradient of step 2 at 15 to 36 times its bound on every case's problem, where the design's scale costs 0.4 % to
    2.1 % of the bound (test_f16x2_steps_cpu.py has the figures per case).
  * recovery: a step with one input element NaN leaves every gradient non-finite where the oracle's is (everywhere: the NaN
    reaches every BatchNorm mean); a clean step after it on the same plan meets the bounds and equals the bits of the clean step
    before it.  The moving statistics are the caller's tensor, not the plan's state: they are put back around the NaN step.
  * split steps: the swing through train_fwd_bwd(defer_dw0=True) + train_dw0 (head-dw0-lds-a2 is that form already), and through
    lipasr_mlp_train_segment, every segment in order on one rank with stat_batch = batch, on the two launch-chain cases.
  * the scale is read: the swing moves the static fall-back scale (2^8 / 2^e of inv_batch) along with the gradients, so it passes a
    GEMM that ignores the maximum.  A step with gamma of the last BatchNorm layer times 2^-T (T = 19) makes every dz from there
    down 2^T times smaller at the same inv_batch; held to the float64 oracle of that problem."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gemm_instances_gpu as G
from f16x2_steps import S, SEGMENT_CASE_IDS, STEP_CASES, T, problem_key, shrunk, shrunk_reference
from helpers import load_params
from oracle import mlp_ref as P
from test_gemm_instances_gpu import _default_knobs_and_closed_models  # noqa: F401  (autouse: knobs back to default, models closed)

pytestmark = pytest.mark.gpu
_ids = [c["id"] for c in STEP_CASES]


def _step(m, spec, case, xt, yt, mt, inv_batch, form):
    """One training step in the given form -> (tensors, correct rows, counters that moved, the raw bits the step left)."""
    N = G._native()
    before = G._snapshot()
    if form == "head+dw0":
        m.train_fwd_bwd(xt, yt, inv_batch=inv_batch, masks=mt, defer_dw0=True)
        m.train_dw0(xt)
    elif form == "segments":
        batch = xt.shape[0]
        cfg = m._dropout_cfg(mt, True)
        for seg in range(m.syncbn_segments()):
            N.check(N.lib.lipasr_mlp_train_segment(m._plan, seg, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xt), N.ptr(yt), batch, inv_batch,
                                                   C.byref(cfg), N.ptr(m._grads), N.ptr(m._loss_rows), N.ptr(m._correct_rows), N.ptr(None),
                                                   N.ptr(m._part), batch, 1.0, N.stream_ptr()))
    else:
        m.train_fwd_bwd(xt, yt, inv_batch=inv_batch, masks=mt)
    errors = m.exchange_errors()  # (synchronises)
    moved = G._moved(before, G._snapshot())
    assert errors == 0, "an exchange gave up"
    batch = case["batch"]
    bits = (m._grads.clone(), m._loss_rows[:batch].clone(), m._correct_rows[:batch].clone())
    return G.step_tensors(m, spec, batch) + (moved, bits)


@functools.lru_cache(maxsize=None)
def _batch_moments(widths, bn_off, drop, batch, seed):
    """{mov_*: the batch statistic behind it}, from the reference's moving statistics after one step."""
    spec, p, *_ = G._problem(widths, bn_off, drop, batch, seed)
    want = G._reference(widths, bn_off, drop, batch, False, seed)[0]
    out = {}
    for l, s in enumerate(spec):
        if s.bn:
            for name, start in ((f"mov_mean{l}", p.mov_mean[l]), (f"mov_var{l}", p.mov_var[l])):
                out[name] = (start.astype(np.float64), (want[name] - P.BN_MOMENTUM * start.astype(np.float64)) / (1 - P.BN_MOMENTUM))
    return out


def _expected(case, factor, k):
    """The reference of the k-th consecutive step taken with inv_batch = factor / batch."""
    key = (case["widths"], case["bn_off"], case["drop"], case["batch"])
    want, correct, _ = G._reference(*key, False, case["seed"])
    out = {}
    for name, v in want.items():
        if name.startswith("mov_"):
            start, stat = _batch_moments(*key, case["seed"])[name]
            out[name] = stat + P.BN_MOMENTUM ** k * (start - stat)
        else:
            out[name] = v if name == "loss_rows" else v * factor
    return out, correct


def _hold(case, what, got, got_correct, want, correct):
    failed = []
    worst = 0.0
    for name in want:
        err = G._err(name, got[name], want[name])
        bound = G._fp32_bound(name)
        worst = max(worst, err / bound) if err == err else float("inf")
        if not err < bound:
            where = np.unravel_index(np.argmax(np.abs(got[name] - want[name])), want[name].shape)
            failed.append(f"{name}: {err:.3e} >= {bound:.3e} at {where}")
    print(f"{case['id']} {what}: worst tensor at {worst:.3g} of its bound")
    assert not failed, (what, failed)
    np.testing.assert_array_equal(got_correct, correct, err_msg=what)


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("gradients", "loss rows", "correct rows")):
        assert torch.equal(x, y), f"{what}: {name} differ"


def _claimed(case, moved, what, claims=None):
    missing = set(case["claims"] if claims is None else claims) - set(moved)
    assert not missing, f"{what}: claimed but did not run: " + ", ".join(G._key_name(k) for k in sorted(missing, key=str))


def _swing(case, form, claims=None):
    m, spec, xt, yt, mt = G.open_plan_case(case)
    batch = case["batch"]
    bits = []
    for k, factor in enumerate((1.0, 2.0 ** -S, 1.0), start=1):
        got, got_correct, moved, b = _step(m, spec, case, xt, yt, mt, factor / batch, form)
        bits.append(b)
        _claimed(case, moved, f"step {k}", claims)
        if form == "head+dw0" and claims is not None:  # layer 0's [dW; db] took a launch of its own (AMODE 1, BMODE 1, mode 2, plain store)
            assert any(key[0] != "group" and key[2:] == (1, 1, 2, G.EPI_STORE) for key in moved), f"step {k}: no launch of layer 0's weight gradient"
        _hold(case, f"form {form}, step {k} (inv_batch {factor:g} / {batch})", got, got_correct, *_expected(case, factor, k))
    _same_bits(bits[0], bits[2], "steps 1 and 3")


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids)
def test_swing_of_the_gradient_scale_against_float64(cuda, case):
    """Three consecutive steps at inv_batch = 1/B, 2^-S/B, 1/B in the case's own form, every step at the fp32 bounds."""
    _swing(case, case["form"])


@pytest.mark.parametrize("case", [c for c in STEP_CASES if c["form"] != "head+dw0"], ids=[i for i in _ids if i != "head-dw0-lds-a2"])
def test_swing_through_head_and_dw0(cuda, case):
    """The same swing through train_fwd_bwd(defer_dw0=True) + train_dw0: the clear and the publish come from the head's launches,
    layer 0's weight gradient reads the scale in a launch of its own.  Without layer 0 the group is another one, so of the case's
    claims only the plain GEMMs are asserted (the forward and input-gradient launches, which the head shares with the whole step)."""
    _swing(case, "head+dw0", claims=[k for k in case["claims"] if k[0] != "group"])


@pytest.mark.parametrize("case", [c for c in STEP_CASES if c["id"] in SEGMENT_CASE_IDS], ids=SEGMENT_CASE_IDS)
def test_swing_through_the_segments(cuda, case):
    """The same swing through lipasr_mlp_train_segment: every segment in order, one rank, stat_batch = batch.  The GEMMs are the
    launch chain's (the exchange epilogue is never taken in a segment), so the case's claims hold as they stand."""
    _swing(case, "segments")


@functools.lru_cache(maxsize=None)
def _oracle_nonfinite(widths, bn_off, drop, batch, seed):
    spec, p, x, y, masks = G._problem(widths, bn_off, drop, batch, seed)
    x64 = x.astype(np.float64)
    x64[0, 0] = np.nan
    with np.errstate(all="ignore"):
        ref = P.forward_backward(spec, p.astype(np.float64), x64, y.astype(np.float64), masks=masks, training=True)
    t = G._tensors(spec, p.astype(np.float64), ref, y.astype(np.float64))
    return {k: ~np.isfinite(v) for k, v in t.items() if k.startswith("d")}


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids)
def test_clean_step_after_a_non_finite_step(cuda, case):
    """clean, NaN (x[0, 0]), clean on one plan: the NaN step's gradients are non-finite where the oracle's are, the clean step after
    it meets the bounds and has the bits of the clean step before it."""
    m, spec, xt, yt, mt = G.open_plan_case(case)
    batch = case["batch"]
    start = m._bnstate.clone()
    want, correct = _expected(case, 1.0, 1)
    got, got_correct, _, before = _step(m, spec, case, xt, yt, mt, 1.0 / batch, case["form"])
    _hold(case, "clean step before", got, got_correct, want, correct)
    m._bnstate.copy_(start)
    bad = xt.clone()
    bad[0, 0] = float("nan")
    got, _, moved, _ = _step(m, spec, case, bad, yt, mt, 1.0 / batch, case["form"])
    _claimed(case, moved, "NaN step")
    finite = {}
    for name, nonfinite in _oracle_nonfinite(case["widths"], case["bn_off"], case["drop"], batch, case["seed"]).items():
        assert nonfinite.any(), name
        n = int((np.isfinite(got[name]) & nonfinite).sum())
        if n:
            finite[name] = f"{n} of {int(nonfinite.sum())}"
    print(f"{case['id']} NaN step: finite where the oracle is not: {finite or 'nowhere'}")
    assert not finite, finite
    m._bnstate.copy_(start)
    got, got_correct, moved, after = _step(m, spec, case, xt, yt, mt, 1.0 / batch, case["form"])
    _claimed(case, moved, "clean step after")
    _hold(case, "clean step after", got, got_correct, want, correct)
    _same_bits(before, after, "the clean steps before and after the NaN step")


@pytest.mark.parametrize("case", STEP_CASES, ids=_ids)
def test_gradients_that_shrink_against_inv_batch(cuda, case):
    """The scale is READ: a step on the case's own parameters (it leaves the maxima of ordinary gradients behind), then, on the same
    plan, a step with gamma of the last BatchNorm layer times 2^-T.  Every dz from that layer down is 2^T times smaller at the same
    inv_batch, so the static scale of inv_batch -- what a GEMM without sa_dyn / sb_dyn falls back to, and what the swing moves along
    with the gradients -- no longer fits them: on the two-plane oracle it puts a weight gradient at 14 to 1070 times its bound
    (T = 19, test_f16x2_steps_cpu.py), where the measured scale costs under 2 % of it.  Held to the float64 oracle of that problem at
    the fp32 bounds, the claimed instances counted."""
    m, spec, xt, yt, mt = G.open_plan_case(case)
    batch = case["batch"]
    start = m._bnstate.clone()
    _step(m, spec, case, xt, yt, mt, 1.0 / batch, case["form"])
    p = G._problem(case["widths"], case["bn_off"], case["drop"], batch, case["seed"])[1]
    load_params(m, shrunk(spec, p))  # (also puts the moving statistics back)
    assert torch.equal(m._bnstate, start)
    got, got_correct, moved, _ = _step(m, spec, case, xt, yt, mt, 1.0 / batch, case["form"])
    _claimed(case, moved, "shrunk step")
    _hold(case, f"gamma of the last BatchNorm layer times 2^-{T}", got, got_correct, *shrunk_reference(problem_key(case)))
