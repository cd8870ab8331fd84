"""What test_f16x2_steps_cpu.py and test_f16x2_steps_gpu.py share: the cases (one per implementation of the gradient-scale state of
arithmetic mode 2, taken from PLAN_CASES of test_gemm_instances_gpu.py at their shapes), the swing S, the gamma shift T, and the
reference-side two-plane rounding that both are chosen with.  Problems, references, bounds, knobs and launch counters are
test_gemm_instances_gpu.py's.

The rounding is an estimate of what a stale scale costs, made on the float64 oracle alone.  It is no model of the kernels' bits and
no device value is compared with it."""
import functools

import numpy as np

import test_gemm_instances_gpu as G
from oracle import mlp_ref as P

# one case per implementation: the clear (amax_zero) sits in the forward GEMM's tile family, the publish (amax_out) in
# bn_apply_bwd_kernel (launch chain) or the EPI_DH_BNX epilogue (exchange), the read (sa_dyn / sb_dyn) in the input-gradient GEMM's
# family and in the grouped / split weight-gradient kernels
STEP_CASE_IDS = ("chain-frag-a2", "chain-lds-a2", "exchange-frag-a2", "exchange-ring-x1", "exchange-ring", "exchange-ring2", "group-lds-a2",
                 "group-ring-64", "group-ring-128-split-pass", "group-ring-128-per-fragment", "head-dw0-lds-a2")
STEP_CASES = [c for c in G.PLAN_CASES if c["id"] in STEP_CASE_IDS]
assert [c["id"] for c in STEP_CASES] == list(STEP_CASE_IDS) and all(c["arith"] == 2 for c in STEP_CASES)
SEGMENT_CASE_IDS = ("chain-frag-a2", "chain-lds-a2")

# The swing: the middle step of three runs with inv_batch = 2^-S / B.  The smallest S at which a scale left over from the step
# before breaks a weight gradient's bound tenfold on every case's problem (test_f16x2_steps_cpu.py holds it to that, and to S - 1
# not doing so).
S = 27


def two_plane(x, c):
    """x as the sum of two fp16 numbers at scale c: hi = f16(x c), lo = f16(x c - hi), value (hi + lo) / c (numpy float16: round to
    nearest even, gradual underflow)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = (x * c).astype(np.float16).astype(np.float64)
        lo = (x * c - hi).astype(np.float16).astype(np.float64)
    return (hi + lo) / c


def scale_of_max(a):
    """2^(14 - e) with max |a| = f 2^e, f in [0.5, 1): the largest value lands in [2^13, 2^14); 1 for an all-zero or non-finite tensor."""
    m = float(np.abs(a).max())
    if not (m > 0.0) or not np.isfinite(m):
        return 1.0
    return float(np.ldexp(1.0, 14 - np.frexp(m)[1]))


class TwoPlaneOperands:
    """round_operands for oracle.mlp_ref.forward_backward: every operand of a matrix product rounded to two fp16 planes at the scale
    the design gives its kind -- activations and inputs 1, kernels 2^12, the gradient at the logits 2^8 / 2^e of inv_batch = f 2^e,
    every other gradient (the dz of a BatchNorm layer) 2^(14 - e) of its own maximum, divided by 2^stale: what a scale that was left
    at the value of a step with 2^stale times larger gradients does to this step.

    The oracle calls it on (input, kernel) per layer on the way forward and on (input, dz, dz[, dz, kernel]) per layer on the way
    back, from the last layer down: kernels are known by identity, the inputs of the forward pass are remembered, and what is
    neither is a gradient -- the last layer's on the first calls (3, or 2 in a one-layer network)."""

    def __init__(self, p64, inv_batch, stale=0, static=False):
        self.kernels = {id(w) for w in p64.W}
        self.layers = len(p64.W)
        self.inputs = {}
        self.grad_calls = 0
        self.logit_scale = float(np.ldexp(1.0, 8 - np.frexp(inv_batch)[1]))
        self.stale = stale
        self.static = static  # every gradient at the scale of the gradient at the logits: what a GEMM does that does not read the maximum

    def __call__(self, a):
        if id(a) in self.kernels:
            return two_plane(a, 4096.0)
        if len(self.inputs) < self.layers or id(a) in self.inputs:
            self.inputs[id(a)] = a  # (kept alive: its identity stays its own)
            return two_plane(a, 1.0)
        self.grad_calls += 1
        if self.static or self.grad_calls <= (3 if self.layers > 1 else 2):
            return two_plane(a, self.logit_scale)
        return two_plane(a, scale_of_max(a) / 2.0 ** self.stale)


# The swing moves every gradient together with inv_batch, and with it the static scale 2^8 / 2^e of inv_batch that a GEMM falls
# back to when it has no maximum to read (sa_dyn / sb_dyn null): the swing cannot see a scale that is not read.  The second problem
# per case moves the gradients AGAINST inv_batch: gamma of the last BatchNorm layer times 2^-T.  Every dz from that layer down is
# 2^T times smaller at the same inv_batch (they are linear in that gamma), while the forward pass stays well conditioned: that
# layer's output is beta + 2^-T gamma xhat, and no BatchNorm follows it that would divide by what is left of its variation.
# T is the smallest shift at which the static scale breaks a weight gradient's bound tenfold on every case's problem
# (test_f16x2_steps_cpu.py), the design's scale staying inside every bound.
T = 19


def shrunk(spec, p, shift=None):
    """p with gamma of the last BatchNorm layer times 2^-shift (exact in fp32)."""
    q = p.copy()
    l = max(i for i, s in enumerate(spec) if s.bn)
    q.gamma[l] = q.gamma[l] * q.gamma[l].dtype.type(2.0 ** -(T if shift is None else shift))
    return q


def problem_key(case):
    return (case["widths"], case["bn_off"], case["drop"], case["batch"], case["seed"])


@functools.lru_cache(maxsize=None)
def shrunk_reference(key, shift=None):
    """The float64 oracle on the case's problem with the shrunk gamma -> (tensors, correct rows), as _reference gives them."""
    widths, bn_off, drop, batch, seed = key
    spec, p, x, y, masks = G._problem(widths, bn_off, drop, batch, seed)
    p64, y64 = shrunk(spec, p, shift).astype(np.float64), y.astype(np.float64)
    ref = P.forward_backward(spec, p64, x.astype(np.float64), y64, masks=masks, training=True)
    return G._tensors(spec, p64, ref, y64), (ref["prob"].argmax(1) == y.argmax(1)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _two_plane_errors(key, stale, static, shift):
    widths, bn_off, drop, batch, seed = key
    spec, p, x, y, masks = G._problem(widths, bn_off, drop, batch, seed)
    if shift is None:
        want = G._reference(widths, bn_off, drop, batch, False, seed)[0]
    else:
        want, p = shrunk_reference(key, shift)[0], shrunk(spec, p, shift)
    p64, x64, y64 = p.astype(np.float64), x.astype(np.float64), y.astype(np.float64)
    rnd = TwoPlaneOperands(p64, 1.0 / batch, stale, static)
    got = G._tensors(spec, p64, P.forward_backward(spec, p64, x64, y64, masks=masks, training=True, round_operands=rnd), y64)
    assert rnd.grad_calls == 3 * len(spec) - 1 and len(rnd.inputs) == len(spec)  # the call order this class relies on
    return {k: G._err(k, got[k], want[k]) / G._fp32_bound(k) for k in want}


def two_plane_errors(case, stale=0, static=False, shift=None):
    """Per tensor, the error of the two-plane oracle against the float64 oracle, as a share of _fp32_bound: on the case's problem,
    or (shift) on the one with the shrunk gamma; at the design's scales, at dz scales stale by 2^stale, or at the static scale."""
    return _two_plane_errors(problem_key(case), stale, static, shift)

