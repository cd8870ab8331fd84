"""Every K3 Lipschitz-projection kernel path (csrc/spectral.hip and spectral_*.hip) against float64, and proof of which kernels ran.

Every case goes through the raw C entry points with ctypes, so that pointers, alignment and iteration counts are the test's:

  * memory: all kernels of a case live in ONE device buffer with at least 8 sentinel floats before, between and after them (an
    "aligned" kernel starts at a multiple of 4 floats, an "unaligned" one at a multiple of 4 plus 1); outputs have a sentinel tail.
    The sentinels must survive: the scaling kernels rewrite the model's weights in place.
  * kernels: every case names the kernels it is meant to run in a module-level table, with the launch counts written out by hand
    from the selector's rules (launch_chain, sigma_fused_fits, run_power_iteration); lipasr_debug_k3_launches must show that
    exactly those counters moved by exactly those amounts.
  * float64: a product norm against the chain multiplied in float64 and numpy.linalg.svd; whole passes against
    oracle.constraints_ref; clipping against the float64 SVD.
  * determinism: twice from the same inputs, bit-identical outputs (the file header of spectral.hip promises it to data-parallel
    replicas).

Tolerances are the project's own: RTOL = 2e-5 of test_spectral_gpu.py for sigma, the norms and the projected kernels (the float32
oracle is within 2e-7 of the float64 chain for every product shape below, so none of it is spent on the reference); the bounds of
test_sv_clip_matches_lapack for lipasr_sv_clip; 1e-6 for the BatchNorm factor (two correctly rounded fp32 operations) and 1e-5 for the
Frobenius projection (test_custom_constraint_frobenius).  Each case prints its worst observed error (-s); the last test prints the
worst per kernel, which DESIGN.md (K3 section) records.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from golden import inputs
from helpers import rel_err
from oracle import constraints_ref as R

pytestmark = pytest.mark.gpu
RTOL = 2e-5
RHO = 0.7
GUARD = 8
SENTINEL = -12345.0

# kernel ids of lipasr_debug_k3_launches (include/lipasr.h)
CS12, CS20, CS32, HEAD, PSIG, SCALE, SSL, PI_U, PI_V, PI_FIN, SVCLIP, FROB, BNC = range(13)
K3_NAMES = ("chain_step_kernel<12>", "chain_step_kernel<20>", "chain_step_kernel<32>", "chain_head_kernel", "product_sigma_kernel",
            "scale_layers_kernel", "sigma_scale_layers_kernel", "pi_u_kernel", "pi_v_kernel", "pi_finish_kernel", "sv_clip_kernel",
            "sumsq_clamped_kernel + frob_scale_kernel", "bn_correction_kernel")
ALL, NONE = "all", ()

_ran = {}    # kernel id -> the first case whose counter assertion showed it running
_worst = {}  # kernel id -> (worst relative error of a case that ran it, that case)


def _native():
    from lipasr import _native as N

    return N


@pytest.fixture(autouse=True)
def _automatic_chain_head():
    """The cases state what the automatic chain-head rule does, whatever LIPASR_CHAIN_HEAD says in the environment."""
    _native().lib.lipasr_debug_chain_head(-1)
    yield


def _snapshot():
    lib = _native().lib
    return [lib.lipasr_debug_k3_launches(k) for k in range(len(K3_NAMES))]


def _moved(before):
    return {k: a - b for k, (b, a) in enumerate(zip(before, _snapshot())) if a != b}


def _names(moved):
    return {K3_NAMES[k]: v for k, v in moved.items()}


def _record(case_id, expect, err):
    for k in expect:
        _ran.setdefault(k, case_id)
        if err is not None and (k not in _worst or err > _worst[k][0]):
            _worst[k] = (err, case_id)


class Guarded:
    """Arrays in one device buffer: [>= 8 sentinels] a0 [>= 8 sentinels] a1 ... [>= 8 sentinels]."""

    def __init__(self, arrays, unaligned=NONE):
        self.shapes = [a.shape for a in arrays]
        self.offs = []
        pos = 0
        for i, a in enumerate(arrays):
            pos = (pos + GUARD + 3) // 4 * 4 + (1 if unaligned == ALL or i in unaligned else 0)
            self.offs.append(pos)
            pos += a.size
        host = np.full(pos + GUARD, SENTINEL, np.float32)
        self.guard = np.ones(host.size, bool)
        for o, a in zip(self.offs, arrays):
            host[o:o + a.size] = np.asarray(a, np.float32).ravel()
            self.guard[o:o + a.size] = False
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        for i, o in enumerate(self.offs):
            assert o % 4 == (1 if unaligned == ALL or i in unaligned else 0)

    def ptr(self, i):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.offs[i])

    def ptrs(self):
        N = _native()
        return C.cast(N.ptr_array([self.buf.data_ptr() + 4 * o for o in self.offs]), N.PV)

    def read(self):
        """The arrays back on the host; asserts that no sentinel was touched."""
        host = self.buf.cpu().numpy()
        bad = np.flatnonzero(host[self.guard] != np.float32(SENTINEL))
        assert bad.size == 0, f"{bad.size} sentinel floats were written, first at float {np.flatnonzero(self.guard)[bad[0]]} (kernels start at {self.offs})"
        return [host[o:o + int(np.prod(s))].reshape(s).copy() for o, s in zip(self.offs, self.shapes)]


def _out(n):
    return torch.full((n + GUARD,), SENTINEL, device="cuda")


def _read_out(t, n):
    host = t.cpu().numpy()
    assert (host[n:] == np.float32(SENTINEL)).all(), "an output was written past its end"
    return host[:n].copy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _chain64(ws):
    p = None
    for w in reversed(ws):
        wt = np.asarray(w, np.float64).T
        p = wt if p is None else p @ wt
    return p


def _sigma64(ws):
    return float(np.linalg.svd(_chain64(ws), compute_uv=False)[0])


# =================================================================================================
# A. product path: lipasr_project_product, then lipasr_product_norm on the result
# =================================================================================================
def _orthonormal(rng, n, k):
    return np.linalg.qr(rng.standard_normal((n, k)))[0]


def _stack(kind, widths):
    if kind == "signed":
        return inputs.signed_kernels(widths)
    if kind == "nonneg":
        return inputs.nonneg_kernels(widths)
    rng = np.random.default_rng(5)
    if kind == "tie":  # orthonormal 48 x 48 times 1.5 x orthonormal 48 x 16: every singular value of the product is 1.5
        return [_orthonormal(rng, 48, 48).astype(np.float32), (1.5 * _orthonormal(rng, 48, 16)).astype(np.float32)]
    if kind == "rank1":  # outer product of two seeded vectors, then a signed 24 x 10
        return [np.outer(rng.standard_normal(60), rng.standard_normal(24)).astype(np.float32) * np.float32(0.2), inputs.signed_kernels([24, 10])[0]]
    if kind == "tiny":
        return [w * np.float32(1e-6) for w in inputs.nonneg_kernels(widths)]
    if kind == "huge":
        return [w * np.float32(1e+4) for w in inputs.nonneg_kernels(widths)]
    if kind == "zero-second":
        ws = inputs.nonneg_kernels(widths)
        ws[1] = np.zeros_like(ws[1])
        return ws
    raise KeyError(kind)


def pc(id, widths, kind, expect, why, unaligned=NONE, affected=()):
    return dict(id=id, widths=widths, kind=kind, expect=expect, why=why, unaligned=unaligned, affected=list(affected))


# Launch counts of ONE lipasr_project_product (n_order > 0) followed by ONE lipasr_product_norm, by hand from the selector:
#   chain: m - 1 chain steps (1 for a single layer) of the instance <12> / <20> / <32> that holds the R classes; with m >= 4, R <= 16
#          and the two leading panels <= 256 columns, multiples of 16, 16-byte aligned: chain_head_kernel + (m - 3) steps.
#   sigma: 80 R^2 + 4 R n_0 + 16 bytes of LDS <= 96 KiB -> sigma_scale_layers_kernel; otherwise the chain's last step emits Gram
#          partials for product_sigma_kernel and scale_layers_kernel follows.  lipasr_product_norm: chain + product_sigma_kernel.
# Shapes changed from the ones first listed for this table, because they would not take the path they were chosen for:
#   40-2052-20 -> 40-1872-20.  An 80-byte x 2052 panel is 164 160 B, over the 163 328 B the chain step admits: the call is refused.
#     1872 columns is the widest multiple of 4 whose panel fits WITH the Gram partials of lipasr_product_norm (163 088 B).
#   order [3] on a stack of three kernels is out of range (EINVAL, asserted in test_order_list_limits); the one-entry list is [2].
_A = {CS12: 2, SSL: 1, PSIG: 1}
_B = {CS20: 2, SSL: 1, PSIG: 1}
_C = {CS32: 2, SSL: 1, PSIG: 1}
PRODUCT_CASES = [
    pc("70-48-12", [70, 48, 12], "signed", _A, "12 classes: the last size of the <12> instance"),
    pc("70-48-13", [70, 48, 13], "signed", _B, "13 classes: the first size of <20>"),
    pc("70-48-20", [70, 48, 20], "signed", _B, "20 classes: the last size of <20>"),
    pc("70-48-21", [70, 48, 21], "signed", _C, "21 classes: the first size of <32>"),
    pc("70-48-32", [70, 48, 32], "signed", _C, "<32>, 1024 Gram entries; sigma_scale_layers_kernel at 90 896 B of LDS (passes the 96 KiB rule)"),
    pc("70-48-32-nonneg", [70, 48, 32], "nonneg", _C, "the same on a stack with a dominant singular value"),
    pc("1000-64-32", [1000, 64, 32], "signed", {CS32: 2, PSIG: 2, SCALE: 1}, "209 936 B fail the 96 KiB rule: 250 Gram partials, one slice, product_sigma + scale_layers"),
    pc("1000-64-32-unaligned", [1000, 64, 32], "signed", {CS32: 2, PSIG: 2, SCALE: 1}, "the scalar loop of scale_layers_kernel", unaligned=ALL),
    pc("64-1500-10", [64, 1500, 10], "signed", _A, "n_in = 1500 > 1024: the row loop past the register prefetch, vector form"),
    pc("64-1501-10", [64, 1501, 10], "signed", _A, "the same, scalar form (n_in % 4 != 0)"),
    pc("40-1872-20", [40, 1872, 20], "signed", _B, "<20> past the prefetch with a 149 760 B panel (163 088 B with Gram partials); R n_0 small: the fused sigma launch"),
    pc("70-1000-32", [70, 1000, 32], "nonneg", _C, "the chain step's LDS near its limit: 161 296 B with Gram partials"),
    pc("50-32", [50, 32], "signed", _C, "one layer (p_mode 2) at 32 classes"),
    pc("40-24-1", [40, 24, 1], "signed", _A, "one class"),
    pc("96-64-32-10-unaligned", [96, 64, 32, 10], "signed", {CS12: 4, SSL: 1, PSIG: 1}, "scalar branches of chain step, sigma-scale and its scaling loop", unaligned=ALL),
    pc("33-17-5-unaligned", [33, 17, 5], "nonneg", _A, "the same with odd sizes", unaligned=ALL),
    pc("33-17-5", [33, 17, 5], "nonneg", _A, "aligned with odd sizes: the float4 loops' scalar tails (561 = 4 x 140 + 1 elements)"),
    pc("300-256-128-64-16", [300, 256, 128, 64, 16], "nonneg", {HEAD: 2, CS20: 2, SSL: 1, PSIG: 1}, "chain head with two fused steps, then one chain step"),
    pc("300-256-128-64-16-w2-unaligned", [300, 256, 128, 64, 16], "nonneg", {CS20: 6, SSL: 1, PSIG: 1}, "chain head refused by the alignment of Ws[2]", unaligned=(2,)),
    pc("100-64-272-64-16", [100, 64, 272, 64, 16], "nonneg", {CS20: 6, SSL: 1, PSIG: 1}, "a 272-column panel: no chain head"),
    pc("300-256-128-64-17", [300, 256, 128, 64, 17], "nonneg", {CS20: 6, SSL: 1, PSIG: 1}, "17 classes: no chain head"),
    pc("256-128-16", [256, 128, 16], "nonneg", _B, "three layers of units: no chain head"),
    pc("256-128-64-16", [256, 128, 64, 16], "nonneg", {CS20: 4, SSL: 1, PSIG: 1}, "three kernels, every panel legal: still no chain head (it needs four)"),
    pc("35-17-9-5", [35, 17, 9, 5], "nonneg", {CS12: 4, SSL: 1, PSIG: 1}, "a 5 x 17 panel between two steps: 85 floats, staged by the scalar loop"),
    pc("16-layers", [32] * 16 + [10], "nonneg", {HEAD: 2, CS12: 26, SSL: 1, PSIG: 1}, "LIPASR_MAX_LAYERS kernels: chain head, then 13 steps; the 16th root of the scale"),
    # order lists (the oracle visits the listed indices in reverse layer order, once per occurrence)
    pc("order-[2]", inputs.SMALL_WIDTHS, "signed", {CS12: 4, SSL: 1, PSIG: 1}, "one entry", affected=[2]),
    pc("order-[0,0,0]", inputs.SMALL_WIDTHS, "signed", {CS12: 4, SSL: 1, PSIG: 1}, "one layer three times", affected=[0, 0, 0]),
    pc("order-64", inputs.SMALL_WIDTHS, "signed", {CS12: 4, SSL: 1, PSIG: 1}, "kMaxOrder entries", affected=[0, 1, 2] * 21 + [0]),
    # spectra
    pc("tie", [48, 48, 16], "tie", _B, "sigma_1 = ... = sigma_16 = 1.5: the squarings never reach a rank-one projector"),
    pc("rank-one", [60, 24, 10], "rank1", _A, "a rank-one product: the squaring loop leaves at once"),
    pc("scaled-1e-6", inputs.SMALL_WIDTHS, "tiny", {CS12: 4, SSL: 1, PSIG: 1}, "sigma = 1.5e-16, next to eps = 2.2e-16"),
    pc("scaled-1e+4", inputs.SMALL_WIDTHS, "huge", {CS12: 4, SSL: 1, PSIG: 1}, "sigma = 1.5e+14"),
    pc("zero-second-kernel", inputs.SMALL_WIDTHS, "zero-second", {CS12: 4, SSL: 1, PSIG: 1}, "sigma = 0: the pass divides by eps"),
]
PRODUCT_BY_ID = {c["id"]: c for c in PRODUCT_CASES}


def _visit_order(case):
    m = len(case["widths"]) - 1
    if not case["affected"]:
        return list(range(m))
    return [i for i in reversed(range(m)) for j in case["affected"] if j == i]  # Constraints.py:181-189


def _project_and_norm(ws, unaligned, order, rho=RHO):
    """One lipasr_project_product and one lipasr_product_norm on kernels in a guarded buffer."""
    N = _native()
    h = N.get_handle(0)
    g = Guarded(ws, unaligned)
    rows, cols = N.int_array([w.shape[0] for w in ws]), N.int_array([w.shape[1] for w in ws])
    norms, sig = _out(len(order) + 1), _out(1)
    before = _snapshot()
    rc1 = N.lib.lipasr_project_product(h.h, g.ptrs(), rows, cols, len(ws), rho, N.int_array(order), len(order), N.ptr(norms), N.stream_ptr())
    err1 = N.last_error() if rc1 else ""
    rc2 = N.lib.lipasr_product_norm(h.h, g.ptrs(), rows, cols, len(ws), N.ptr(sig), N.stream_ptr())
    err2 = N.last_error() if rc2 else ""
    torch.cuda.synchronize()
    return dict(rc=(rc1, rc2), err=(err1, err2), moved=_moved(before), ws=g.read(), norms=_read_out(norms, len(order) + 1), sigma=float(_read_out(sig, 1)[0]))


@functools.lru_cache(maxsize=None)
def _product_result(case_id):
    """Runs the case twice (bitwise repeatability), checks its counters and returns the first run with its inputs."""
    case = PRODUCT_BY_ID[case_id]
    ws = _stack(case["kind"], case["widths"])
    order = _visit_order(case)
    a = _project_and_norm(ws, case["unaligned"], order)
    b = _project_and_norm(ws, case["unaligned"], order)
    for r in (a, b):
        assert r["rc"] == (0, 0), r["err"]
        assert r["moved"] == case["expect"], (_names(r["moved"]), "expected", _names(case["expect"]))
    assert all(_same_bits(x, y) for x, y in zip(a["ws"], b["ws"])), "projected kernels differ between two runs"
    assert _same_bits(a["norms"], b["norms"]) and _same_bits(np.float32(a["sigma"]), np.float32(b["sigma"]))
    a["inputs"] = ws
    return a


@pytest.mark.parametrize("case_id", [c["id"] for c in PRODUCT_CASES])
def test_product_path_against_float64(cuda, case_id):
    case = PRODUCT_BY_ID[case_id]
    got = _product_result(case_id)
    ref_ws, ref_norms = R.simple_norm_constraint_pass(got["inputs"], RHO, case["affected"])
    e_norm = max((abs(float(x) - y) / y if y > 0 else abs(float(x))) for x, y in zip(got["norms"], ref_norms))
    e_w = max(rel_err(x, y) for x, y in zip(got["ws"], ref_ws))
    want_sigma = _sigma64(got["ws"])  # the norm of what the projection left behind, chain in float64
    e_sigma = abs(got["sigma"] - want_sigma) / want_sigma if want_sigma > 0 else abs(got["sigma"])
    print(f"\n{case_id}: norms {e_norm:.2e}, kernels {e_w:.2e}, sigma after {e_sigma:.2e} (sigma before {got['norms'][0]:.6g}, after {got['sigma']:.6g}); {case['why']}")
    _record(case_id, case["expect"], max(e_norm, e_w, e_sigma))
    assert len(got["norms"]) == len(ref_norms)
    np.testing.assert_allclose(got["norms"], ref_norms, rtol=RTOL, atol=0)
    assert e_w < RTOL
    assert e_sigma < RTOL
    assert all(np.isfinite(w).all() for w in got["ws"])
    if case["kind"] == "zero-second":
        assert got["norms"].max() == 0.0 and got["sigma"] == 0.0 and not got["ws"][1].any()
    if case["kind"] == "tie":
        assert abs(got["norms"][0] - 1.5) < RTOL * 1.5
    if case["affected"]:  # kernels that are not listed keep their bits
        for l, (w, w0) in enumerate(zip(got["ws"], got["inputs"])):
            assert l in case["affected"] or _same_bits(w, w0)


def test_chain_head_refused_by_alignment_gives_the_same_result(cuda):
    """The fused head associates its sums differently from one launch per step: 2e-6, the bound test_spectral_gpu.py gives it."""
    a, b = _product_result("300-256-128-64-16"), _product_result("300-256-128-64-16-w2-unaligned")
    np.testing.assert_allclose(a["norms"], b["norms"], rtol=2e-6, atol=0)
    for x, y in zip(a["ws"], b["ws"]):
        np.testing.assert_allclose(x, y, rtol=2e-6, atol=0)


def test_panel_above_the_lds_limit_is_refused(cuda):
    """70-1400-32: a 32 x 1400 panel is 179 200 B, over the 163 328 B the chain step admits.  Both entry points return
    LIPASR_EUNSUPPORTED with a message before anything is launched, and the kernels keep their bits."""
    N = _native()
    ws = inputs.signed_kernels([70, 1400, 32])
    got = _project_and_norm(ws, NONE, [0, 1])
    assert got["rc"] == (N.EUNSUPPORTED, N.EUNSUPPORTED)
    assert all("does not fit LDS" in e for e in got["err"]), got["err"]
    assert got["moved"] == {}, _names(got["moved"])
    assert all(_same_bits(x, y) for x, y in zip(got["ws"], ws))
    assert (got["norms"] == np.float32(SENTINEL)).all() and got["sigma"] == SENTINEL


def test_order_list_limits(cuda):
    """No order (norm only, through both entry points), 65 entries and an index past the last layer."""
    N = _native()
    h = N.get_handle(0)
    ws = inputs.signed_kernels(inputs.SMALL_WIDTHS)
    _, ref_norms = R.simple_norm_constraint_pass(ws, RHO, [])
    want = _sigma64(ws)
    assert abs(ref_norms[0] - want) / want < 1e-6
    rows, cols = N.int_array([w.shape[0] for w in ws]), N.int_array([w.shape[1] for w in ws])
    res = []
    for _ in range(2):
        g = Guarded(ws)
        sig, norms = _out(1), _out(1)
        before = _snapshot()
        N.check(N.lib.lipasr_product_norm(h.h, g.ptrs(), rows, cols, 3, N.ptr(sig), N.stream_ptr()))
        N.check(N.lib.lipasr_project_product(h.h, g.ptrs(), rows, cols, 3, RHO, N.int_array([]), 0, N.ptr(norms), N.stream_ptr()))
        torch.cuda.synchronize()
        expect = {CS12: 4, PSIG: 2}  # two chains of two steps; with no order the projection takes the Gram path and scales nothing
        moved = _moved(before)
        assert moved == expect, _names(moved)
        assert all(_same_bits(x, y) for x, y in zip(g.read(), ws))
        res.append((_read_out(sig, 1)[0], _read_out(norms, 1)[0]))
    assert _same_bits(np.float32(res[0]), np.float32(res[1])) and res[0][0] == res[0][1]
    err = abs(float(res[0][0]) - want) / want
    print(f"\norder []: sigma {err:.2e}")
    _record("order-[]", expect, err)
    assert err < RTOL
    for order in ([0] * 65, [3], [-1]):
        g = Guarded(ws)
        norms = _out(len(order) + 1)
        before = _snapshot()
        assert N.lib.lipasr_project_product(h.h, g.ptrs(), rows, cols, 3, RHO, N.int_array(order), len(order), N.ptr(norms), N.stream_ptr()) == N.EINVAL
        torch.cuda.synchronize()
        assert _moved(before) == {}
        assert all(_same_bits(x, y) for x, y in zip(g.read(), ws))
        assert (_read_out(norms, len(order) + 1) == np.float32(SENTINEL)).all()


# =================================================================================================
# B. per-layer path: lipasr_project_per_layer and lipasr_sigma_max
# =================================================================================================
# One batched call.  Seeds: signed_kernels' default for the shape's position; the 1 x 1 kernel is reseeded to a positive entry (a
# negative one clamps to the zero matrix).  sigma_2 / sigma_1 of the clamped kernels is at most 0.61 (asserted below): 48 cold
# iterations leave an error of the order 0.61^96 = 2e-21.
PER_LAYER_SHAPES = [(1, 1), (1, 37), (37, 1), (9, 33), (64, 32), (130, 70), (8192, 3), (3, 8192)]
PER_LAYER_ITERS = 48
PER_LAYER_EXPECT = {PI_U: PER_LAYER_ITERS + 1, PI_V: PER_LAYER_ITERS, PI_FIN: 1}  # (u, v) per iteration, the closing u, one finish


@functools.lru_cache(maxsize=None)
def _per_layer_inputs():
    ws = [inputs.signed_kernels(list(s), seed=11 + i)[0] for i, s in enumerate(PER_LAYER_SHAPES)]
    ws[0] = np.abs(ws[0])
    for w in ws:
        s = np.linalg.svd(np.maximum(w, 0).astype(np.float64), compute_uv=False)
        assert s[0] > 0 and (len(s) == 1 or s[1] / s[0] < 0.8), "reseed: the gap is too small for 48 iterations"
        assert min(w.shape) == 1 or (w < 0).any()
    ref = R.norm_constraint_pass(ws, 10.0)
    sig = np.array([np.linalg.svd(np.maximum(w, 0).astype(np.float64), compute_uv=False)[0] for w in ws])
    return ws, ref, sig


def _per_layer(ws, unaligned, rho, warm, iters):
    N = _native()
    h = N.get_handle(0)
    g = Guarded(ws, unaligned)
    n_v = sum(w.shape[1] for w in ws)
    v, sig = _out(n_v), _out(len(ws))
    v[:n_v] = 0.0
    before = _snapshot()
    rc = N.lib.lipasr_project_per_layer(h.h, g.ptrs(), N.int_array([w.shape[0] for w in ws]), N.int_array([w.shape[1] for w in ws]), len(ws), rho,
                                        N.ptr(v), warm, iters, N.ptr(sig), N.stream_ptr())
    torch.cuda.synchronize()
    return rc, _moved(before), g.read(), _read_out(sig, len(ws)), _read_out(v, n_v)


@pytest.mark.parametrize("unaligned", [NONE, ALL], ids=["aligned", "unaligned"])
def test_per_layer_batched_call_against_float64(cuda, unaligned):
    """1 x 1, one row, one column, rows no multiple of 8, columns no multiple of 32, and the 8192 limit both ways, in one launch
    sequence; signed kernels on the clamping path from a cold start."""
    ws, ref, sig64 = _per_layer_inputs()
    a = _per_layer(ws, unaligned, 10.0, 0, PER_LAYER_ITERS)
    b = _per_layer(ws, unaligned, 10.0, 0, PER_LAYER_ITERS)
    for r in (a, b):
        assert r[0] == 0
        assert r[1] == PER_LAYER_EXPECT, _names(r[1])
    assert all(_same_bits(x, y) for x, y in zip(a[2], b[2])) and _same_bits(a[3], b[3]) and _same_bits(a[4], b[4])
    e_sig = float(np.max(np.abs(a[3] - sig64) / sig64))
    e_w = max(rel_err(x, y) for x, y in zip(a[2], ref))
    print(f"\nper-layer {'unaligned' if unaligned else 'aligned'}: sigma {e_sig:.2e}, kernels {e_w:.2e}")
    _record("per-layer-" + ("unaligned" if unaligned else "aligned"), PER_LAYER_EXPECT, max(e_sig, e_w))
    np.testing.assert_allclose(a[3], sig64, rtol=RTOL, atol=0)
    assert e_w < RTOL
    assert all(w.min() >= 0 for w in a[2])


def _sigma_max(w, unaligned, warm, iters, clamp, v_init=None):
    N = _native()
    h = N.get_handle(0)
    g = Guarded([w], unaligned)
    v, out = _out(w.shape[1]), _out(1)
    v[:w.shape[1]] = 0.0 if v_init is None else torch.as_tensor(np.asarray(v_init, np.float32)).cuda()
    before = _snapshot()
    rc = N.lib.lipasr_sigma_max(h.h, g.ptr(0), w.shape[0], w.shape[1], N.ptr(v), warm, iters, clamp, N.ptr(out), N.stream_ptr())
    torch.cuda.synchronize()
    assert _same_bits(g.read()[0], w)  # a read-out: the kernel keeps its bits
    return rc, _moved(before), float(_read_out(out, 1)[0]), _read_out(v, w.shape[1])


def test_power_iteration_refuses_dimensions_above_8192(cuda):
    N = _native()
    h = N.get_handle(0)
    for shape in [(8193, 3), (3, 8193)]:
        w = np.ones(shape, np.float32)
        rc, moved, out, v = _sigma_max(w, NONE, 0, 4, 0)
        assert rc == N.EUNSUPPORTED and "8192" in N.last_error() and moved == {} and out == SENTINEL
        g = Guarded([w])
        vs, sig = _out(shape[1]), _out(1)
        before = _snapshot()
        assert N.lib.lipasr_project_per_layer(h.h, g.ptrs(), N.int_array([shape[0]]), N.int_array([shape[1]]), 1, 10.0, N.ptr(vs), 0, 4, N.ptr(sig),
                                              N.stream_ptr()) == N.EUNSUPPORTED
        torch.cuda.synchronize()
        assert _moved(before) == {} and _same_bits(g.read()[0], w) and _read_out(sig, 1)[0] == SENTINEL


def _constructed(shape, s_head, seed):
    """U diag(s) V^T with s = s_head, then a ramp from 2.4 down to 0.1 (as test_sigma_max_signed_matrix builds it)."""
    rng = np.random.default_rng(seed)
    k = min(shape)
    u, v = _orthonormal(rng, shape[0], k), _orthonormal(rng, shape[1], k)
    s = np.concatenate([s_head, np.linspace(2.4, 0.1, k - len(s_head))])
    return ((u * s) @ v.T).astype(np.float32), v


@pytest.mark.parametrize("unaligned", [NONE, ALL], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("head", [(3.0,), (3.0, 3.0)], ids=["gap-0.8", "tie"])
@pytest.mark.parametrize("shape", [(257, 40), (40, 257)])
def test_sigma_max_on_constructed_spectra(cuda, shape, head, unaligned):
    """Gap ratio 0.8 after 200 iterations: 0.8^400 = 1e-39.  With a tie at the top the iterate stays a mixture of the two leading
    vectors, and sigma must still come out as 3."""
    w, _ = _constructed(shape, list(head), shape[0] + len(head))
    want = float(np.linalg.svd(w.astype(np.float64), compute_uv=False)[0])
    expect = {PI_U: 201, PI_V: 200, PI_FIN: 1}
    a = _sigma_max(w, unaligned, 0, 200, 0)
    b = _sigma_max(w, unaligned, 0, 200, 0)
    assert a[0] == 0 and a[1] == expect and b[1] == expect, (_names(a[1]), _names(b[1]))
    assert _same_bits(np.float32(a[2]), np.float32(b[2])) and _same_bits(a[3], b[3])
    err = abs(a[2] - want) / want
    print(f"\nsigma_max {shape} {head} {'unaligned' if unaligned else 'aligned'}: {err:.2e}")
    _record(f"sigma-max-{shape[0]}x{shape[1]}", expect, err)
    assert err < RTOL and abs(want - 3.0) < 1e-5


def test_sigma_max_warm_start_reads_and_normalises_v_state(cuda):
    w, v = _constructed((257, 40), [3.0], 7)
    u64, s64, vt64 = np.linalg.svd(w.astype(np.float64), full_matrices=False)
    # no iteration: sigma = || W v / ||v|| ||, right only if v_state is read and normalised (1000 x too large otherwise)
    rc, moved, got, _ = _sigma_max(w, NONE, 1, 0, 0, v_init=1000.0 * vt64[0])
    assert rc == 0 and moved == {PI_U: 1, PI_FIN: 1}, _names(moved)
    e0 = abs(got - s64[0]) / s64[0]
    _record("sigma-max-warm-0", moved, e0)
    assert e0 < RTOL
    # a start vector that is not the singular vector gives another number: the check above is decisive
    rc, moved, off, _ = _sigma_max(w, NONE, 1, 0, 0, v_init=vt64[5])
    assert abs(off - s64[5]) / s64[5] < RTOL and abs(off - s64[0]) / s64[0] > 0.1
    # v_state left behind by a call on another matrix, then 200 warm iterations: the cold result
    other, _ = _constructed((100, 40), [5.0], 8)
    rc, _, _, v_left = _sigma_max(other, NONE, 0, 20, 0)
    assert rc == 0 and np.linalg.norm(v_left) > 0
    rc, moved, warm, _ = _sigma_max(w, NONE, 1, 200, 0, v_init=v_left)
    assert rc == 0 and moved == {PI_U: 201, PI_V: 200, PI_FIN: 1}, _names(moved)
    rc, _, cold, _ = _sigma_max(w, NONE, 0, 200, 0)
    e1 = abs(warm - cold) / cold
    print(f"\nwarm start: exact vector x 1000, no iteration {e0:.2e}; warm against cold after 200 iterations {e1:.2e}")
    assert e1 < RTOL and abs(cold - s64[0]) / s64[0] < RTOL


# =================================================================================================
# C. singular-value clipping
# =================================================================================================
SV_SHAPES = [(31, 255), (32, 256), (32, 257), (5, 513), (32, 20)]


def _sv_clip(x, hi, in_place):
    """X and (out of place) the output in one guarded buffer, the output unaligned; returns (out, singular values)."""
    N = _native()
    h = N.get_handle(0)
    R_, n = x.shape
    g = Guarded([x] if in_place else [x, np.zeros_like(x)], unaligned=(1,))
    sv = _out(R_)
    before = _snapshot()
    N.check(N.lib.lipasr_sv_clip(h.h, g.ptr(0), R_, n, hi, g.ptr(0 if in_place else 1), N.ptr(sv), N.stream_ptr()))
    torch.cuda.synchronize()
    moved = _moved(before)
    assert moved == {SVCLIP: 1}, _names(moved)
    arrs = g.read()
    if not in_place:
        assert _same_bits(arrs[0], x)
    return arrs[-1], _read_out(sv, R_)


def _check_sv_clip(name, x, hi):
    u, sv, vt = np.linalg.svd(x.astype(np.float64), full_matrices=False)
    want = (u * np.clip(sv, 0, hi)) @ vt
    out, got_sv = _sv_clip(x, hi, False)
    out2, got_sv2 = _sv_clip(x, hi, False)
    inp, got_sv3 = _sv_clip(x, hi, True)
    assert _same_bits(out, out2) and _same_bits(got_sv, got_sv2), "two runs differ"
    assert _same_bits(out, inp) and _same_bits(got_sv, got_sv3), "in place differs from out of place"
    k = min(x.shape)
    e_sv = float(np.max(np.abs(got_sv[:k] - sv[:k]) / (2e-6 * sv[:k] + 1e-6 * sv[0])))
    e_out = float(np.max(np.abs(out - want)) / (2e-6 * max(sv[0], 1.0)))
    print(f"\nsv_clip {name} {x.shape} hi={hi:.4g}: singular values {e_sv:.2f} of their bound, output {e_out:.2f} of its bound ({np.max(np.abs(out - want)):.2e})")
    _record(f"sv-clip-{name}-{x.shape[0]}x{x.shape[1]}", {SVCLIP: 1}, float(np.max(np.abs(out - want)) / max(sv[0], 1.0)))
    np.testing.assert_allclose(got_sv[:k], sv[:k], rtol=2e-6, atol=1e-6 * sv[0])
    assert np.all(np.abs(got_sv[k:]) <= 1e-6 * sv[0])
    assert np.max(np.abs(out - want)) <= 2e-6 * max(sv[0], 1.0)


@pytest.mark.parametrize("R_,n", SV_SHAPES)
def test_sv_clip_rank_deficient(cuda, R_, n):
    """Two identical rows and a zero row (rank R - 2 at most), at R = 31 / 32 and at the edges of the 256-column tile."""
    rng = np.random.default_rng(100 + R_ + n)
    x = rng.standard_normal((R_, n)).astype(np.float32)
    x[0] *= 4.0
    x[R_ - 1] = x[1]
    x[R_ // 2] = 0.0
    sv = np.linalg.svd(x.astype(np.float64), compute_uv=False)
    assert np.sum(sv > 1e-6 * sv[0]) == min(R_ - 2, n)
    j = min(R_ - 2, n) // 2
    _check_sv_clip("rank-deficient", x, float(np.float32(0.5 * (sv[j - 1] + sv[j]))))  # between two singular values: the upper half is clipped


@pytest.mark.parametrize("hi", [1.5, 1.0])
def test_sv_clip_equal_singular_values(cuda, hi):
    """Singular values [2, 2, 1, 1, 0.5]: the singular vectors of a pair are not unique, the clipped matrix is.  hi = 1.5 cuts the first
    pair only, hi = 1 sits exactly on the second."""
    rng = np.random.default_rng(3)
    x = ((_orthonormal(rng, 5, 5) * np.array([2.0, 2.0, 1.0, 1.0, 0.5])) @ _orthonormal(rng, 513, 5).T).astype(np.float32)
    _check_sv_clip("pairs", x, hi)


# =================================================================================================
# D. the small kernels, directly
# =================================================================================================
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1024])
def test_bn_correction_against_float64(cuda, n):
    N = _native()
    h = N.get_handle(0)
    rng = np.random.default_rng(n)
    gamma = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    var = rng.uniform(0.5, 2.0, n).astype(np.float32)
    want = float(np.max(np.sqrt(var.astype(np.float64)) / gamma.astype(np.float64)))
    res = []
    for unaligned in (NONE, ALL):
        for _ in range(2):
            g = Guarded([gamma, var], unaligned)
            out = _out(1)
            before = _snapshot()
            N.check(N.lib.lipasr_bn_correction(h.h, g.ptr(0), g.ptr(1), n, N.ptr(out), N.stream_ptr()))
            torch.cuda.synchronize()
            moved = _moved(before)
            assert moved == {BNC: 1}, _names(moved)
            arrs = g.read()
            assert _same_bits(arrs[0], gamma) and _same_bits(arrs[1], var)
            res.append(float(_read_out(out, 1)[0]))
    assert all(_same_bits(np.float32(r), np.float32(res[0])) for r in res)
    err = abs(res[0] - want) / abs(want)
    print(f"\nbn_correction n={n}: {err:.2e} (factor {want:.6g})")
    _record(f"bn-correction-{n}", {BNC: 1}, err)
    assert err < 1e-6


@pytest.mark.parametrize("unaligned", [NONE, ALL], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n,sign", [(1, 1.0), (1, -1.0), (3, 0.0), (255, 0.0), (65537, 0.0)])
def test_frobenius_project_against_float64(cuda, n, sign, unaligned):
    """Signed input (the single element of either sign: a negative one clamps to the zero kernel, norm 0)."""
    N = _native()
    h = N.get_handle(0)
    w = np.random.default_rng(n).uniform(-1, 1, n).astype(np.float32)
    if sign:
        w = np.float32(sign) * np.abs(w)
    want = R.custom_constraint(w, 5.0)
    res = []
    for _ in range(2):
        g = Guarded([w], unaligned)
        before = _snapshot()
        N.check(N.lib.lipasr_frobenius_project(h.h, g.ptr(0), n, 5.0, N.stream_ptr()))
        torch.cuda.synchronize()
        moved = _moved(before)
        assert moved == {FROB: 1}, _names(moved)
        res.append(g.read()[0])
    assert _same_bits(res[0], res[1])
    err = rel_err(res[0], want)
    print(f"\nfrobenius n={n}: {err:.2e}")
    _record(f"frobenius-{n}", {FROB: 1}, err)
    assert err < 1e-5 and np.isfinite(res[0]).all()


# =================================================================================================
# E. completeness
# =================================================================================================
CLAIMS = {"order-[]": {CS12, PSIG}, "per-layer": set(PER_LAYER_EXPECT), "sv-clip": {SVCLIP}, "bn-correction": {BNC}, "frobenius": {FROB}}
CLAIMS.update({c["id"]: set(c["expect"]) for c in PRODUCT_CASES})
CLAIMED = set().union(*CLAIMS.values())


def test_every_k3_kernel_is_claimed_and_ran(cuda):
    """The ids lipasr_debug_k3_launches knows against the claims of the tables above: a kernel added without a case fails here.
    Every id has a positive count attributed to a named case; a product case whose kernel has not run yet in this session (the
    module was run in part) is run here."""
    lib = _native().lib
    have = {k for k in range(64) if lib.lipasr_debug_k3_launches(k) >= 0}
    assert lib.lipasr_debug_k3_launches(-1) == -1 and lib.lipasr_debug_k3_launches(len(K3_NAMES)) == -1
    assert have == CLAIMED, (sorted(have), sorted(CLAIMED))
    for k in sorted(have - set(_ran)):
        case = next((c for c in PRODUCT_CASES if k in c["expect"]), None)
        if case is not None:
            _product_result(case["id"])
            _record(case["id"], case["expect"], None)
    alone = {PI_U: lambda: test_per_layer_batched_call_against_float64(None, NONE), SVCLIP: lambda: test_sv_clip_equal_singular_values(None, 1.5),
             FROB: lambda: test_frobenius_project_against_float64(None, 3, 0.0, NONE), BNC: lambda: test_bn_correction_against_float64(None, 63)}
    for k in sorted(set(alone) - set(_ran)):
        alone[k]()
    missing = have - set(_ran)
    assert not missing, "no case of this session ran: " + ", ".join(K3_NAMES[k] for k in sorted(missing))
    print()
    for k in sorted(have):
        assert lib.lipasr_debug_k3_launches(k) > 0
        worst = _worst.get(k)
        print(f"{K3_NAMES[k]}: {lib.lipasr_debug_k3_launches(k)} launches, first shown by {_ran[k]}" + (f"; worst error {worst[0]:.2e} ({worst[1]})" if worst else ""))
