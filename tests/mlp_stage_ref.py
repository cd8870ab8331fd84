"""Float64 references per stage of the training step's own kernels (test_mlp_stages_gpu.py, test_mlp_stages_cpu.py): K5 Adam + NonNeg,
BatchNorm statistics / apply / backward (the apply kernels and the exchange epilogue carry the same arithmetic) and the three softmax
forms.  NumPy only.  Every function returns the value and a per-element bound on |device - value|; dtype=np.float32 evaluates the same
steps in the kernel's order in single precision (the restatement the CPU companion holds inside the bound) and `wrong` names a
mutant (the CPU companion holds each outside it).  Hyper-parameters enter as the float32 values the C entry receives: 1 - b1 is the
float64 difference of the float32 b1, which is also what the kernel's fp32 `1.0f - b1` gives for b1 >= 0.5 (Sterbenz).

U = 2^-24 is one rounding to nearest (half an ulp, relative).  A sum of n fp32 terms in ANY order is within (n - 1) U sum|term| of
the exact sum (first order); a fused multiply-add has fewer roundings than the separate operations counted here, so contraction by
the compiler only helps.  TINY = 2^-126 is added wherever a result may be subnormal (a device may flush it).

Library functions: the HIP math API documents a maximum error of 1 ulp for expf, logf and sqrtf and a correctly rounded fp32
division by default; ULP_EXP, ULP_LOG, ULP_SQRT, ULP_DIV below are those figures with the division also taken as 1 ulp (an ulp is
at most 2 U relative).  None of them is read off a kernel's output.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
ULP_EXP = ULP_LOG = ULP_SQRT = ULP_DIV = 1.0
BN_EPS = float(np.float32(1e-3))
BN_MOM = float(np.float32(0.99))
TILE = 32  # rows per GEMM row tile whose column partial sums reach BatchNorm in fp32 (the 32 x 32 fragment tile the suite's shapes take)
ADAM_T = (0, 1, 9, 999, 100000)
ADAM_GSCALE = (1.0, 0.5, 1.0 / 3.0)
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-7)
ADAM_SEED = 11
# (widths, bn, nonneg): the small plans (segments that are no multiples of 4, padding behind W, b, gamma and beta, one workgroup) and
# the 2.27 M-parameter plan (more than 2048 x 256 quads: the stride loop's second trip) with the (t, gscale) pairs it runs at
ADAM_MODELS = {
    "nonneg-layer-0": ((5, 7, 3), (1, 0), (1, 0)),
    "nonneg-layer-1": ((5, 7, 3), (1, 0), (0, 1)),
    "stride-loop": ((1500, 1500, 10), (0, 0), (1, 1)),
}
ADAM_STRIDE_LOOP_CASES = ((0, 1.0), (9, 1.0 / 3.0), (100000, 0.5))


def f32(x):
    return float(np.float32(x))


# ====================================================================================================== layout
def align4(x):
    return (x + 3) & ~3


def segments(widths, bn, nonneg):
    """The flat parameter layout of lipasr_mlp_create restated: [(name, layer, start, count, clamp)], n_params.  Segments start at
    multiples of 4; the padding floats behind a segment take that segment's rule (the kernel looks a quad's rule up by its first
    float, and a quad never straddles a segment start)."""
    L = len(widths) - 1
    po, out = 0, []
    for l in range(L):
        ni, no = widths[l], widths[l + 1]
        out.append(("W", l, po, ni * no, bool(nonneg[l]))); po = align4(po + ni * no)
        out.append(("b", l, po, no, False)); po = align4(po + no)
        if l + 1 < L and bn[l]:
            out.append(("gamma", l, po, no, False)); po = align4(po + no)
            out.append(("beta", l, po, no, False)); po = align4(po + no)
    return out, po


def clamp_mask(segs, n_params):
    """per-float NonNeg rule, padding included"""
    mask = np.zeros(n_params, bool)
    for i, (_, _, start, _, clamp) in enumerate(segs):
        end = segs[i + 1][2] if i + 1 < len(segs) else n_params
        mask[start:end] = clamp
    return mask


def live_mask(segs, n_params):
    """True on parameters, False on the padding floats"""
    live = np.zeros(n_params, bool)
    for _, _, start, count, _ in segs:
        live[start:start + count] = True
    return live


# ====================================================================================================== K5 Adam + NonNeg
def adam_inputs(segs, n_params, seed, nonfinite=False):
    """(w, g, m, v) float32 [n_params]: |g|, |m| log-uniform in [1e-12, 1e3] with random signs, v log-uniform in [1e-24, 1e6], zeros
    in all three (an eighth each), w normal with scale 0.05; zeros on the padding.  In every segment of at least 6 floats the first
    floats are the edge rows: 0 g = m = v = 0 (the update is exactly 0), 1 the same at w = +0.0, 2 at w = -0.0 (x lands on -0.0),
    3 a weight the update drives negative; nonfinite: 4 a NaN gradient, 5 an inf gradient."""
    rng = np.random.default_rng(seed)
    n = n_params
    logu = lambda lo, hi: np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = logu(1e-12, 1e3) * sign() * (rng.random(n) >= 0.125)
    m = logu(1e-12, 1e3) * sign() * (rng.random(n) >= 0.125)
    v = logu(1e-24, 1e6) * (rng.random(n) >= 0.125)
    w = 0.05 * rng.standard_normal(n)
    for _, _, start, count, _ in segs:
        if count < 6:
            continue
        g[start:start + 3] = 0.0; m[start:start + 3] = 0.0; v[start:start + 3] = 0.0
        w[start] = 0.0371; w[start + 1] = 0.0; w[start + 2] = -0.0
        w[start + 3], g[start + 3], m[start + 3], v[start + 3] = 1e-4, 1.0, 1.0, 1e-4
        if nonfinite:
            g[start + 4], g[start + 5] = np.nan, np.inf
    out = [a.astype(np.float32) for a in (w, g, m, v)]
    live = live_mask(segs, n)
    for a in out:
        a[~live] = 0.0
    return out


def adam(w, g, m, v, t_word, lr, b1, b2, eps, gscale, clamp, dtype=np.float64, wrong=None):
    """One call of adam_nonneg_kernel on flat float32 arrays; t_word is the step word BEFORE the call (t = t_word + 1), clamp the
    per-float NonNeg rule.  Keras optimizer_v2 Adam as oracle/mlp_ref.adam_update states it, on g' = g gscale:
        m' = m b1 + g' (1 - b1);  v' = v b2 + g'^2 (1 - b2);  x = w - lr_t m' / (sqrt(v') + eps);  w' = clamp ? x (x >= 0) : x
        lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
    -> dict(w, m, v, x, bw, bm, bv).  The bounds, counted from the kernel (separate multiplies and adds; fused ones round less):
      g'   one rounding                                                                 1 U |g'|
      m'   two products, one sum, g' under the second product                           3 U (|m b1| + |g' (1-b1)|)           = bm
      v'   g' twice (2), g'g' (1), (1-b2) (1), the sum (1) on one term, 2 on the other; all terms >= 0      5 U v', taken as 6 = bv
      lr_t fp64 on the device, rounded once                                             1 U
      sqrtf(v')  half of v's 6 U, plus ULP_SQRT ulp = 2 U                               5 U
      + eps      one rounding                                                           6 U on the denominator
      lr_t m'    lr_t (1) and the product (1)                                           2 U, plus m's own bm
      the quotient  ULP_DIV ulp = 2 U                                                   10 U |lr_t m'| / (sqrt(v') + eps) in all
      w - ...    one rounding                                                           1 U |x|
      bw = U (2 |x| + lr_t (3 (|m b1| + |g' (1-b1)|) + 10 |m'|) / (sqrt(v') + eps)) + TINY
    (the factor 2 on |x| is a stated allowance, not a count; the clamp is 1-Lipschitz, so bw also bounds w').
    wrong: 't' (t one off), 'eps_in' (eps inside the root), 'eps_hat' (eps bias-corrected, textbook Adam), 'ob2_m' (1 - b2 on the
    first moment), 'gscale_once' (g' once under the square)."""
    lr, b1, b2, eps, gscale = (float(np.float32(a)) for a in (lr, b1, b2, eps, gscale))
    assert b1 >= 0.5 and b2 >= 0.5, "1.0f - b is exact only from 0.5 on"
    t = float(t_word + 1 + (1 if wrong == "t" else 0))
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    eps_eff = eps * np.sqrt(1.0 - b2 ** t) if wrong == "eps_hat" else eps
    dt = np.dtype(dtype).type
    w, g, m, v = (np.asarray(a, np.float32).astype(dtype) for a in (w, g, m, v))
    ob1, ob2 = dt(1.0 - (b2 if wrong == "ob2_m" else b1)), dt(1.0 - b2)
    with np.errstate(all="ignore"):
        gg = g * dt(gscale)
        t1, t2 = m * dt(b1), gg * ob1
        m1 = t1 + t2
        sq = (g * g) * dt(gscale) if wrong == "gscale_once" else gg * gg
        v1 = v * dt(b2) + sq * ob2
        den = np.sqrt(v1 + dt(eps_eff)) if wrong == "eps_in" else np.sqrt(v1) + dt(eps_eff)
        x = w - dt(lr_t) * m1 / den
        w1 = np.where(np.asarray(clamp, bool) & (x < 0), dt(0.0), x)
        bm = 3 * U * (np.abs(t1) + np.abs(t2)) + TINY
        bv = 6 * U * v1 + TINY
        bw = U * (2 * np.abs(x) + lr_t * (3 * (np.abs(t1) + np.abs(t2)) + 10 * np.abs(m1)) / den) + TINY
    return dict(w=w1, m=m1, v=v1, x=x, bw=bw, bm=bm, bv=bv)


ADAM_MUTANTS = ("t", "eps_in", "eps_hat", "ob2_m", "gscale_once")  # + the clamp on the wrong segment (another `clamp`)
# the two mutants that live in lr_t and eps sqrt(1 - b2^t) equal the reference to rounding once b^t has vanished
ADAM_BLIND = {("t", 100000), ("eps_hat", 100000)}


# ====================================================================================================== BatchNorm
def _tile_sums(x, tile, dtype):
    """column sums per row tile [tiles][N]: float64 exact, or fp32 row after row (one of the orders the bound allows)"""
    B = x.shape[0]
    out = []
    for r0 in range(0, B, tile):
        blk = x[r0:r0 + tile]
        if dtype == np.float64:
            out.append(blk.astype(np.float64).sum(axis=0))
        else:
            s = np.zeros(x.shape[1], np.float32)
            for row in blk:
                s = s + row
            out.append(s)
    return np.asarray(out)


def bn_stats(A, mmean, mvar, Bstat=None, tile=TILE, extra=0, dtype=np.float64, wrong=None):
    """Statistics of the device's own post-ReLU A [rows][N] float32 (the stacked shards under synchronized BatchNorm):
        mean = s1 / B, var = max(s2 / B - mean^2, 0) (population), rstd = 1 / sqrt(var + 1e-3f), moving' = moving 0.99f + stat (1 - 0.99f)
    -> dict(mean, var, rstd, mmean, mvar and b_mean, b_var, b_rstd, b_mmean, b_mvar).
    Propagation.  The device sums a and a a per row tile in fp32: a tile of T rows is within (T + 1) U sum|term| of its exact sum
    (T - 1 additions, one rounding of a a, one to spare), so over all tiles e1 = (tile + 1 + extra) U sum|a| and
    e2 = (tile + 1 + extra) U sum a^2; the tiles are then added in fp64 (exact at this precision).  extra: further fp32 roundings
    of a whole sum on its way (synchronized BatchNorm: the reduced partial is stored as fp32 and the shards are added in fp32: 2).
        d_mean = e1 / B                      b_mean = d_mean + U |mean|           (stored as fp32)
        d_var  = e2 / B + 2 |mean| d_mean + d_mean^2   (the clamp at 0 is 1-Lipschitz)      b_var = d_var + U var
        b_rstd = 0.5 (max(var - d_var, 0) + eps)^-1.5 d_var + U rstd     (|d rstd / d var| is largest at the low end of the interval)
        b_mmean = (1 - mom) b_mean + 3 U (|mmean mom| + |mean (1 - mom)|)   (two products, one sum), b_mvar likewise
    wrong: 'sample_var' (divide the squares' sum by B - 1 -- Bessel), 'mom_batch' (the momentum on the batch statistic),
    'eps_out' (1 / (sqrt(var) + eps))."""
    A = np.asarray(A, np.float32)
    B = int(Bstat or A.shape[0])
    k = tile + 1 + extra
    a64 = A.astype(np.float64)
    if dtype == np.float64:
        s1, s2 = a64.sum(axis=0), (a64 * a64).sum(axis=0)
    else:
        s1 = _tile_sums(A, tile, np.float32).astype(np.float64).sum(axis=0)
        s2 = _tile_sums(A * A, tile, np.float32).astype(np.float64).sum(axis=0)
    mean = s1 / B
    if wrong == "sample_var":
        var = np.maximum((s2 - B * mean * mean) / max(B - 1, 1), 0.0)
    else:
        var = np.maximum(s2 / B - mean * mean, 0.0)
    rstd = 1.0 / (np.sqrt(var) + BN_EPS) if wrong == "eps_out" else 1.0 / np.sqrt(var + BN_EPS)
    mom = 1.0 - BN_MOM if wrong == "mom_batch" else BN_MOM
    mm, mv = np.asarray(mmean, np.float32).astype(np.float64), np.asarray(mvar, np.float32).astype(np.float64)
    if dtype == np.float64:
        mm1, mv1 = mm * mom + mean * (1.0 - mom), mv * mom + var * (1.0 - mom)
    else:
        q = np.float32
        mean, var, rstd = mean.astype(q), var.astype(q), rstd.astype(q)
        mm1 = mm.astype(q) * q(mom) + mean * q(1.0 - mom)
        mv1 = mv.astype(q) * q(mom) + var * q(1.0 - mom)
    e1, e2 = k * U * np.abs(a64).sum(axis=0), k * U * (a64 * a64).sum(axis=0)
    mean64, var64 = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    d_mean = e1 / B
    d_var = e2 / B + 2 * np.abs(mean64) * d_mean + d_mean ** 2
    b_mean, b_var = d_mean + U * np.abs(mean64) + TINY, d_var + U * var64 + TINY
    b_rstd = 0.5 * (np.maximum(var64 - d_var, 0.0) + BN_EPS) ** -1.5 * d_var + U * np.asarray(rstd, np.float64)
    b_mm = (1 - BN_MOM) * b_mean + 3 * U * (np.abs(mm * BN_MOM) + np.abs(mean64 * (1 - BN_MOM))) + TINY
    b_mv = (1 - BN_MOM) * b_var + 3 * U * (np.abs(mv * BN_MOM) + np.abs(var64 * (1 - BN_MOM))) + TINY
    return dict(mean=mean, var=var, rstd=rstd, mmean=mm1, mvar=mv1, b_mean=b_mean, b_var=b_var, b_rstd=b_rstd, b_mmean=b_mm, b_mvar=b_mv)


def bn_apply(A, mean, rstd, gamma, beta, mask=None, dtype=np.float64):
    """H = ((a - mean) rstd gamma + beta) mask, fed the device's own float32 mean and rstd; mask: the inverted-dropout multipliers
    (0 or 1 / (1 - rate) as float32) or None -> (H, bound).  Roundings: a - mean (1, relative to |a| + |mean| so that cancellation is
    covered), two products (2), + beta (1 on the sum), the mask (1): bound = 5 U ((|a| + |mean|) rstd |gamma| + |beta|) |mask|.
    No BatchNorm (dropout only): H = a mask, one rounding -- pass mean = 0, rstd = 1, gamma = 1, beta = 0."""
    dt = dtype
    A, mean, rstd, gamma, beta = (np.asarray(a, np.float32).astype(dt) for a in (A, mean, rstd, gamma, beta))
    mk = np.ones_like(A) if mask is None else np.asarray(mask, np.float32).astype(dt)
    H = ((A - mean) * rstd * gamma + beta) * mk
    bound = 5 * U * ((np.abs(A) + np.abs(mean)) * np.abs(rstd * gamma) + np.abs(beta)).astype(np.float64) * np.abs(mk) + TINY
    return H, bound


def bn_bwd_sums(g, A, mean, rstd, tile=TILE, extra=0, dg=None, dtype=np.float64):
    """dbeta = sum_rows g, dgamma = sum_rows g xhat, xhat = (a - mean) rstd, from the device's g, A, mean, rstd (float32; g may be a
    float64 array formed by the caller, then dg is its per-element error) -> (dbeta, dgamma, b_dbeta, b_dgamma).
    dbeta: T - 1 additions per tile, the fp32 store and the grad_scale product: (tile + 2 + extra) U sum|g| + sum dg.
    dgamma: xhat costs 2 roundings relative to X = (|a| + |mean|) rstd, g xhat one more, then as above:
    (tile + 5 + extra) U sum |g| X + sum dg X."""
    A, mean, rstd = (np.asarray(a, np.float32) for a in (A, mean, rstd))
    X = (np.abs(A.astype(np.float64)) + np.abs(mean.astype(np.float64))) * rstd.astype(np.float64)
    g64 = np.asarray(g, np.float64)
    dgv = np.zeros_like(g64) if dg is None else np.asarray(dg, np.float64)
    if dtype == np.float64:
        xh = (A.astype(np.float64) - mean) * rstd.astype(np.float64)
        dbeta, dgamma = g64.sum(axis=0), (g64 * xh).sum(axis=0)
    else:
        g32 = np.asarray(g, np.float32)
        xh = (A - mean) * rstd
        dbeta = _tile_sums(g32, tile, np.float32).astype(np.float64).sum(axis=0).astype(np.float32)
        dgamma = _tile_sums(g32 * xh, tile, np.float32).astype(np.float64).sum(axis=0).astype(np.float32)
    b_db = (tile + 2 + extra) * U * np.abs(g64).sum(axis=0) + dgv.sum(axis=0) + TINY
    b_dg = (tile + 5 + extra) * U * (np.abs(g64) * X).sum(axis=0) + (dgv * X).sum(axis=0) + TINY
    return dbeta, dgamma, b_db, b_dg


def bn_bwd_dz(g, A, mean, rstd, gamma, dbeta, dgamma, Bstat, dg=None, dtype=np.float64, wrong=None):
    """dz = [a > 0] gamma rstd (g - dbeta / B - xhat dgamma / B), fed the device's own column sums (before grad_scale) -> (dz, bound).
    Roundings, with X = (|a| + |mean|) rstd >= |xhat|: 1 / B (1); dbeta / B (2 in all); xhat (2), xhat dgamma / B (5 in all); two
    subtractions (2 on every term); gamma rstd and the last product (2 on every term):
        bound = U |gamma rstd| (4 |g| + 6 |dbeta| / B + 9 X |dgamma| / B) + |gamma rstd| dg     (the counted constants, no allowance)
    wrong: 'no_rstd' (rstd missing from dz), 'no_dgamma' (the dgamma / B term dropped)."""
    dt = dtype
    A32 = np.asarray(A, np.float32)
    A, mean, rstd, gamma, dbeta, dgamma = (np.asarray(a, np.float32).astype(dt) for a in (A32, mean, rstd, gamma, dbeta, dgamma))
    gv = np.asarray(g, dt)
    invB = dt(1.0) / dt(Bstat) if dt != np.float64 else 1.0 / Bstat
    xh = (A - mean) * rstd
    t3 = np.zeros_like(xh) if wrong == "no_dgamma" else xh * dgamma * invB
    scale = gamma if wrong == "no_rstd" else gamma * rstd
    dz = np.where(A32 > 0, scale * (gv - dbeta * invB - t3), dt(0.0))
    a64, m64, r64 = A32.astype(np.float64), np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
    X = (np.abs(a64) + np.abs(m64)) * r64
    gr = np.abs(np.asarray(gamma, np.float64) * r64)
    dgv = 0.0 if dg is None else np.asarray(dg, np.float64)
    bound = gr * (U * (4 * np.abs(np.asarray(gv, np.float64)) + 6 * np.abs(np.asarray(dbeta, np.float64)) / Bstat
                       + 9 * X * np.abs(np.asarray(dgamma, np.float64)) / Bstat) + dgv) + TINY
    return dz, np.where(A32 > 0, bound, 0.0)


def g_from_next_layer(dz_next, W_next, mask=None):
    """The exchange path never stores g: g = (dz_{l+1} W_{l+1}^T) mask in float64 from the device's dz_{l+1} [B][K] and W_{l+1} [N][K],
    with the error of the device's K-term fp32 dot product and the mask product, (K + 1) U sum_k |dz W| |mask| -> (g, dg)."""
    dzn, Wn = np.asarray(dz_next, np.float64), np.asarray(W_next, np.float64)
    mk = 1.0 if mask is None else np.asarray(mask, np.float64)
    K = dzn.shape[1]
    return (dzn @ Wn.T) * mk, (K + 1) * U * (np.abs(dzn) @ np.abs(Wn).T) * np.abs(mk) + TINY


def bn_model(n_in, N, C, B, seed=0):
    """A two-layer model (n_in, N, C) with BatchNorm on layer 0 and a batch, all float32.  Layer 0's units: 0 dead (a = 0 in every
    row: zero weights, bias -1), 1 constant positive (zero weights, bias 0.75: zero variance), 2 offset (mean / std about 100),
    the rest ordinary."""
    rng = np.random.default_rng(500 + 1000 * N + B + seed)
    q = np.float32
    x = rng.standard_normal((B, n_in)).astype(q)
    W0 = (rng.standard_normal((n_in, N)) / np.sqrt(n_in)).astype(q)
    b0 = (0.2 * rng.standard_normal(N)).astype(q)
    W0[:, 0] = 0.0; b0[0] = -1.0
    if N > 1:
        W0[:, 1] = 0.0; b0[1] = 0.75
    if N > 2:
        W0[:, 2] *= q(0.1); b0[2] = 10.0
    gamma = (rng.uniform(0.5, 1.5, N) * np.where(rng.random(N) < 0.25, -1.0, 1.0)).astype(q)
    beta = (0.3 * rng.standard_normal(N)).astype(q)
    mmean, mvar = (0.1 * rng.standard_normal(N)).astype(q), rng.uniform(0.5, 2.0, N).astype(q)
    W1 = (rng.standard_normal((N, C)) / np.sqrt(N)).astype(q)
    b1 = (0.1 * rng.standard_normal(C)).astype(q)
    y = np.eye(C, dtype=q)[rng.integers(0, C, B)]
    return dict(x=x, W0=W0, b0=b0, gamma=gamma, beta=beta, mmean=mmean, mvar=mvar, W1=W1, b1=b1, y=y)


def dropout_masks(B, N, rate, seed):
    """injected inverted-dropout multipliers [B][N]: 0 or the float32 1 / (1 - rate)"""
    rng = np.random.default_rng(900 + seed)
    keep = rng.random((B, N)) >= rate
    return np.where(keep, np.float32(1.0) / (np.float32(1.0) - np.float32(rate)), np.float32(0.0)).astype(np.float32)


# (N, B) of the BatchNorm cases and the condition each is there for
BN_SHAPES = {
    (3, 7): "scalar lanes (N % 4 != 0), fewer than 8 rows, exactly the three special units",
    (3, 1): "one row: zero variance in every column",
    (33, 33): "scalar lanes with a ragged last quad, a second row tile of one row",
    (128, 7): "one full column strip of float4 lanes, fewer than 8 rows",
    (128, 77): "float4 lanes, three row tiles with a ragged last one",
    (132, 33): "a second column strip with ONE live lane (31 dead lanes still meet the barrier of sum_partials)",
    (132, 300): "ten row tiles: the second trip of the rl-strided loop over the partials, with the dead lanes",
    (33, 300): "ten row tiles on the scalar lanes",
}
BN_N_IN, BN_C, BN_RATE = 6, 3, 0.25

BN_MUTANTS = ("sample_var", "mom_batch", "eps_out", "no_rstd", "no_dgamma")


# ====================================================================================================== softmax
def _first_argmax(a):
    return np.argmax(a, axis=1)  # NumPy returns the first maximum


def softmax_ce(z, y=None, inv_batch=1.0, dtype=np.float64, wrong=None):
    """The device's own float32 logits z [B][C] (and labels y) -> dict(p, loss, dz, am, ay, correct, onehot, b_p, b_loss, b_dz):
        zs = z - max z;  se = sum exp(zs);  p = exp(zs) / se;  loss = -sum_{y != 0} y (zs - log se);  dz = (p - y) inv_batch;
        am, ay: the FIRST maximum of z and of y;  correct = [am == ay];  onehot = e_am
    Bounds, per row: zs is exact or one rounding (U |zs|, which exp turns into a relative U |zs|), expf ULP_EXP ulp:
        r_e(c) = (2 ULP_EXP + |zs_c|) U;   se: C terms in any order, r_se = (C - 1) U + max_c r_e(c);   1 / se: 2 U;  the product: 1 U
        b_p = 2 p (r_e + r_se + 3 U) + TINY            (the leading 2 is the stated safety factor; TINY: a flushed subnormal)
        log se: ULP_LOG ulp of |lse| plus r_se;  a term y (zs - lse): U |zs| + d_lse + 2 U |zs - lse|;  C additions:
        b_loss = 2 (sum |y| (U |zs| + r_se + 2 ULP_LOG U |lse| + 2 U |zs - lse|) + C U sum |y (zs - lse)|) + TINY
        b_dz = (b_p + 2 U |p - y|) |inv_batch|
    wrong: 'last_tie' (both argmax rules take the LAST maximum), 'log_p' (loss = -sum y log p with the float32 p)."""
    z32 = np.asarray(z, np.float32)
    B, C = z32.shape
    dt = dtype
    zz = z32.astype(dt)
    zs = zz - zz.max(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        e = np.exp(zs)
        if dt == np.float64:
            se = e.sum(axis=1, keepdims=True)
        else:
            se = np.zeros((B, 1), dt)
            for c in range(C):
                se = se + e[:, c:c + 1]
        lse = np.log(se)
        p = e * (dt(1.0) / se)
    out = dict(p=p)
    zs64, p64, lse64 = zs.astype(np.float64), p.astype(np.float64), lse.astype(np.float64)
    r_e = (2 * ULP_EXP + np.abs(zs64)) * U
    r_se = (C - 1) * U + r_e.max(axis=1, keepdims=True)
    out["b_p"] = 2 * p64 * (r_e + r_se + 3 * U) + TINY
    last = wrong == "last_tie"
    arg = (lambda a: a.shape[1] - 1 - np.argmax(a[:, ::-1], axis=1)) if last else _first_argmax
    out["am"] = arg(z32)
    out["onehot"] = np.eye(C, dtype=np.float32)[out["am"]]
    if y is not None:
        y32 = np.asarray(y, np.float32)
        yy = y32.astype(dt)
        with np.errstate(all="ignore"):
            if wrong == "log_p":
                terms = np.where(y32 != 0, yy.astype(np.float64) * np.log(p.astype(np.float32).astype(np.float64)), 0.0)
            else:
                terms = np.where(y32 != 0, yy * (zs - lse), dt(0.0))
        if dt == np.float64 or wrong == "log_p":
            loss = -terms.sum(axis=1)
        else:
            loss = np.zeros(B, dt)
            for c in range(C):
                loss = loss - terms[:, c]
        ya = np.abs(y32.astype(np.float64))
        out["loss"] = loss
        out["b_loss"] = 2 * ((ya * (U * np.abs(zs64) + r_se + 2 * ULP_LOG * U * np.abs(lse64) + 2 * U * np.abs(zs64 - lse64))).sum(axis=1)
                             + C * U * np.abs(ya * (zs64 - lse64)).sum(axis=1)) + TINY
        out["dz"] = (p - yy) * dt(np.float32(inv_batch))
        out["b_dz"] = (out["b_p"] + 2 * U * np.abs(p64 - y32)) * abs(float(np.float32(inv_batch))) + TINY
        out["ay"] = arg(y32)
        out["correct"] = (out["am"] == out["ay"]).astype(np.float32)
    return out


def softmax_vjp(z, v, on_logits, dtype=np.float64):
    """dz = v (on the logits) or p (v - p . v) (on the probabilities) from the device's float32 logits -> (dz, bound, p, b_p).
    p . v: C fused multiply-adds, d_dot = sum |v| b_p + C U sum |p v|;  v - dot (1), the product (1):
        bound = b_p |v - dot| + p (d_dot + 2 U |v - dot|) + TINY        (b_p carries softmax_ce's safety factor 2)"""
    s = softmax_ce(z, dtype=dtype)
    p, bp = s["p"], s["b_p"]
    v32 = np.asarray(v, np.float32)
    if on_logits:
        return v32.astype(dtype), np.zeros(v32.shape), p, bp
    vv = v32.astype(dtype)
    if dtype == np.float64:
        dot = (p * vv).sum(axis=1, keepdims=True)
    else:
        dot = np.zeros((p.shape[0], 1), dtype)
        for c in range(p.shape[1]):
            dot = dot + p[:, c:c + 1] * vv[:, c:c + 1]
    dz = p * (vv - dot)
    p64, v64, dot64 = p.astype(np.float64), v32.astype(np.float64), dot.astype(np.float64)
    C = p.shape[1]
    d_dot = (np.abs(v64) * bp).sum(axis=1, keepdims=True) + C * U * np.abs(p64 * v64).sum(axis=1, keepdims=True)
    bound = bp * np.abs(v64 - dot64) + p64 * (d_dot + 2 * U * np.abs(v64 - dot64)) + TINY
    return dz, bound, p, bp


SOFTMAX_MUTANTS = ("last_tie", "log_p")


def softmax_rows(C, B, seed=0):
    """Logit and label rows of the softmax cases, cycled over B rows -> (z, y) float32 [B][C].  Logit rows: random, all equal, a tie
    for the maximum at columns 3 and 7 (C > 7; else at the first and the last column), a spread of 87, a spread of 200 (p underflows
    to 0; the loss is 200 to rounding), one row at -1e4.  Label rows: one-hot, soft labels with a tie, all zero."""
    rng = np.random.default_rng(7000 + 100 * C + B + seed)
    z = (3.0 * rng.standard_normal((B, C))).astype(np.float32)
    y = np.zeros((B, C), np.float32)
    hi, lo = (3, 7) if C > 7 else (0, C - 1)
    for b in range(B):
        k = b % 6
        if k == 1:
            z[b] = np.float32(1.25)
        elif k == 2:
            z[b, hi] = z[b, lo] = np.float32(np.abs(z[b]).max() + 1.0)
        elif k == 3:
            z[b] = np.linspace(0.0, 87.0, C, dtype=np.float32)[rng.permutation(C)] if C > 1 else np.float32(87.0)
        elif k == 4:
            z[b] = np.float32(-100.0)
            z[b, (b // 6) % C] = np.float32(100.0)
            if C > 1:  # the label sits on a class whose probability underflows
                y[b, ((b // 6) + 1) % C] = 1.0
        elif k == 5:
            z[b] = np.float32(-1e4)
        j = (b // 6) % 3
        if k == 4 and C > 1:
            continue
        if j == 0:
            y[b, rng.integers(C)] = 1.0
        elif j == 1:
            y[b] = 0.1 / C
            y[b, hi] += 0.45
            y[b, lo] = y[b, hi]
    return z, y
