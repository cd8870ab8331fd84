"""Every kernel instance of the MFCC backward pass stage by stage against float64, and proof of which kernels ran.

The pattern of test_mfcc_instances_gpu.py (whose Buf / Plan machinery is reused as it is), through the raw C entry points with ctypes:

  * memory: sig, g_feat, g_sig, n_valid and every hook destination live in a buffer of their own between sentinels; plans are made
    with batch_max > batch, so rows >= batch of g_sig and of the hook destinations hold sentinels too; "off" arrays start one float
    off a 16-byte boundary wherever include/lipasr.h allows it (the one-length and short-window entries: all three arrays; the ragged
    entry: g_feat and g_sig -- its rows must be aligned, and the refusal of misaligned rows is asserted by return code).
  * kernels: every case names the counters of lipasr_debug_k1_vjp_launches that must move and by how much, written out by hand from
    plan_vjp and the launchers; exactly those move.  The last test fails when the library knows an id that no case claims and prints
    (-s) per kernel the first case that ran it, its worst error as a fraction of its bound and the device / yardstick ratio.
  * determinism: each case runs twice into fresh buffers, bit for bit; then the forward is run by the caller and the backward reuses
    it (flags bit 0): the same bits again.  The forward counters (lipasr_debug_k1_launches) say what each call ran: without the flag
    the resampler (domain 0) and the backward's own STFT kernel; with it no resampler, and on a default 2048/512 plan
    stft_mel2_kernel again (the block-DFT tile is never read), on a plan with stage-mask bit 256 and on short-window plans no
    forward kernel at all.  The one-length and ragged cases run on both kinds of plan, with the same bits.
  * stage 1: the device's own dB tile and frame maxima (lipasr_debug_mfcc_stage) and Gmel (lipasr_debug_mfcc_vjp_stage) against
    mfcc_vjp_stage_ref.stage1, per element |got - ref| <= F1 2^-24 A, exactly 0 where the reference is exactly 0.  Ties and elements on
    the floor come from tiles poked into the plan (lipasr_debug_mfcc_stage_put) and read with flags bit 0.
  * stages 2+3: the device's g_y (g_sig for domain 1, the hook for domain 0) against mfcc_vjp_stage_ref.stage23 fed the DEVICE's
    Gmel and the signal the device read, in the metric of mfcc_grad_ref.errs; bound F2 x the float32 restatement's error, the worst
    clip of the case; samples reached only by frames with a zero cotangent are exactly 0.
  * stage 4: g_sig against the explicit float64 R^T of the device's g_y over the fp32 taps of lipasr_debug_table, per element
    (nt + 1) 2^-24 sum |h| |g_y|; and combs of unit impulses, whose every g_x sample is one fp32 tap or 0 bit for bit.
  * end to end: 8 x the float32 autograd oracle (the statement of test_wave_attacks_gpu.py), on the clips of a case that pass
    guard_margins (>= 1e-2 dB from the floor and from a tie).  The clips that do not are printed per case and listed by the last
    test, and are checked stage by stage only: on the MI355X clip 0 of one-22050-2205-L44-d0 and, by construction, every poked
    tile.

UNREACHABLE lists the instances no public entry reaches, with the reason and a test that the only route is refused.

What the end-to-end statement found (MI355X figures; DESIGN.md 3, "Backward pass", has the whole account).  On the burst clips (1e-5
noise with a full-scale burst of ~100 samples centred on one frame; they pass guard_margins) the gradient was 3.7e-05 from float64
where the bound was 3.2e-05 (one-3000-L4-d1; ragged-8000-d1-f32 7.3e-05 against 7.1e-05), with every backward stage inside its bound
against the DEVICE's tile: the excess came in with the forward's dB tile, which 1 / mel magnifies.  stft_bdft_kernel windows in the
frequency domain and a burst under the tail of a window cancels a large spectrum down to a small one (worst frame 9.8e-06 and 1.2e-05
of its peak from float64, 49 and 86 x the float32 yardstick); stft_mel2_kernel sent frames of any loudness through one packed
transform (1.5e-05).  The backward pass now runs stft_mel2_kernel for its own tile, with every frame scaled by its own power of two,
and reuses a caller's forward only where that kernel ran it: the same clips are 5.3e-06 .. 8.4e-06 from float64 (tile 1.3e-06 ..
1.8e-06), and no clip of any case is above 0.36 of the end-to-end bound.  Each case prints, per clip, the tile's stage-B figure
(tests/mfcc_stage_ref.py) next to its float32 yardstick.
"""
import functools

import numpy as np
import pytest
import torch

import mfcc_grad_ref as G
import mfcc_stage_ref as S
import mfcc_vjp_stage_ref as V
import test_mfcc_instances_gpu as F

pytestmark = pytest.mark.gpu
Buf, Plan, SENTINEL = F.Buf, F.Plan, F.SENTINEL

# kernel ids of lipasr_debug_k1_vjp_launches (include/lipasr.h)
DB, DB_R, STFT, STFT_R, FOLD, FOLD_R, RS8, RS1, RS8_R, RS1_R, COPY_CUT, DFT, DFT_FOLD = range(13)
KV_NAMES = ("mfcc_vjp_db_kernel<false>", "mfcc_vjp_db_kernel<true>", "stft_vjp_kernel<false>", "stft_vjp_kernel<true>",
            "stft_vjp_fold_kernel<false>", "stft_vjp_fold_kernel<true>", "resample_vjp_kernel<8,false>", "resample_vjp_kernel<1,false>",
            "resample_vjp_kernel<8,true>", "resample_vjp_kernel<1,true>", "copy_cut_kernel", "dft_vjp_kernel", "dft_vjp_fold_kernel")
UNREACHABLE = {
    RS1_R: "resample_vjp_kernel<1,true> serves per-clip lengths at a rate whose 8-output window of g_y exceeds 60 KiB of LDS; "
           "lipasr_mfcc_plan_vjp_ragged, the only entry that passes lengths, refuses every plan that is not 16 kHz or 8 kHz, and both "
           "take the 8-output form (test_the_only_route_to_the_unreachable_instance_is_refused)",
}
F2_FAMILY = {STFT: "stft", STFT_R: "stft", FOLD: "stft", FOLD_R: "stft", DFT: "dft", DFT_FOLD: "dft"}

# the clips that fail guard_margins on the MI355X and are therefore checked stage by stage only (every other clip of every case is held
# to the end-to-end bound too); the poked-tile cases are stage-checked by construction
STAGE_ONLY = {"one-22050-2205-L44-d0": [0]}

_ran, _worst = {}, {}
_stage_only = {}  # case -> the clips that fail guard_margins (stage-checked only)


def _native():
    from lipasr import _native as N

    return N


def _snapshot():
    lib = _native().lib
    return [lib.lipasr_debug_k1_vjp_launches(k) for k in range(len(KV_NAMES))], F._snapshot()


RESAMPLERS = set(range(F.H2_F32, F.CLEAR_TAIL + 1))  # forward ids 0 .. 9: the resamplers, copy_pad_kernel, clear_tail_kernel


def _assert_moved(before, expect, what, forward_may_run=False, fwd=None):
    """expect: the backward counters that move.  fwd: None (not judged), or (resampler ran, id of the STFT kernel that ran or None): the
    forward counters a backward call moves when it re-runs, or reuses, the forward."""
    now = _snapshot()
    moved = {k: a - b for k, (b, a) in enumerate(zip(before[0], now[0])) if a != b}
    names = lambda d: {KV_NAMES[k]: v for k, v in d.items()}
    assert moved == expect, f"{what}: launched {names(moved)}, the case is meant to launch {names(expect)}"
    fmoved = {k: a - b for k, (b, a) in enumerate(zip(before[1], now[1])) if a != b}
    if not expect and not forward_may_run:  # a refusal launches nothing at all, forward kernels included
        assert not fmoved, f"{what}: a refused call launched forward kernels"
    if fwd is not None:
        fnames = {F.K1_NAMES[k]: v for k, v in fmoved.items()}
        rs = {k: v for k, v in fmoved.items() if k in RESAMPLERS}
        rest = {k: v for k, v in fmoved.items() if k not in RESAMPLERS}
        assert bool(rs) == fwd[0] and all(v == 1 for v in rs.values()), f"{what}: forward kernels {fnames}; a resampler is {'' if fwd[0] else 'not '}meant to run"
        assert rest == ({fwd[1]: 1} if fwd[1] is not None else {}), f"{what}: forward kernels {fnames}; the STFT meant to run: {fwd[1]}"


def _record(case, kernels, frac, ratio=None):
    for k in kernels:
        _ran.setdefault(k, case)
        if k not in _worst or frac > _worst[k][0]:
            _worst[k] = (frac, case, ratio)


def _vstage(plan, which, batch):
    """lipasr_debug_mfcc_vjp_stage into a guarded destination laid out for batch_max rows"""
    N = _native()
    dst = Buf({0: (plan.batch_max, plan.n_frames, 128), 1: (plan.batch_max, plan.n_y)}[which])
    N.check(N.lib.lipasr_debug_mfcc_vjp_stage(plan.h, which, batch, dst.ptr(), N.stream_ptr()))
    torch.cuda.synchronize()
    return dst.read(batch)


def _vjp(plan, entry, sig, fmt, nv, domain, batch, L, scale, gfeat, gsig, flags):
    N = _native()
    lib, s, sc = N.lib, N.stream_ptr(), N.ptr(scale)
    if entry == "ragged":
        return lib.lipasr_mfcc_plan_vjp_ragged(plan.h, sig.ptr(), fmt, nv.ptr(), domain, batch, L, sc, gfeat.ptr(), gsig.ptr(), flags, s)
    fn = lib.lipasr_mfcc_plan_vjp if entry == "one" else lib.lipasr_mfcc_plan_vjp_short
    return fn(plan.h, sig.ptr(), domain, batch, L, sc, gfeat.ptr(), gsig.ptr(), flags, s)


def _forward(plan, entry, sig, fmt, nv, domain, batch, L):
    """the caller's forward that flags bit 0 refers to"""
    N = _native()
    out = Buf((plan.batch_max, 20 * L))
    nvp = nv.ptr() if nv is not None else None
    if domain == 0:
        N.check(N.lib.lipasr_mfcc_extract(plan.h, sig.ptr(), fmt, nvp, batch, L, None, None, out.ptr(), N.stream_ptr()))
    elif nv is not None:
        N.check(N.lib.lipasr_mfcc_plan_from_22k_ragged(plan.h, sig.ptr(), nvp, batch, L, None, None, out.ptr(), N.stream_ptr()))
    else:
        N.check(N.lib.lipasr_mfcc_plan_from_22k(plan.h, sig.ptr(), batch, plan.n_y, L, None, None, out.ptr(), N.stream_ptr()))
    torch.cuda.synchronize()
    out.read(batch)


def _run(plan, entry, rows, g_feat, L, scale, domain, expect, case, nv=None, fmt=0, offs=(False, False, False), flags=0, forward=False,
         poke=None, fwd=None):
    """One backward call from fresh guarded buffers -> dict of g_sig and the plan's intermediates, rows < batch"""
    N = _native()
    batch, width = rows.shape[0], (plan.n if domain == 0 else plan.n_y)
    assert rows.shape[1] == width
    sig = Buf(rows.shape, rows, offs[0], np.int16 if fmt else np.float32)
    gf = Buf(g_feat.shape, g_feat, offs[1])
    gs = Buf((plan.batch_max, width), None, offs[2])
    nvb = Buf((batch,), nv, False, np.int32) if nv is not None else None
    sc = F._dev64(scale)
    if forward:
        _forward(plan, entry, sig, fmt, nvb, domain, batch, L)
    if poke is not None:
        for which, arr in enumerate(poke):
            src = Buf(arr.shape, arr)
            N.check(N.lib.lipasr_debug_mfcc_stage_put(plan.h, which, batch, src.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            src.read()
    before = _snapshot()
    N.check(_vjp(plan, entry, sig, fmt, nvb, domain, batch, L, sc, gf, gs, flags))
    torch.cuda.synchronize()
    _assert_moved(before, expect, case, fwd=fwd)
    sig.read(), gf.read()
    if nvb is not None:
        nvb.read()
    res = dict(g_sig=gs.read(batch), db=plan.stage(0, batch), fmax=plan.stage(1, batch), gmel=_vstage(plan, 0, batch))
    if domain == 0:
        res["y"], res["gy"] = plan.stage(2, batch), _vstage(plan, 1, batch)
    else:
        res["gy"] = res["g_sig"]
    return res


def _run_case(plan, entry, rows, g_feat, L, scale, domain, expect, case, frames, **kw):
    """Twice bit for bit, then the caller's forward and flags bit 0: the same bits; returns the first run.  The forward counters say
    what each call ran: without the flag the resampler (domain 0) and the backward's own STFT kernel (stft_mel2_kernel, dft_mel_kernel on
    short-window plans); with it no resampler, and the STFT again only where the caller's forward was another kernel than that one (a
    2048/512 plan without stage-mask bit 256)."""
    stft = F.DFT if entry == "short" else F.MEL2
    tile_reused = entry == "short" or bool(plan.mask & 256)
    a = _run(plan, entry, rows, g_feat, L, scale, domain, expect, case, fwd=(domain == 0, stft), **kw)
    b = _run(plan, entry, rows, g_feat, L, scale, domain, expect, case + " (second run)", fwd=(domain == 0, stft), **kw)
    c = _run(plan, entry, rows, g_feat, L, scale, domain, expect, case + " (caller's forward, flags bit 0)", flags=1, forward=True,
             fwd=(False, None if tile_reused else stft), **kw)
    for other, what in ((b, "two runs from the same inputs"), (c, "the re-run and the reused forward")):
        assert F._same_bits(a["g_sig"], other["g_sig"]) and F._same_bits(a["gy"], other["gy"]), f"{case}: {what} differ"
        for u, T in enumerate(frames):  # (ragged: frames past a clip's own hold what an earlier call left)
            assert F._same_bits(a["gmel"][u, :T], other["gmel"][u, :T]), f"{case}: {what} differ in Gmel of clip {u}"
    return a


# ====================================================================================================== clips
def _clip(kind, n, rate, seed=0):
    """n samples at `rate` (float64).  case: chirp + noise + edge tones; quiet: the same 60 dB down; loud-last: S.loud_last_clip; zeros;
    ('burst', f): 1e-5 noise with a full-scale burst of ~100 resampled samples centred on frame f of the 2048/512 grid."""
    if kind == "zeros" or n == 0:
        return np.zeros(n)
    if kind == "case":
        return V.case_clip(n, seed).astype(np.float64)
    if kind == "quiet":
        return 1e-3 * V.case_clip(n, seed + 1).astype(np.float64)
    if kind == "loud-last":
        return S.loud_last_clip(n, seed).astype(np.float64) if n > 105 else V.case_clip(n, seed).astype(np.float64)
    rng = np.random.default_rng(3000 + n + seed)
    y = 1e-5 * rng.standard_normal(n)
    c, h = int(kind[1] * 512 * rate / V.SR), max(2, int(50 * rate / V.SR))
    y[c - h:c + h] = rng.uniform(-1.0, 1.0, 2 * h)
    return y


def _check(case, res, plan, entry, rows, fmt, lens, g_feat, L, scale, domain, kernels, sr, n_fft=2048, hop=512, e2e=True):
    """Every stage of one case.  lens: per clip the samples at the plan's input rate; kernels: (stage-1 id, stage-2 id, stage-3 id, stage-4
    id or None).  Every figure is printed before anything about it is asserted."""
    k1, k2, k3, k4 = kernels
    ragged = entry == "ragged"
    fam = F2_FAMILY[k2]
    f1, f2 = V.F1, V.F2[fam]
    assert f1 <= V.F_MAX and f2 <= V.F_MAX
    sigf = rows.astype(np.float32) / np.float32(32768.0) if fmt else rows.astype(np.float32)
    tab = _tables(sr) if (domain == 0 and sr != V.SR) else None
    clips, r1, yard = [], 0.0, [0.0, 0.0]
    for u, n in enumerate(lens):
        if n_fft == 2048:
            n_vy, c_y, T = V.clip_lengths(n, sr)
            T = min(T, plan.n_frames)
        else:
            n_vy, c_y, T = plan.n_y, plan.n_y, plan.n_frames
        # ---- stage 1
        ref, A = V.stage1(res["db"][u], res["fmax"][u], g_feat[u], L, T, scale)
        got = res["gmel"][u, :T].astype(np.float64)
        err = np.abs(got - ref)
        live = A > 0.0
        ratio1 = float((err[live] / (V.U * A[live])).max()) if live.any() else 0.0
        r1 = max(r1, ratio1)
        at = np.unravel_index((err - f1 * V.U * A).argmax(), err.shape) if T else (0, 0)
        print(f"\n{case}: clip {u} ({n} samples, {T} frames): stage 1 worst |got - ref| / (2^-24 A) = {ratio1:.2f} (factor {f1:g})", end="")
        assert T == 0 or (err <= f1 * V.U * A).all(), f"{case}: clip {u}: Gmel[frame, mel {at}] = {got[at]:.9e}, float64 {ref[at]:.9e}, bound {f1 * V.U * A[at]:.3e}"
        assert not got[ref == 0.0].any(), f"{case}: clip {u}: Gmel is not exactly 0 where the reference is"
        # ---- stages 2 + 3
        gy = res["gy"][u].astype(np.float64)
        assert not gy[c_y:].any(), f"{case}: clip {u}: g_y is not exactly 0 past the clip's end {c_y}"
        if c_y < 2:
            clips.append(None)
            assert not res["g_sig"][u].any()
            continue
        y = (res["y"][u] if domain == 0 else sigf[u]).astype(np.float64)[:c_y].copy()
        if ragged:
            y[n_vy:] = 0.0  # fix_length's zero, whatever the row holds there
        ref2, reached = V.stage23(y, res["gmel"][u, :T], n_fft, hop)
        assert not gy[:c_y][~reached].any(), f"{case}: clip {u}: a sample reached only by zero-cotangent frames is not exactly 0"
        if not ref2.any():
            assert not gy.any() and not res["g_sig"][u].any(), f"{case}: clip {u}: a zero cotangent (or clip) gives a non-zero gradient"
            clips.append(None)
            continue
        y32 = V.errs(V.stage23(y, res["gmel"][u, :T], n_fft, hop, dtype=torch.float32)[0], ref2)
        dev = V.errs(gy[:c_y], ref2)
        yard = [max(yard[0], y32[0]), max(yard[1], y32[1])]
        clips.append((dev, y32))
        print(f"; stages 2+3 device inf {dev[0]:.3e} two {dev[1]:.3e}, float32 restatement inf {y32[0]:.3e} two {y32[1]:.3e}", end="")
        # ---- stage 4
        if domain == 0:
            gs = res["g_sig"][u].astype(np.float64)
            assert not gs[n:].any(), f"{case}: clip {u}: g_sig is not exactly 0 past the clip's end {n}"
            ref4, mag = V.resample_vjp(res["gy"][u], n, sr, tab)
            bound4 = (_nt(sr) + 1) * V.U * mag if tab is not None else np.zeros(n)
            e4 = np.abs(gs[:n] - ref4)
            frac4 = float((e4[mag > 0] / bound4[mag > 0]).max()) if tab is not None and (mag > 0).any() else 0.0
            print(f"; stage 4 worst {frac4:.3f} of the a-priori bound", end="")
            assert (e4 <= bound4).all(), f"{case}: clip {u}: g_sig is {e4.max():.3e} from R^T g_y"
            _record(case, [k4], frac4)
    print()
    r2 = 0.0
    for u, c in enumerate(clips):
        if c is None:
            continue
        dev, _ = c
        r2 = max(r2, dev[0] / yard[0], dev[1] / yard[1])
    print(f"{case}: stage 1 device / yardstick {r1:.2f} (factor {f1:g}); stages 2+3 device / float32 restatement {r2:.2f} (factor {f2:g}, yardstick "
          f"inf {yard[0]:.3e} two {yard[1]:.3e})")
    for u, c in enumerate(clips):
        if c is not None:
            assert c[0][0] <= f2 * yard[0] and c[0][1] <= f2 * yard[1], f"{case}: clip {u}: g_y is {c[0]} from float64, bound {f2:g} x {yard}"
    _record(case, [k1], r1 / f1, r1)
    _record(case, [k2, k3], r2 / f2, r2)
    # ---- end to end: 8 x the float32 autograd oracle, on the clips that keep clear of the floor and of ties
    if not e2e:
        return
    rowsE, skipped = [], []
    for u, n in enumerate(lens):
        if clips[u] is None:
            continue
        n_vy, c_y, T = V.clip_lengths(n, sr) if n_fft == 2048 else (plan.n_y, plan.n_y, plan.n_frames)
        y = (res["y"][u] if domain == 0 else sigf[u]).astype(np.float64)[:c_y].copy()
        if ragged:
            y[n_vy:] = 0.0
        to_floor, gap, _ = G.guard_margins(y, n_fft, hop)
        P64, yard_b, _ = S.stage_b_reference(y.astype(np.float32), n_fft, hop)  # (reported only: the forward tile this backward read)
        loud = ~S.silent_frames(P64)
        if loud.any():
            tile_b = S.frame_metric(S.db_to_power(res["db"][u, :T]), P64)[loud]
            print(f"{case}: clip {u}: forward tile: worst frame {tile_b.max():.3e} of its peak from float64, float32 yardstick {yard_b[loud].max():.3e}; "
                  f"closest element to the floor {to_floor:.2e} dB, top gap {gap:.2e} dB")
        if min(to_floor, gap) < 1e-2:
            skipped.append(u)
            continue
        end = n if domain == 0 else c_y
        x = sigf[u, :end].astype(np.float64)
        if ragged and domain == 1:
            x[n_vy:] = 0.0
        row = G.parity_row(res["g_sig"][u, :end].astype(np.float64), x, g_feat[u], sr_in=sr, utterance_length=L, scale=scale,
                           domain="input" if domain == 0 else "22k", n_fft=n_fft, hop=hop)
        rowsE.append((u,) + row[:2])
    _stage_only[case] = skipped
    assert skipped == STAGE_ONLY.get(case, []), f"{case}: clips {skipped} fail guard_margins, expected {STAGE_ONLY.get(case, [])}"
    print(f"{case}: clips checked stage by stage only (they fail guard_margins): {skipped}")
    if rowsE:
        y8 = (8 * max(r[2][0] for r in rowsE), 8 * max(r[2][1] for r in rowsE))
        for u, dev, y32 in rowsE:
            print(f"{case}: clip {u} end to end: device inf {dev[0]:.3e} two {dev[1]:.3e} | float32 oracle inf {y32[0]:.3e} two {y32[1]:.3e} | bounds {y8[0]:.3e} / {y8[1]:.3e}")
        for u, dev, _ in rowsE:
            assert dev[0] <= y8[0] and dev[1] <= y8[1], (case, u, dev, y8)


@functools.lru_cache(maxsize=None)
def _tables(sr):
    N = _native()
    return V.polyphase_from_tables(N.debug_table(3, sr), N.debug_table(4, sr), N.debug_table(5, sr))


@functools.lru_cache(maxsize=None)
def _nt(sr):
    return V.adjoint_taps(_tables(sr))


def _cotangent(batch, L, seed=0):
    g, scale = V.case_cotangent(L, seed)
    rng = np.random.default_rng(500 + seed)
    return np.stack([g] + [rng.standard_normal(20 * L).astype(np.float32) for _ in range(batch - 1)]), scale


# ====================================================================================================== 2048/512, one length
# id: (sr, n, L, domain, scale?, offs (sig, g_feat, g_sig), clip kinds, counters)
ONE_KERNELS = {0: (DB, STFT, FOLD, RS8), 1: (DB, STFT, FOLD, None)}
KINDS = {1487: ("case", "loud-last", "zeros"), 3000: ("case", ("burst", 5), ("burst", 6)), 7000: ("case", "loud-last", "quiet")}
ONE_CASES = {}
for _n in V.ONE_LENGTH_N:
    for _L in (4, 44):
        for _dom in (0, 1):
            _exp = {DB: 1, STFT: 1, FOLD: 1, RS8: 1} if _dom == 0 else {DB: 1, STFT: 1, FOLD: 1}
            ONE_CASES[f"one-{_n}-L{_L}-d{_dom}"] = (16000, _n, _L, _dom, (_L == 4) == (_dom == 0), (_dom == 1, True, _dom == 1 or _L == 44), KINDS[_n], _exp)
ONE_CASES["one-8k-1500-L44-d0"] = (8000, 1500, 44, 0, True, (True, True, True), ("case", "loud-last", "zeros"), {DB: 1, STFT: 1, FOLD: 1, RS8: 1})
ONE_CASES["one-22050-2205-L44-d0"] = (22050, 2205, 44, 0, False, (True, True, True), ("case", "loud-last", "zeros"), {DB: 1, STFT: 1, FOLD: 1, COPY_CUT: 1})
# 16 010 Hz: up 2205, down 1601: the 8-output window of g_y is (7 x 2205 + span) floats > 60 KiB, so the one-output form runs, and
# 1601 phases need gridDim.z = 2 workgroups of 1024 threads
ONE_CASES["one-16010-3300-L44-d0"] = (16010, 3300, 44, 0, True, (True, True, True), ("case", "loud-last", "zeros"), {DB: 1, STFT: 1, FOLD: 1, RS1: 1})


@pytest.mark.parametrize("case", list(ONE_CASES))
def test_one_length(cuda, case):
    """lipasr_mfcc_plan_vjp, batch 3 of batch_max 4.  L = 4: frames >= 4 have a zero cotangent and are skipped, except the frame of the
    clip maximum, which receives the floored sum: the last, unpaired frame of the loud-last clips (frame a alone), frame 5 of a burst clip
    (frame a of its pair zero, frame b not) and frame 6 of the other (the reverse)."""
    sr, n, L, domain, use_scale, offs, kinds, expect = ONE_CASES[case]
    with Plan(sr, n, 4) as plan:
        width = n if domain == 0 else plan.n_y
        rate = sr if domain == 0 else V.SR
        rows = np.stack([_clip(k, width, rate, u) for u, k in enumerate(kinds)]).astype(np.float32)
        g_feat, scale = _cotangent(3, L, n)
        scale = scale if use_scale else None
        T = plan.n_frames
        res = _run_case(plan, "one", rows, g_feat, L, scale, domain, expect, case, [T] * 3, offs=offs)
        # the same on a plan whose forward is stft_mel2_kernel (stage-mask bit 256): flags bit 0 then reuses the tile too -- no forward
        # kernel runs -- and every run has the bits of the default plan's
        with Plan(sr, n, 4, keys=((0, 256),)) as plan2:
            res2 = _run_case(plan2, "one", rows, g_feat, L, scale, domain, expect, case + " (stage-mask bit 256)", [T] * 3, offs=offs)
        assert F._same_bits(res["g_sig"], res2["g_sig"]) and F._same_bits(res["gmel"], res2["gmel"]), f"{case}: the two plans differ"
        kern = ONE_KERNELS[domain][:3] + ((RS1 if RS1 in expect else COPY_CUT if COPY_CUT in expect else RS8) if domain == 0 else None,)
        _check(case, res, plan, "one", rows, 0, [n] * 3, g_feat, L, scale, domain, kern, sr)
    live = (res["gmel"] != 0.0).any(axis=2)  # [3][T]
    for u, k in enumerate(kinds):
        if L == 4 and k == "loud-last":
            assert int(res["fmax"][u].argmax()) >= L and live[u, 4:].sum() == 1, (case, u, live[u])
            assert (res["gmel"][u, 4:] != 0.0).sum() == 1  # the floored sum, on the maximum alone
        if L == 4 and isinstance(k, tuple):
            f = k[1]
            assert int(res["fmax"][u].argmax()) == f and live[u, 4:].tolist() == [t == f for t in range(4, T)], (case, u, live[u])
        if k == "zeros":
            assert not res["g_sig"][u].any() and not res["gmel"][u].any()


def test_a_plan_of_stft_mel_kernel_is_not_reused_either(cuda):
    """Stage-mask bit 64: the plan's forward is stft_mel_kernel, two frames of any loudness in one transform.  The backward pass runs
    stft_mel2_kernel for itself, with flags bit 0 too (the forward counters say so), and the burst clips meet every bound."""
    case, n, L = "round2-3000-L4-d1", 3000, 4
    expect = {DB: 1, STFT: 1, FOLD: 1}
    with Plan(16000, n, 4, keys=((0, 64),)) as plan:
        rows = np.stack([_clip(k, plan.n_y, V.SR, u) for u, k in enumerate(KINDS[n])]).astype(np.float32)
        g_feat, scale = _cotangent(3, L, n)
        res = _run_case(plan, "one", rows, g_feat, L, scale, 1, expect, case, [plan.n_frames] * 3, offs=(True, True, True))
        _check(case, res, plan, "one", rows, 0, [n] * 3, g_feat, L, scale, 1, ONE_KERNELS[1], 16000)


# ====================================================================================================== 2048/512, per-clip lengths
RAG_ROW = {16000: 7000, 8000: 3500}
RAG_KINDS = ("zeros", "case", "case", "case", "case", "loud-last", ("burst", 5), "case", "zeros")


# (int16 rows are rows at the input rate: int16 with domain 1 is a refusal, asserted in test_ragged_refusals)
@pytest.mark.parametrize("sr,domain,fmt", [(sr, d, f) for sr in (16000, 8000) for d, f in ((0, 0), (1, 0), (0, 1))])
def test_ragged(cuda, sr, domain, fmt):
    """lipasr_mfcc_plan_vjp_ragged: 0 samples, 2 (3) resampled samples, repeated reflection (vj_fold_any), either side of the three-term
    fold, 9 frames, the full row and an all-zero clip in one launch, 9 of batch_max 10; rows hold 10 x noise past each clip's end."""
    n_row = RAG_ROW[sr]
    lens = list(V.RAGGED_NV[sr]) + [V.RAGGED_NV[sr][6]]
    L = 6 if domain else 44
    case = f"ragged-{sr}-d{domain}-{'i16' if fmt else 'f32'}"
    expect = {DB_R: 1, STFT_R: 1, FOLD_R: 1, RS8_R: 1} if domain == 0 else {DB_R: 1, STFT_R: 1, FOLD_R: 1}
    with Plan(sr, n_row, 10) as plan:
        width = n_row if domain == 0 else plan.n_y
        rng = np.random.default_rng(sr + domain)
        rows = (10.0 * rng.standard_normal((9, width))).astype(np.float32) if not fmt else rng.integers(-30000, 30000, (9, width)).astype(np.float32)
        frames = []
        for u, (n, k) in enumerate(zip(lens, RAG_KINDS)):
            n_vy, c_y, T = V.clip_lengths(n, sr)
            frames.append(T)
            m = n if domain == 0 else n_vy
            clip = _clip(k, m, sr if domain == 0 else V.SR, u)
            rows[u, :m] = np.clip(np.round(clip * 32767.0), -32768, 32767) if fmt else clip
        assert frames == [0, 1, 1, 2, 5, 5, 9, 19, 9]
        dev_rows = rows.astype(np.int16) if fmt else rows
        g_feat, scale = _cotangent(9, L, sr)
        res = _run_case(plan, "ragged", dev_rows, g_feat, L, scale, domain, expect, case, frames, nv=lens, fmt=fmt, offs=(False, True, True))
        with Plan(sr, n_row, 10, keys=((0, 256),)) as plan2:  # (as in test_one_length: the tile is reused too, same bits)
            res256 = _run_case(plan2, "ragged", dev_rows, g_feat, L, scale, domain, expect, case + " (stage-mask bit 256)", frames, nv=lens,
                               fmt=fmt, offs=(False, True, True))
        assert F._same_bits(res["g_sig"], res256["g_sig"]), f"{case}: the two plans differ"
        _check(case, res, plan, "ragged", dev_rows, fmt, lens, g_feat, L, scale, domain, (DB_R, STFT_R, FOLD_R, RS8_R if domain == 0 else None), sr)
        # n_valid below 0 and above the row length is clamped: the bits of 0 and of the full row
        wild = [-7, n_row + 1000] + lens[2:]
        res2 = _run(plan, "ragged", dev_rows, g_feat, L, scale, domain, expect, case + " (n_valid -7 and past the row)", nv=wild, fmt=fmt,
                    offs=(False, True, True))
        tame = [0, n_row] + lens[2:]
        res3 = _run(plan, "ragged", dev_rows, g_feat, L, scale, domain, expect, case + " (n_valid 0 and the row)", nv=tame, fmt=fmt,
                    offs=(False, True, True))
        assert F._same_bits(res2["g_sig"], res3["g_sig"]) and not res2["g_sig"][0].any() and res2["g_sig"][1].any()
    for u in (0, 8):
        assert not res["g_sig"][u].any()  # no samples; an all-zero clip


def test_ragged_refusals(cuda):
    """Misaligned rows, int16 rows at 22 050 Hz, a short-window plan: refused by return code, nothing launched."""
    N = _native()
    with Plan(16000, 3000, 3) as plan:
        g_feat, scale = _cotangent(2, 6)
        rows = np.zeros((2, 3000), np.float32)
        gf, gs, nv = Buf(g_feat.shape, g_feat), Buf((3, 3000)), Buf((2,), [3000, 1487], False, np.int32)
        for what, sig, fmt, domain in (("float32 rows one float off", Buf(rows.shape, rows, True), 0, 0),
                                       ("int16 rows one sample off", Buf(rows.shape, rows, True, np.int16), 1, 0),
                                       ("int16 rows at 22 050 Hz", Buf((2, plan.n_y), None, False, np.int16), 1, 1)):
            before = _snapshot()
            rc = _vjp(plan, "ragged", sig, fmt, nv, domain, 2, 6, None, gf, gs, 0)
            assert rc == N.EUNSUPPORTED, (what, rc, N.last_error())
            _assert_moved(before, {}, what)
        before = _snapshot()
        assert N.lib.lipasr_mfcc_plan_vjp_ragged(plan.h, Buf(rows.shape, rows).ptr(), 0, None, 0, 2, 6, None, gf.ptr(), gs.ptr(), 0, N.stream_ptr()) == N.EINVAL
        _assert_moved(before, {}, "null n_valid")
        torch.cuda.synchronize()
        gs.read(0)


def test_the_only_route_to_the_unreachable_instance_is_refused(cuda):
    """resample_vjp_kernel<1,true>: per-clip lengths at a rate that needs the one-output form.  16 010 Hz is such a rate (the one-length
    case one-16010-3300-L44-d0 shows it taking resample_vjp_kernel<1,false>); the ragged entry refuses the plan, both domains."""
    N = _native()
    assert set(UNREACHABLE) == {RS1_R}
    with Plan(16010, 3300, 3) as plan:
        g_feat, _ = _cotangent(2, 6)
        gf, nv = Buf(g_feat.shape, g_feat), Buf((2,), [3300, 1600], False, np.int32)
        for domain, width in ((0, 3300), (1, plan.n_y)):
            sig, gs = Buf((2, width), np.zeros((2, width), np.float32)), Buf((3, width))
            before = _snapshot()
            rc = _vjp(plan, "ragged", sig, 0, nv, domain, 2, 6, None, gf, gs, 0)
            assert rc == N.EUNSUPPORTED and "16 kHz or 8 kHz" in N.last_error(), (domain, rc, N.last_error())
            _assert_moved(before, {}, f"ragged entry on a 16 010 Hz plan, domain {domain}")
            torch.cuda.synchronize()
            gs.read(0)


# ====================================================================================================== short windows
@pytest.mark.parametrize("shape", V.SHORT_SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("L", [4, 44])
def test_short_window(cuda, shape, L):
    """lipasr_mfcc_plan_vjp_short at 22 050 Hz, domain 1 and domain 0 (the identity's copy_cut_kernel), batch 3 of 4.  64/32/1000: 34
    frame rows per clip, so every 32-row workgroup after the first straddles two clips."""
    n_fft, hop, n = shape
    with Plan(22050, n, 4, n_fft, hop) as plan:
        T = plan.n_frames
        assert T == 1 + (n + 2 * (n_fft // 2) - n_fft) // hop
        if shape == (64, 32, 1000):
            assert (n + 2 * (n_fft // 2) + hop - 1) // hop == 34
        rows = np.stack([_clip(k, n, V.SR, u + n_fft) for u, k in enumerate(("case", "quiet", "zeros"))]).astype(np.float32)
        g_feat, scale = _cotangent(3, L, n_fft)
        for domain in (1, 0):
            case = f"short-{n_fft}-{hop}-{n}-L{L}-d{domain}"
            expect = {DB: 1, DFT: 1, DFT_FOLD: 1, COPY_CUT: 1} if domain == 0 else {DB: 1, DFT: 1, DFT_FOLD: 1}
            sc = scale if domain else None
            res = _run_case(plan, "short", rows, g_feat, L, sc, domain, expect, case, [T] * 3, offs=(True, True, True))
            _check(case, res, plan, "short", rows, 0, [n] * 3, g_feat, L, sc, domain, (DB, DFT, DFT_FOLD, COPY_CUT if domain == 0 else None), V.SR,
                   n_fft, hop)
            assert not res["g_sig"][2].any()


def test_short_window_refusals(cuda):
    """short_vjp_geometry and the entries' plan checks, by return code; nothing is launched."""
    N = _native()
    for (n_fft, hop, n, L, entry, why) in ((64, 1, 100, 4, "short", "more than two workgroup images"),  # n_fft > 33 hop
                                           (32, 7, 5000, 600, "short", "bytes of LDS"),                  # 715 frames, L 600: 20 x 600 floats
                                           (2048, 512, 2205, 4, "short", "short-window backward pass covers"),
                                           (441, 220, 2205, 4, "one", "backward pass covers the 2048/512 plans"),
                                           (2048, 512, 2048, 4, "one", "longer than the reflect padding")):
        with Plan(22050, n, 2, n_fft, hop) as plan:
            g_feat, _ = _cotangent(1, L)
            sig, gf, gs = Buf((1, n), np.zeros((1, n), np.float32)), Buf(g_feat.shape, g_feat), Buf((2, n))
            before = _snapshot()
            rc = _vjp(plan, entry, sig, 0, None, 1, 1, L, None, gf, gs, 0)
            assert rc == N.EUNSUPPORTED and why in N.last_error(), (n_fft, hop, rc, N.last_error())
            # (the LDS limit of step 1 is met after the forward re-ran: no backward kernel, but forward ones)
            _assert_moved(before, {}, f"{entry} entry on a {n_fft}/{hop} plan of {n} samples", forward_may_run=(L == 600))
            torch.cuda.synchronize()
            gs.read(0)


# ====================================================================================================== stage 1 on poked tiles
def _poke_tiles(T_plan, frames, seed):
    """per clip a tile of its own frame count inside a [T_plan] tile whose frames past the clip's own hold LARGER stale values"""
    makers = (V.tie_tile, V.floor_tile, lambda T: V.dead_tile(T), V.last_element_tile, lambda T: V.last_element_tile(T, seed + 1))
    db = np.full((len(frames), T_plan, 128), 55.0, np.float32)
    fmax = np.full((len(frames), T_plan), 55.0, np.float32)
    for u, T in enumerate(frames):
        db[u, :T], fmax[u, :T] = makers[u % len(makers)](T)
    return db, fmax


@pytest.mark.parametrize("L", [3, 44])
@pytest.mark.parametrize("entry", ["one", "ragged"])
def test_stage1_on_poked_tiles(cuda, entry, L):
    """Ties, elements exactly on the floor, an all -100 dB tile, a maximum that is the clip's very last element, handed to
    mfcc_vjp_db_kernel through lipasr_debug_mfcc_stage_put and flags bit 0 (domain 1: the signal is the caller's).  The first maximum in
    (frame, mel) order takes the floored sum; !(d > thr) floors an element on the threshold; ragged: stale larger values past a clip's own
    frames are ignored.  Stages 2+3 run on whatever Gmel comes out and are checked against it."""
    case = f"poked-{entry}-L{L}"
    if entry == "one":
        sr, n, lens, nv, expect, kern = 22050, 2560, [2560] * 5, None, {DB: 1, STFT: 1, FOLD: 1}, (DB, STFT, FOLD, None)
    else:
        sr, n, lens, expect, kern = 16000, 3000, [1487, 3000, 1487, 3000, 400], {DB_R: 1, STFT_R: 1, FOLD_R: 1}, (DB_R, STFT_R, FOLD_R, None)
        nv = lens
    # (stage-mask bit 256: the caller's forward is stft_mel2_kernel, the one forward whose tile a 2048/512 backward call reuses)
    with Plan(sr, n, 6, keys=((0, 256),)) as plan:
        frames = [min(V.clip_lengths(m, sr)[2], plan.n_frames) for m in lens]
        assert frames == ([6] * 5 if entry == "one" else [5, 9, 5, 9, 2])
        db, fmax = _poke_tiles(plan.n_frames, frames, L)
        rows = np.stack([_clip("case", plan.n_y, V.SR, u) for u in range(5)]).astype(np.float32)
        g_feat, scale = _cotangent(5, L, 9)
        runs = [_run(plan, entry, rows, g_feat, L, scale, 1, expect, case, nv=nv, offs=(False, True, True), flags=1, forward=True, poke=(db, fmax),
                     fwd=(False, None))
                for _ in range(2)]
        res = runs[0]
        assert F._same_bits(res["db"], db) and F._same_bits(res["fmax"], fmax), "the poked tile did not reach the plan"
        assert F._same_bits(runs[0]["g_sig"], runs[1]["g_sig"]) and all(F._same_bits(runs[0]["gmel"][u, :T], runs[1]["gmel"][u, :T]) for u, T in enumerate(frames))
        _check(case, res, plan, entry, rows, 0, lens, g_feat, L, scale, 1, kern, sr, e2e=False)
    _stage_only[case] = list(range(5))
    g = res["gmel"]
    # clip 0, the tie tile: maxima at (1, 40), (1, 90), (3, 7); the first alone carries the floored sum
    plain, _ = V.stage1(db[0], fmax[0], g_feat[0], L, frames[0], scale, wrong="drop")
    right, A = V.stage1(db[0], fmax[0], g_feat[0], L, frames[0], scale)
    assert abs(right[1, 40] - plain[1, 40]) > 1e3 * V.U * A[1, 40] and g[0, 1, 40] != np.float32(plain[1, 40])
    if L == 3:
        assert g[0, 3, 7] == 0.0  # a later maximum in a frame >= L: no cotangent and no floored sum
    # clip 1, the floor tile: on the threshold and below it nothing, one step above it something (frames < L only carry a cotangent)
    T1 = frames[1]
    assert not g[1, :T1, 30].any() and not g[1, :T1, 32].any() and g[1, :min(L, T1), 31].all() and not g[1, :T1, 100:104].any()
    assert not g[2, :frames[2]].any() and not res["g_sig"][2].any()  # all at -100 dB
    assert g[3, frames[3] - 1, 127] != 0.0  # the very last element is the maximum: with L = 3 it holds the floored sum alone in its frame
    if L == 3:
        assert np.count_nonzero(g[3, frames[3] - 1]) == 1


# ====================================================================================================== stage 4 alone: every tap
@pytest.mark.parametrize("sr,n,kid", [(16000, 1487, RS8), (8000, 1500, RS8), (16010, 3300, RS1)])
def test_stage4_taps_bit_for_bit(cuda, sr, n, kid):
    """lipasr_mfcc_plan_resample_vjp on combs of unit impulses: row s carries impulses at s, s + spacing, ... (spacing >= nt, so every g_x
    sample sees at most one) and one on the appended zero sample; the rows s = 0 .. spacing - 1 go out in one launch.  Every g_x sample
    is one fp32 tap of lipasr_debug_table, or 0, bit for bit: every (phase, tap) pair and both clip ends, with no tolerance."""
    N = _native()
    tab, nt = _tables(sr), _nt(sr)
    n_vy, n_y, _ = V.clip_lengths(n, sr)
    spacing = nt + 3
    rows = V.comb_rows(n_y, n_vy, spacing)
    case = f"taps-{sr}-{n}"
    with Plan(sr, n, spacing + 1) as plan:
        assert plan.n_y == n_y and n_vy < n_y
        runs = []
        for rep in range(2):
            gy, gx = Buf(rows.shape, rows, True), Buf((spacing + 1, n), None, True)
            before = _snapshot()
            N.check(N.lib.lipasr_mfcc_plan_resample_vjp(plan.h, gy.ptr(), spacing, gx.ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            _assert_moved(before, {kid: 1}, case)
            gy.read()
            runs.append(gx.read(spacing))
    assert F._same_bits(runs[0], runs[1])
    want = np.stack([V.resample_vjp(rows[s], n, sr, tab)[0] for s in range(spacing)])
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64))  # one tap each: the float64 sum is that tap
    bad = np.argwhere(runs[0].view(np.uint32) != want.astype(np.float32).view(np.uint32))
    assert len(bad) == 0, f"{case}: {len(bad)} samples differ from their tap, first (row, sample) {bad[0]}: {runs[0][tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"
    assert len(np.unique(want)) > 1000  # the combs reach the table
    print(f"\n{case}: {spacing} rows x {n} samples, nt {nt}, {np.count_nonzero(want)} taps compared bit for bit")
    _record(case, [kid], 0.0)


def test_hooks_validate(cuda):
    N = _native()
    with Plan(22050, 2205, 2) as plan:
        dst = Buf((2, 5))
        # before the first backward call the plan has no workspaces
        assert N.lib.lipasr_debug_mfcc_vjp_stage(plan.h, 0, 1, dst.ptr(), N.stream_ptr()) == N.EINVAL and "no backward pass" in N.last_error()
        g_feat, _ = _cotangent(1, 4)
        rows = _clip("case", 2205, V.SR)[None].astype(np.float32)
        _run(plan, "one", rows, g_feat, 4, None, 1, {DB: 1, STFT: 1, FOLD: 1}, "hooks")
        for fn in (N.lib.lipasr_debug_mfcc_vjp_stage, N.lib.lipasr_debug_mfcc_stage_put):
            for args in ((None, 1, 1, dst.ptr()), (plan.h, 1, 1, None), (plan.h, 2, 1, dst.ptr()), (plan.h, -1, 1, dst.ptr()), (plan.h, 1, 0, dst.ptr()),
                         (plan.h, 1, 3, dst.ptr())):
                assert fn(*args, N.stream_ptr()) == N.EINVAL, (fn.__name__, args)
        torch.cuda.synchronize()
        dst.read(0)


def test_every_backward_kernel_is_claimed_and_ran():
    """The ids lipasr_debug_k1_vjp_launches knows against the claims of the cases above and the UNREACHABLE table: a kernel added
    without a case fails here.  Prints (-s) the table that DESIGN.md 3 ("Backward pass") records.  Like its forward twin this is the
    last test of the module and reads what the cases of THIS process recorded: it passes only after the whole module ran in one
    process, in file order."""
    lib = _native().lib
    have = {k for k in range(64) if lib.lipasr_debug_k1_vjp_launches(k) >= 0}
    assert lib.lipasr_debug_k1_vjp_launches(-1) == -1 and lib.lipasr_debug_k1_vjp_launches(len(KV_NAMES)) == -1
    assert have == set(range(len(KV_NAMES)))
    claimed = set(UNREACHABLE) | {RS8, RS1}  # test_stage4_taps_bit_for_bit
    for c in ONE_CASES.values():
        claimed |= set(c[-1])
    claimed |= {DB_R, STFT_R, FOLD_R, RS8_R, DFT, DFT_FOLD}  # test_ragged, test_short_window
    assert have - claimed == set(), "kernels no case claims: " + ", ".join(KV_NAMES[k] for k in sorted(have - claimed))
    assert not (set(UNREACHABLE) & set(_ran)), "an instance listed as unreachable ran"
    missing = have - set(_ran) - set(UNREACHABLE)
    assert not missing, "no case of this session ran: " + ", ".join(KV_NAMES[k] for k in sorted(missing))
    for k in sorted(have):
        if k in UNREACHABLE:
            assert lib.lipasr_debug_k1_vjp_launches(k) == 0
            print(f"{k:2d} {KV_NAMES[k]}: UNREACHABLE: {UNREACHABLE[k]}")
            continue
        assert lib.lipasr_debug_k1_vjp_launches(k) > 0
        frac, case, ratio = _worst[k]
        print(f"{k:2d} {KV_NAMES[k]}: first shown by {_ran[k]}; worst error {frac:.3f} of its bound ({case})" + (f"; device / yardstick {ratio:.2f}" if ratio is not None else ""))
    print("cases with clips checked stage by stage only:", {c: v for c, v in _stage_only.items() if v})
