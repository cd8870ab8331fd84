"""Input-transformation defences over audio: the clip is cleaned before the recogniser hears it (Rajaratnam and Kalita 2018; Yang et
al. 2019; ART's SpatialSmoothing, FeatureSqueezing and Resample preprocessors), and the detector built on them (Xu, Evans and Qi
2018, "feature squeezing").

    lowpass_taps(cutoff_hz, sr, taps)      a Hamming-windowed sinc, host only (NumPy)
    bandpass_taps(lo_hz, hi_hz, sr, taps)  the difference of two of them
    parse_defence(spec, sr)                "median:5,lowpass:4000:101,quantize:8" -> the stage list below
    AudioDefence(stages)                   a chain of 1 to 4 stages on the device; apply / vjp over lipasr_defence_apply / _vjp
    TransformationDetector(base, defences) the largest L1 distance between the base's probabilities at x and at T(x)

A stage is ("median", width), ("fir", taps) -- "lowpass" and "bandpass" are other names for it -- or ("quantize", bits);
include/lipasr.h has the formulas.  ``apply`` and ``vjp`` are ONE launch each, whatever the chain: the intermediates stay in LDS.
``vjp(..., backward="chain")`` differentiates through the chain (the median routes each gradient to the element it selected, the
FIR is its exact adjoint, the quantiser is straight-through where its clamp was idle); ``backward="identity"`` treats the whole
defence as the identity on the way back (BPDA's plainest form, Athalye, Carlini and Wagner 2018) and launches nothing.
``lipasr.estimators.DefendedClassifier`` puts an AudioDefence in front of a WaveformClassifier.

Not built: MP3 compression; resampling as a stage of its own (a low-pass is its linear part); randomised defences
(``lipasr.smoothing.Smooth`` is the certified one); training with the defence in the loop."""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

MAX_STAGES, MAX_HALO = N.DEFENCE_MAX_STAGES, N.DEFENCE_MAX_HALO
_FIR_NAMES = ("fir", "lowpass", "bandpass")


def _sinc_taps(cutoff_hz, sr, taps):
    taps, sr, cutoff_hz = int(taps), float(sr), float(cutoff_hz)
    if taps < 1 or taps > 255 or taps % 2 == 0:
        raise ValueError(f"taps={taps}: an odd count from 1 to 255")
    if not sr > 0 or not 0 < cutoff_hz <= sr / 2:
        raise ValueError(f"cutoff {cutoff_hz} Hz at sr={sr}: 0 < cutoff <= sr / 2")
    k = np.arange(taps, dtype=np.float64) - (taps - 1) / 2
    fc = cutoff_hz / sr  # cycles per sample
    return 2.0 * fc * np.sinc(2.0 * fc * k) * np.hamming(taps)


def lowpass_taps(cutoff_hz, sr, taps=101):
    """float32 [taps]: sinc(2 fc k) hamming(k) about the centre tap, fc = cutoff_hz / sr, in float64, normalised to sum 1 (unit gain
    at 0 Hz), then cast."""
    h = _sinc_taps(cutoff_hz, sr, taps)
    return (h / h.sum()).astype(np.float32)


def bandpass_taps(lo_hz, hi_hz, sr, taps=101):
    """float32 [taps]: the low-pass at ``hi_hz`` minus the low-pass at ``lo_hz``, each normalised to unit gain at 0 Hz in float64
    (so the band-pass has none there), then cast."""
    if not float(lo_hz) < float(hi_hz):
        raise ValueError(f"band ({lo_hz}, {hi_hz}) Hz: lo < hi")
    hi, lo = _sinc_taps(hi_hz, sr, taps), _sinc_taps(lo_hz, sr, taps)
    return (hi / hi.sum() - lo / lo.sum()).astype(np.float32)


def parse_defence(spec, sr):
    """``"median:5,lowpass:4000:101,bandpass:300:4000:101,quantize:8"`` -> [("median", 5), ("lowpass", taps), ...]; the tap count
    may be left out (101).  ``sr``: the rate of the rows the defence will meet."""
    stages = []
    for part in str(spec).split(","):
        name, *args = part.strip().split(":")
        try:
            if name == "median" and len(args) == 1:
                stages.append((name, int(args[0])))
            elif name == "quantize" and len(args) == 1:
                stages.append((name, int(args[0])))
            elif name == "lowpass" and len(args) in (1, 2):
                stages.append((name, lowpass_taps(float(args[0]), sr, *(int(a) for a in args[1:]))))
            elif name == "bandpass" and len(args) in (2, 3):
                stages.append((name, bandpass_taps(float(args[0]), float(args[1]), sr, *(int(a) for a in args[2:]))))
            else:
                raise ValueError("unknown stage or wrong number of arguments")
        except ValueError as e:
            raise ValueError(f"defence stage {part!r}: {e} (median:K, lowpass:HZ[:TAPS], bandpass:LO:HI[:TAPS], quantize:BITS)") from None
    return stages


def chain_of(stages):
    """``stages`` checked and in the ABI's terms: a list of (kind, arg, taps) with taps a float32 NumPy array or device tensor for a
    FIR stage and None otherwise, and the sum of the half-widths."""
    stages = list(stages)
    if not 1 <= len(stages) <= MAX_STAGES:
        raise ValueError(f"a defence has 1 to {MAX_STAGES} stages, got {len(stages)}")
    out, halo = [], 0
    for i, st in enumerate(stages):
        if not isinstance(st, (tuple, list)) or len(st) != 2:
            raise ValueError(f"stage {i}: a pair (name, argument), got {st!r}")
        name, arg = st
        if name == "median":
            k = int(arg)
            if k % 2 == 0 or not 3 <= k <= 15:
                raise ValueError(f"stage {i}: a median of width {k}; odd widths 3 to 15")
            out.append((N.DEFENCE_MEDIAN, k, None))
            halo += (k - 1) // 2
        elif name in _FIR_NAMES:
            t = arg if torch.is_tensor(arg) else np.ascontiguousarray(np.asarray(arg, dtype=np.float32))
            if t.ndim != 1 or t.shape[0] % 2 == 0 or not 1 <= t.shape[0] <= 255:
                raise ValueError(f"stage {i}: taps must be a vector of an odd length from 1 to 255, got shape {tuple(t.shape)}")
            out.append((N.DEFENCE_FIR, int(t.shape[0]), t))
            halo += (int(t.shape[0]) - 1) // 2
        elif name == "quantize":
            bits = int(arg)
            if not 2 <= bits <= 16:
                raise ValueError(f"stage {i}: {bits} bits; 2 to 16")
            out.append((N.DEFENCE_QUANTIZE, bits, None))
        else:
            raise ValueError(f"stage {i}: unknown kind {name!r} (median, fir / lowpass / bandpass, quantize)")
    if halo > MAX_HALO:
        raise ValueError(f"the half-widths of the chain sum to {halo}; at most {MAX_HALO}")
    return out, halo


class AudioDefence:
    """A chain of 1 to 4 stages, e.g. ``[("median", 5), ("lowpass", taps), ("quantize", 8)]``, with its taps held on the device.
    ``halo``: the sum of the stages' half-widths (at most 256), how far the chain reaches to either side of a sample."""

    def __init__(self, stages, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        chain, self.halo = chain_of(stages)
        self.stages = [(k, a) for k, a, _ in chain]
        self._taps = [None if t is None else torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous() for _, _, t in chain]
        self._chain = N.defence_chain(self.stages, [None if t is None else t.data_ptr() for t in self._taps])

    def _rows(self, x, what, shape=None):
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 device tensor [B, n]")
        if shape is not None and tuple(x.shape) != tuple(shape):
            raise ValueError(f"{what} must be {tuple(shape)}, got {tuple(x.shape)}")
        return x.shape

    def _out(self, out, shape):
        if out is None:
            return torch.empty(*shape, device=self.device)
        self._rows(out, "out", shape)
        return out

    def _n_valid(self, n_valid, b):
        if n_valid is None:
            return None
        if not torch.is_tensor(n_valid) or n_valid.dtype != torch.int32 or tuple(n_valid.shape) != (b,) or not n_valid.is_cuda \
                or not n_valid.is_contiguous():
            raise ValueError(f"n_valid must be a contiguous int32 device tensor [{b}]")
        return n_valid

    def apply(self, x, n_valid=None, out=None):
        """[B, n] -> [B, n]: the chain in one launch.  ``n_valid``: int32 device tensor [B], the POSITIONS of each row that belong
        to its clip (None: all n); the output is exactly 0 from there on."""
        b, n = self._rows(x, "x")
        out = self._out(out, (b, n))
        kinds, args, taps, count = self._chain
        N.check(N.lib.lipasr_defence_apply(N.ptr(x), N.ptr(self._n_valid(n_valid, b)), kinds, args, taps, count, b, n, N.ptr(out),
                                           N.stream_ptr()))
        return out

    def vjp(self, x, g, n_valid=None, backward="chain", out=None):
        """[B, n], [B, n] -> [B, n]: the cotangent ``g`` of ``apply(x)`` carried back to ``x``.  backward="chain": through the
        chain, one launch; "identity": ``g`` masked to the clip, no launch."""
        b, n = self._rows(x, "x")
        self._rows(g, "g", (b, n))
        nv = self._n_valid(n_valid, b)
        if backward == "identity":
            if nv is None:
                return g.clone() if out is None else self._out(out, (b, n)).copy_(g)
            inside = torch.arange(n, device=g.device, dtype=torch.int32)[None, :] < nv.clamp(0, n)[:, None]
            res = torch.where(inside, g, torch.zeros((), device=g.device))
            return res if out is None else self._out(out, (b, n)).copy_(res)
        if backward != "chain":
            raise ValueError(f"backward={backward!r}: 'chain' or 'identity'")
        out = self._out(out, (b, n))
        kinds, args, taps, count = self._chain
        N.check(N.lib.lipasr_defence_vjp(N.ptr(x), N.ptr(g), N.ptr(nv), kinds, args, taps, count, b, n, N.ptr(out), N.stream_ptr()))
        return out


def quantile_threshold(clean_scores, fpr=0.05):
    """The (1 - fpr) quantile of the clean scores (NumPy's linear interpolation): a clip is flagged when its score EXCEEDS it."""
    s = np.asarray(clean_scores, dtype=np.float64).reshape(-1)
    if s.size == 0 or not 0.0 <= float(fpr) <= 1.0:
        raise ValueError("fit needs at least one clean score and 0 <= fpr <= 1")
    return float(np.quantile(s, 1.0 - float(fpr)))


def roc_auc(clean_scores, adv_scores):
    """The probability that an adversarial score exceeds a clean one, ties counting a half (the Mann-Whitney statistic)."""
    c = np.sort(np.asarray(clean_scores, dtype=np.float64).reshape(-1))
    a = np.asarray(adv_scores, dtype=np.float64).reshape(-1)
    if c.size == 0 or a.size == 0:
        raise ValueError("roc_auc needs scores of both kinds")
    below = np.searchsorted(c, a, side="left")            # clean scores strictly below each adversarial one
    ties = np.searchsorted(c, a, side="right") - below
    return float((below.sum() + 0.5 * ties.sum()) / (c.size * a.size))


class TransformationDetector:
    """Feature squeezing as a detector (Xu, Evans and Qi 2018): a clip whose prediction moves much under a harmless transformation
    is suspect.  ``base``: an estimator over audio (predict_device); ``defences``: the AudioDefences to compare against.
        scores(x, lengths=None)   max over the defences of || p(x) - p(T(x)) ||_1, a device tensor [B] (torch ops on [B, classes])
        fit(x_clean, fpr=0.05)    the threshold: the (1 - fpr) quantile of the clean scores
        detect(x, lengths=None)   (flags, scores): flags = scores > threshold
        roc_auc(clean, adv)       threshold-free: NumPy, on score arrays"""

    roc_auc = staticmethod(roc_auc)

    def __init__(self, base, defences):
        defences = list(defences)
        if not hasattr(base, "predict_device"):
            raise TypeError("base must be an estimator (predict_device)")
        if not defences or not all(isinstance(d, AudioDefence) for d in defences):
            raise TypeError("defences must be a non-empty list of AudioDefence")
        self.base, self.defences, self.threshold = base, defences, None

    def scores(self, x, lengths=None):
        base = self.base
        xt = base.rows_device(x)
        lt = base.lengths_device(lengths, xt.shape[0])
        nv = None if lt is None else base.clip_positions(lt).contiguous()
        p0 = base.predict_device(xt, lengths=lt)
        best = torch.zeros(xt.shape[0], device=xt.device)
        for d in self.defences:
            best = torch.maximum(best, (base.predict_device(d.apply(xt, nv), lengths=lt) - p0).abs().sum(dim=1))
        return best

    def fit_scores(self, clean_scores, fpr=0.05):
        self.threshold = quantile_threshold(clean_scores, fpr)
        return self

    def fit(self, x_clean, fpr=0.05, lengths=None):
        return self.fit_scores(self.scores(x_clean, lengths).cpu().numpy(), fpr)

    def flag_scores(self, scores):
        if self.threshold is None:
            raise RuntimeError("fit the detector first")
        return scores > self.threshold

    def detect(self, x, lengths=None):
        s = self.scores(x, lengths)
        return self.flag_scores(s), s
