"""The over-the-air channel: what a room does to a clip between the loudspeaker and the microphone, as a bank of room impulse
responses (Qin et al. 2019, section 5: the adversarial example is optimised over a set of simulated rooms).

    synthetic_rirs(count, ...)     a bank of decaying-noise responses, host only (NumPy)
    RoomChannel(rirs)              the bank on the device; apply / vjp over lipasr_room_apply / lipasr_room_vjp

``apply`` sends every clip through every room: [B, n] -> [B * R, n], row b * R + j being clip b through room j; ``vjp`` is its
exact adjoint with the rooms summed, [B * R, n] -> [B, n].  The response is causal, as long as the clip and cut at the clip's
end (include/lipasr.h has the formulas), so a clip's length means the same on both sides of the channel.
``lipasr.estimators.OverTheAirClassifier`` puts a RoomChannel in front of a WaveformClassifier.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

MAX_TAPS = 8192


def _per_room(rng, v, count, what):
    """A scalar fixes the value for every room (no draw); a pair (lo, hi) draws one uniform value per room."""
    if np.ndim(v) == 0:
        return np.full(count, float(v), dtype=np.float64)
    lo, hi = (float(a) for a in v)
    if not lo <= hi:
        raise ValueError(f"{what}: ({lo}, {hi}) is not a range")
    return rng.uniform(lo, hi, size=count)


def synthetic_rirs(count, sr=22050, taps=2048, t60=(0.15, 0.5), drr_db=(0.0, 12.0), seed=0):
    """``count`` room impulse responses of ``taps`` samples at ``sr`` Hz, float32 [count, taps]: the decaying-noise room model.

        h[0] = 1                                              the direct path (the bulk delay is removed, so that the clip
                                                              stays aligned with its ``lengths``)
        h[k] = a * eps_k * 10^(-3 k / (t60 * sr)),  k > 0     eps_k ~ N(0, 1): the level falls by 60 dB in t60 seconds
        a    such that  sum_{k > 0} h[k]^2 = 10^(-drr_db / 10)    the direct-to-reverberant energy ratio

    Everything is NumPy float64 from ``rng = np.random.Generator(np.random.PCG64(seed))``, cast to float32 at the end.  Draw order:
    ``rng.uniform(lo, hi, count)`` for t60 if it is a range, then the same for drr_db if it is a range (a scalar fixes the value and
    draws nothing), then ``rng.standard_normal((count, taps - 1))`` for eps, room by room."""
    count, taps, sr = int(count), int(taps), float(sr)
    if count < 0 or not 1 <= taps <= MAX_TAPS or not sr > 0:
        raise ValueError(f"count={count}, taps={taps}, sr={sr}: count >= 0, 1 <= taps <= {MAX_TAPS}, sr > 0")
    rng = np.random.Generator(np.random.PCG64(seed))
    t = _per_room(rng, t60, count, "t60")
    d = _per_room(rng, drr_db, count, "drr_db")
    if np.any(t <= 0):
        raise ValueError("t60 must be positive")
    eps = rng.standard_normal((count, taps - 1))
    k = np.arange(1, taps, dtype=np.float64)
    tail = eps * 10.0 ** (-3.0 * k[None, :] / (t[:, None] * sr))
    energy = np.sum(tail * tail, axis=1, keepdims=True)
    a = np.sqrt(10.0 ** (-d[:, None] / 10.0) / np.where(energy > 0, energy, 1.0))
    h = np.empty((count, taps), dtype=np.float64)
    h[:, 0] = 1.0
    h[:, 1:] = a * tail
    return h.astype(np.float32)


class RoomChannel:
    """A bank of room impulse responses [R, taps] (array or tensor; synthetic_rirs' or measured ones, at the rate of the rows they
    will meet) held on the device."""

    def __init__(self, rirs, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        t = rirs if torch.is_tensor(rirs) else torch.as_tensor(np.asarray(rirs, dtype=np.float32))
        if t.dim() != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= MAX_TAPS:
            raise ValueError(f"rirs must be [R >= 1, 1 <= taps <= {MAX_TAPS}], got {tuple(t.shape)}")
        self.rirs = t.to(device=self.device, dtype=torch.float32).contiguous()
        self.count, self.taps = int(t.shape[0]), int(t.shape[1])

    def subset(self, idx):
        """A channel over the rooms ``idx`` (indices, a slice or a mask) of this one."""
        if not isinstance(idx, slice):
            idx = torch.as_tensor(np.asarray(idx), device=self.device)
        return RoomChannel(self.rirs[idx].reshape(-1, self.taps), device=self.device)

    def _rows(self, x, what, multiple=1):
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous() \
                or x.shape[0] % multiple:
            raise ValueError(f"{what} must be a contiguous float32 device tensor [{'B * %d' % multiple if multiple > 1 else 'B'}, n]")
        return x.shape[0] // multiple, x.shape[1]

    def _out(self, out, rows, n, what):
        if out is None:
            return torch.empty(rows, n, device=self.device)
        if self._rows(out, what) != (rows, n):
            raise ValueError(f"{what} must be [{rows}, {n}], got {tuple(out.shape)}")
        return out

    def _n_valid(self, n_valid, b):
        if n_valid is None:
            return None
        if not torch.is_tensor(n_valid) or n_valid.dtype != torch.int32 or tuple(n_valid.shape) != (b,) or not n_valid.is_cuda \
                or not n_valid.is_contiguous():
            raise ValueError(f"n_valid must be a contiguous int32 device tensor [{b}]")
        return n_valid

    def apply(self, x, n_valid=None, out=None):
        """[B, n] -> [B * R, n]: clip b through room j in row b * R + j.  ``n_valid``: int32 device tensor [B], the POSITIONS of
        each row that belong to its clip (None: all n); the output is exactly 0 from there on."""
        b, n = self._rows(x, "x")
        out = self._out(out, b * self.count, n, "out")
        N.check(N.lib.lipasr_room_apply(N.ptr(x), N.ptr(self._n_valid(n_valid, b)), N.ptr(self.rirs), self.taps, self.count, b, n,
                                        N.ptr(out), N.stream_ptr()))
        return out

    def vjp(self, g, n_valid=None, scale=1.0, out=None):
        """[B * R, n] -> [B, n]: ``scale`` times the adjoint of ``apply`` at the cotangent ``g``, summed over the rooms."""
        b, n = self._rows(g, "g", self.count)
        out = self._out(out, b, n, "out")
        N.check(N.lib.lipasr_room_vjp(N.ptr(g), N.ptr(self._n_valid(n_valid, b)), N.ptr(self.rirs), self.taps, self.count, b, n,
                                      float(scale), N.ptr(out), N.stream_ptr()))
        return out
