"""Psychoacoustic masking threshold of a clip (ART's ``PsychoacousticMasker``) and the loss an imperceptible attack drives
under it: how far a perturbation's power spectrum rises above what the clip itself masks.

    STFT (2048 / 512, periodic Hann, no padding) -> PSD normalised to 96 dB -> tonal maskers (strict local maxima over the
    absolute threshold of hearing, merged within half a Bark) -> threshold = ATH + the maskers' spreading functions

Every step is a kernel behind the C ABI (lipasr_psy_* in include/lipasr.h, which has the equations); this module owns the plans
and hands device tensors through.  The device keeps the threshold LINEAR, ``theta [B, T, 1025]``; ART's surface
(``calculate_threshold_and_psd_maximum``) returns 10 log10 of it as ``[1025, T]``.

``bark_by="position"`` reproduces a quirk of ART's merge: it looks the Bark value up at a masker's position in the list instead
of at its frequency bin.  The default, "bin", is what the rule means.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N

WINDOW, HOP, BINS = 2048, 512, 1025


class PsychoacousticMasker:
    """ART ``PsychoacousticMasker(window_size, hop_size, sample_rate)`` for the 2048 / 512 framing.  Native plans are made per
    (clip length, batch) on first use and kept."""

    def __init__(self, window_size=WINDOW, hop_size=HOP, sample_rate=16000, bark_by="bin", device=None):
        if int(window_size) != WINDOW or int(hop_size) != HOP:
            raise ValueError(f"window_size={window_size}, hop_size={hop_size}: the kernels are built for {WINDOW} / {HOP}")
        if bark_by not in ("bin", "position"):
            raise ValueError(f"bark_by={bark_by!r}: 'bin' or 'position'")
        if int(sample_rate) < 1:
            raise ValueError(f"sample_rate={sample_rate}")
        self.window_size, self.hop_size, self.sample_rate, self.bark_by = WINDOW, HOP, int(sample_rate), bark_by
        self._device_arg = device
        self.device = None
        self.h = None
        self._plans = {}  # (n, batch_max) -> native plan

    # ---- tables (host only: no GPU needed) ----
    @property
    def fft_frequencies(self):
        return N.psy_table(0, self.sample_rate)

    @property
    def bark(self):
        return N.psy_table(1, self.sample_rate)

    @property
    def absolute_threshold_hearing(self):
        return N.psy_table(2, self.sample_rate)

    # ---- plans ----
    @staticmethod
    def n_frames(n):
        if n < WINDOW:
            raise ValueError(f"a clip of {n} samples does not hold one window of {WINDOW}")
        return 1 + (n - WINDOW) // HOP

    def _plan(self, n, batch):
        if self._plans is None:
            raise RuntimeError("PsychoacousticMasker used after close()")
        if self.h is None:
            dev = self._device_arg
            self.device = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
            self.h = N.get_handle(self.device.index)
            N.register_owner(self)
        for (pn, pb), plan in self._plans.items():
            if pn == n and pb >= batch:
                return plan
        plan = N.c_h()
        N.check(N.lib.lipasr_psy_create(self.h.h, self.sample_rate, n, batch, 1 if self.bark_by == "position" else 0, C.byref(plan)))
        self._plans[(n, batch)] = plan
        return plan

    def close(self):
        plans, self._plans = getattr(self, "_plans", None), None
        if plans and self.h is not None and self.h.alive:
            for plan in plans.values():
                N.destroy_or_defer(N.lib.lipasr_psy_destroy, plan)  # (a finaliser may run in the middle of a graph capture)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _rows(x, what):
        if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or not x.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 device tensor [B, n]")
        PsychoacousticMasker.n_frames(x.shape[1])
        return x.shape

    # ---- device entries ----
    def psd_device(self, x):
        """[B, n] -> (psd [B, T, 1025] in dB, psd_max [B])."""
        b, n = self._rows(x, "x")
        psd = torch.empty(b, self.n_frames(n), BINS, device=x.device)
        mx = torch.empty(b, device=x.device)
        N.check(N.lib.lipasr_psy_psd(self._plan(n, b), N.ptr(x), n, b, N.ptr(psd), N.ptr(mx), N.stream_ptr()))
        return psd, mx

    def threshold_device(self, psd, return_counts=False):
        """Any PSD [B, T, 1025] in dB -> theta [B, T, 1025] (linear), and the surviving maskers per frame [B, T] on request."""
        if not torch.is_tensor(psd) or not psd.is_cuda or psd.dtype != torch.float32 or psd.dim() != 3 or psd.shape[2] != BINS \
                or not psd.is_contiguous():
            raise ValueError(f"psd must be a contiguous float32 device tensor [B, T, {BINS}]")
        b, t = psd.shape[0], psd.shape[1]
        theta = torch.empty_like(psd)
        cnt = torch.empty(b, t, dtype=torch.int32, device=psd.device) if return_counts else None
        N.check(N.lib.lipasr_psy_threshold(self._plan(WINDOW + HOP * (t - 1), b), N.ptr(psd), t, b, N.ptr(theta), N.ptr(cnt), N.stream_ptr()))
        return (theta, cnt) if return_counts else theta

    def prepare_device(self, x):
        """[B, n] -> (theta [B, T, 1025] linear, psd_max [B]): what ``loss_gradient_device`` needs of the clean clips."""
        b, n = self._rows(x, "x")
        theta = torch.empty(b, self.n_frames(n), BINS, device=x.device)
        mx = torch.empty(b, device=x.device)
        N.check(N.lib.lipasr_psy_prepare(self._plan(n, b), N.ptr(x), n, b, N.ptr(theta), N.ptr(mx), N.stream_ptr()))
        return theta, mx

    def loss_gradient_device(self, delta, theta, psd_max, need_grad=True, out=None):
        """Perturbations [B, n] against the clips' theta / psd_max -> (loss [B], gradient [B, n] or None)."""
        b, n = self._rows(delta, "delta")
        if tuple(theta.shape) != (b, self.n_frames(n), BINS) or tuple(psd_max.shape) != (b,) or not theta.is_contiguous() \
                or theta.dtype != torch.float32 or psd_max.dtype != torch.float32 or not psd_max.is_contiguous():
            raise ValueError(f"theta must be float32 [{b}, {self.n_frames(n)}, {BINS}] and psd_max float32 [{b}]")
        loss = torch.empty(b, device=delta.device)
        g = (torch.empty_like(delta) if out is None else out) if need_grad else None
        N.check(N.lib.lipasr_psy_loss_grad(self._plan(n, b), N.ptr(delta), n, b, N.ptr(theta), N.ptr(psd_max), N.ptr(loss), N.ptr(g),
                                           N.stream_ptr()))
        return loss, g

    def step_device(self, delta, x_adv, x0, g_net, g_theta, alpha, eps, lr, use_sign, clip_values):
        """One attack step in place on ``delta`` and ``x_adv`` (lipasr_psy_step); alpha, eps: float32 device tensors [B]."""
        b, n = delta.shape
        lo, hi = (-np.inf, np.inf) if clip_values is None else clip_values
        N.check(N.lib.lipasr_psy_step(self._plan(max(n, WINDOW), b), N.ptr(delta), N.ptr(x_adv), N.ptr(x0), N.ptr(g_net), N.ptr(g_theta),
                                      N.ptr(alpha), N.ptr(eps), n, b, float(lr), 1 if use_sign else 0, float(lo), float(hi), N.stream_ptr()))
        return delta, x_adv

    # ---- ART's surface: NumPy in and out, one clip ----
    def _one(self, audio):
        a = np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(1, -1))
        self.n_frames(a.shape[1])
        dev = self._device_arg if self._device_arg is not None else torch.device("cuda", torch.cuda.current_device())
        return torch.as_tensor(a).to(dev)

    def power_spectral_density(self, audio):
        """-> (psd [1025, T] normalised to 96 dB, psd_max)."""
        psd, mx = self.psd_device(self._one(audio))
        return psd[0].t().cpu().numpy(), float(mx[0])

    def calculate_threshold_and_psd_maximum(self, audio):
        """-> (masking threshold in dB [1025, T], psd_max); -inf where nothing masks and the ATH is undefined."""
        theta, mx = self.prepare_device(self._one(audio))
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(theta[0].t().double().cpu().numpy()), float(mx[0])
