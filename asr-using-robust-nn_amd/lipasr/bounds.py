"""Certified robustness of the dense classifier by bound propagation (ours: the reference has no certificate).

Interval bounds (IBP; Gowal et al. 2018) go forward through the dense layers, one backward linear-relaxation pass gives the
margins (CROWN-IBP; Zhang et al. 2020): lipasr_mlp_bounds, DESIGN.md "Bound propagation".  What comes out is deterministic and
speaks about the base classifier itself, in norm inf (the threat model of FGSM, PGD, Auto-PGD, Square and AutoAttack) and norm 2:

    bound_margins       lower bounds of z_y - z_k over  {v : ||v - x_b|| <= eps_b} /\\ clip box,  per row and class
    certified_radius    per row the largest eps of a bisection at which every margin stayed positive
    certified_accuracy  the share of rows certified at each eps of a grid: the lower end of the bracket whose upper end an attack gives

The estimator is a TensorFlowV2Classifier (rows of MFCC features; its ``clip_values`` are honoured).  A WaveformClassifier is
refused: the log of the MFCC stage has no interval form here, as ``certified`` is None over audio in get_robustness_radius.
The bounds hold for the real-arithmetic function of the fp32 weights: every rounding of the propagation itself is accounted for.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from . import estimators as E
from .keras import CategoricalCrossentropy

METHODS = ("crown-ibp", "ibp")


class IBPCrossentropy(CategoricalCrossentropy):
    """IBP certified training (Gowal et al. 2018) as a loss for ``Model.compile``:

        loss = (1 - kappa_t) CE(logits(x), y) + kappa_t CE(worst-case logits over the eps_t-box around x, y)

    The worst-case logits are the interval bounds of lipasr_mlp_bounds (norm inf, the classifier in inference form: running
    BatchNorm statistics, dropout off), their gradient is lipasr_mlp_bounds_grad ("Certified training").  For
    ``warmup_steps`` steps the loss is plain cross-entropy; over the next ``ramp_steps`` steps eps_t and kappa_t rise linearly from
    0 to ``eps`` and ``kappa`` and stay there.  The step counter lives here, on the host: one count per ``train_on_batch``.
    ``clip_values``: the box the inputs live in (default none), as an estimator's.  ``evaluate`` and ``save`` of the model stay on
    plain cross-entropy; ``fit`` logs the mixed loss.  Not built: norm 2, data parallel, TrainPipeline."""

    name = "ibp_categorical_crossentropy"
    certified = True  # Model.train_on_batch hands the step to train_step below

    def __init__(self, eps, kappa=0.5, warmup_steps=0, ramp_steps=1, clip_values=None, norm=float("inf")):
        if N._norm_f(norm) != float("inf"):
            raise ValueError(f"norm = {norm!r}: IBP certified training is built for norm inf; norm 2 (the column-norm branch of the "
                             "first layer) is not built")
        if not float(eps) >= 0 or not np.isfinite(eps):
            raise ValueError(f"eps = {eps!r}: a finite number >= 0")
        if not 0.0 <= float(kappa) <= 1.0:
            raise ValueError(f"kappa = {kappa!r}: in [0, 1]")
        if int(warmup_steps) < 0 or int(ramp_steps) < 1:
            raise ValueError(f"warmup_steps = {warmup_steps!r}, ramp_steps = {ramp_steps!r}: >= 0 and >= 1")
        self.clip = (-float("inf"), float("inf")) if clip_values is None else (float(clip_values[0]), float(clip_values[1]))
        if not self.clip[0] <= self.clip[1]:
            raise ValueError(f"clip_values = {clip_values!r}: low <= high")
        self.eps, self.kappa = float(eps), float(kappa)
        self.warmup_steps, self.ramp_steps = int(warmup_steps), int(ramp_steps)
        self.step = 0

    def schedule(self, step):
        """(eps_t, kappa_t) of the ``step``-th call of train_on_batch, counted from 0."""
        f = min(max((int(step) - self.warmup_steps) / self.ramp_steps, 0.0), 1.0)
        return self.eps * f, self.kappa * f

    def _buffers(self, model):
        """The device floats of one certified step, once per model at its max_batch."""
        buf = getattr(model, "_ibp_buffers", None)
        if buf is None:
            b, w, dev = model._max_batch, model._widths, model._device
            need, need_g = N.sz(), N.sz()
            N.check(N.lib.lipasr_mlp_bounds_workspace(model._plan, b, N.C.byref(need)))
            N.check(N.lib.lipasr_mlp_bounds_grad_workspace(model._plan, b, N.C.byref(need_g)))
            fam = N.bounds_family_floats(w, b)
            f = lambda n: torch.zeros(n, device=dev)
            buf = {"ws": f(need.value), "ws_grad": f(need_g.value), "lo": f(fam), "hi": f(fam), "margin": f(b * w[-1]), "eps": f(b),
                   "rows": f(b)}
            model._ibp_buffers = buf
        return buf

    def train_step(self, model, xb, yb, masks=None, dropout=True):
        """One step of ``model`` under this loss; False when kappa_t is 0 (the caller then makes the plain step's calls).
        Otherwise: the plain forward and backward pass scaled by 1 - kappa_t, the interval bounds at eps_t on the same parameters,
        their gradient mixed in at kappa_t / batch, Adam.  Stream-ordered; nothing synchronises."""
        eps_t, kappa_t = self.schedule(self.step)
        self.step += 1
        if kappa_t == 0.0:
            return False
        b = xb.shape[0]
        buf = self._buffers(model)
        model.train_fwd_bwd(xb, yb, inv_batch=(1.0 - kappa_t) / b, masks=masks, dropout=dropout)
        yt = yb.argmax(dim=1).to(torch.int32)
        buf["eps"][:b].fill_(eps_t)
        args = (model._plan, N.ptr(model._params), N.ptr(model._bnstate))
        N.check(N.lib.lipasr_mlp_bounds(*args, N.ptr(xb), N.ptr(buf["eps"]), float("inf"), self.clip[0], self.clip[1], N.ptr(yt), b,
                                        N.ptr(buf["ws"]), buf["ws"].numel(), N.ptr(buf["margin"]), None, None, N.ptr(buf["lo"]),
                                        N.ptr(buf["hi"]), N.stream_ptr()))
        N.check(N.lib.lipasr_mlp_bounds_grad(*args, N.ptr(buf["margin"]), N.ptr(buf["lo"]), N.ptr(buf["hi"]), N.ptr(yt), b,
                                             N.ptr(buf["ws_grad"]), buf["ws_grad"].numel(), 1.0, kappa_t / b, N.ptr(model._grads),
                                             N.ptr(buf["rows"]), N.stream_ptr()))
        rows = model._loss_rows[:b]
        rows.mul_(1.0 - kappa_t).add_(buf["rows"][:b], alpha=kappa_t)  # what fit() logs
        model.apply_adam()
        return True


class CrownIBPCrossentropy(IBPCrossentropy):
    """CROWN-IBP certified training (Zhang et al. 2020) as a loss for ``Model.compile``: IBPCrossentropy with the worst-case logits
    taken from the mixed margin

        (1 - beta_t) margin_ibp + beta_t margin_crown

    of ONE lipasr_mlp_bounds call; its gradient is lipasr_mlp_bounds_crown_grad ("CROWN-IBP certified training").
    beta_t goes linearly from ``beta_start`` to ``beta_end`` over the ramp of eps_t and kappa_t; the paper's schedule is 1 -> 0,
    ``beta_start = beta_end = 1`` trains on the CROWN-IBP margin throughout.  A step at beta_t = 0 makes exactly the calls of
    IBPCrossentropy, a step at kappa_t = 0 those of the plain step.  Not built: norm 2, data parallel, TrainPipeline."""

    name = "crown_ibp_categorical_crossentropy"

    def __init__(self, eps, kappa=0.5, warmup_steps=0, ramp_steps=1, beta_start=1.0, beta_end=0.0, clip_values=None, norm=float("inf")):
        super().__init__(eps, kappa=kappa, warmup_steps=warmup_steps, ramp_steps=ramp_steps, clip_values=clip_values, norm=norm)
        for k, v in (("beta_start", beta_start), ("beta_end", beta_end)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"{k} = {v!r}: in [0, 1]")
        self.beta_start, self.beta_end = float(beta_start), float(beta_end)

    def beta_schedule(self, step):
        """beta_t of the ``step``-th call of train_on_batch, counted from 0."""
        f = min(max((int(step) - self.warmup_steps) / self.ramp_steps, 0.0), 1.0)
        return self.beta_start + (self.beta_end - self.beta_start) * f

    def _crown_buffers(self, model):
        buf = self._buffers(model)
        if "ws_crown" not in buf:
            b, w, dev = model._max_batch, model._widths, model._device
            need = N.sz()
            N.check(N.lib.lipasr_mlp_bounds_crown_grad_workspace(model._plan, b, N.C.byref(need)))
            buf["ws_crown"] = torch.zeros(need.value, device=dev)
            buf["margin_crown"] = torch.zeros(b * w[-1], device=dev)
        return buf

    def train_step(self, model, xb, yb, masks=None, dropout=True):
        """One step of ``model`` under this loss; False when kappa_t is 0.  Otherwise the plain pass scaled by 1 - kappa_t, the
        bounds at eps_t with margin_crown, lipasr_mlp_bounds_crown_grad at beta_t mixed in at kappa_t / batch, Adam."""
        beta_t = self.beta_schedule(self.step)
        if beta_t == 0.0 or self.schedule(self.step)[1] == 0.0:
            return super().train_step(model, xb, yb, masks=masks, dropout=dropout)
        eps_t, kappa_t = self.schedule(self.step)
        self.step += 1
        b = xb.shape[0]
        buf = self._crown_buffers(model)
        model.train_fwd_bwd(xb, yb, inv_batch=(1.0 - kappa_t) / b, masks=masks, dropout=dropout)
        yt = yb.argmax(dim=1).to(torch.int32)
        buf["eps"][:b].fill_(eps_t)
        args = (model._plan, N.ptr(model._params), N.ptr(model._bnstate))
        N.check(N.lib.lipasr_mlp_bounds(*args, N.ptr(xb), N.ptr(buf["eps"]), float("inf"), self.clip[0], self.clip[1], N.ptr(yt), b,
                                        N.ptr(buf["ws"]), buf["ws"].numel(), N.ptr(buf["margin"]), N.ptr(buf["margin_crown"]), None,
                                        N.ptr(buf["lo"]), N.ptr(buf["hi"]), N.stream_ptr()))
        N.check(N.lib.lipasr_mlp_bounds_crown_grad(*args, N.ptr(buf["margin"]), N.ptr(buf["margin_crown"]), N.ptr(buf["lo"]),
                                                   N.ptr(buf["hi"]), N.ptr(yt), b, beta_t, N.ptr(buf["ws_crown"]),
                                                   buf["ws_crown"].numel(), 1.0, kappa_t / b, N.ptr(model._grads), N.ptr(buf["rows"]),
                                                   N.stream_ptr()))
        rows = model._loss_rows[:b]
        rows.mul_(1.0 - kappa_t).add_(buf["rows"][:b], alpha=kappa_t)  # what fit() logs
        model.apply_adam()
        return True


def _check(estimator, norm, method):
    if getattr(estimator, "extractor", None) is not None or isinstance(estimator, E.WaveformClassifier):
        raise TypeError("bound propagation needs rows of features (a TensorFlowV2Classifier): over audio the MFCC stage's log has "
                        "no interval form here, so nothing can be certified through it")
    if not isinstance(estimator, E.TensorFlowV2Classifier):
        raise TypeError("estimator must be a lipasr.estimators.TensorFlowV2Classifier")
    if method not in METHODS:
        raise ValueError(f"method = {method!r}: one of {METHODS}")
    norm = N._norm_f(norm)
    if norm not in (2.0, float("inf")):
        raise ValueError(f"norm = {norm!r}: inf or 2")
    return norm


def _clip(estimator, clip_values):
    cv = estimator.clip_values if clip_values is None else clip_values
    return (-float("inf"), float("inf")) if cv is None else (float(cv[0]), float(cv[1]))


def _eps_device(eps, b, device):
    if torch.is_tensor(eps):
        et = eps.to(device=device, dtype=torch.float32).reshape(-1)
    else:
        e = np.asarray(eps, dtype=np.float64).reshape(-1)
        if not (e >= 0).all():  # also refuses a NaN
            raise ValueError("eps must be >= 0")
        et = torch.as_tensor(e, dtype=torch.float32, device=device)
    if et.numel() == 1:
        et = et.expand(b)
    if et.numel() != b:
        raise ValueError(f"eps must be a number or one per row ({b}), got {et.numel()}")
    return et.contiguous()


def _labels_device(estimator, xt, y):
    if y is None:
        return estimator.own_labels_device(xt).argmax(dim=1).to(torch.int32).contiguous()
    yt = y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y))
    if yt.dim() == 2:
        yt = yt.argmax(dim=1)
    yt = yt.to(device=xt.device, dtype=torch.int32).reshape(-1).contiguous()
    if yt.numel() != xt.shape[0]:
        raise ValueError(f"y must hold one class per row ({xt.shape[0]}), got {yt.numel()}")
    return yt


class _Workspace:
    """The device floats lipasr_mlp_bounds works in, grown on demand and kept for the next chunk."""

    def __init__(self, model):
        self.model, self.buf = model, None

    def get(self, b):
        need = N.sz()
        N.check(N.lib.lipasr_mlp_bounds_workspace(self.model._plan, b, N.C.byref(need)))
        if self.buf is None or self.buf.numel() < need.value:
            self.buf = torch.empty(need.value, device="cuda", dtype=torch.float32)
        return self.buf, need.value


def _margins(estimator, xt, et, yt, norm, clip, method, ws, details=False):
    m = estimator.model
    b, c = xt.shape[0], estimator.nb_classes
    ibp = torch.empty(b, c, device=xt.device)
    crown = torch.empty(b, c, device=xt.device) if method == "crown-ibp" else None
    slack = torch.empty(b, c, device=xt.device) if (details and crown is not None) else None
    lo = hi = None
    if details:
        fam = N.bounds_family_floats(m._widths, 1)
        lo, hi = torch.empty(b * fam, device=xt.device), torch.empty(b * fam, device=xt.device)
    bs = estimator.batch_limit
    o = 0
    for s in range(0, b, bs):
        xb = xt[s:s + bs]
        n = xb.shape[0]
        buf, floats = ws.get(n)
        sl = lambda t: None if t is None else t[s:s + bs]
        fl = None if lo is None else (lo[o:], hi[o:])
        N.check(N.lib.lipasr_mlp_bounds(m._plan, N.ptr(m._params), N.ptr(m._bnstate), N.ptr(xb), N.ptr(et[s:s + bs]), norm, clip[0], clip[1],
                                        N.ptr(yt[s:s + bs]), n, N.ptr(buf), floats, N.ptr(ibp[s:s + bs]), N.ptr(sl(crown)), N.ptr(sl(slack)),
                                        N.ptr(None if fl is None else fl[0]), N.ptr(None if fl is None else fl[1]), N.stream_ptr()))
        if details:
            o += n * fam
    out = ibp if crown is None else torch.maximum(ibp, crown)
    if details:
        return out, {"margin_ibp": ibp, "margin_crown": crown, "slack": slack, "lo": lo, "hi": hi}
    return out


def bound_margins(estimator, x, eps, norm=float("inf"), y=None, method="crown-ibp", clip_values=None, details=False):
    """Lower bounds [B, classes] (device tensor) of z_y - z_k over the input set of every row: eps a number or one per row, y the
    class per row (ints or one-hot; default the estimator's own label).  Column y holds +inf, a row with a NaN holds NaN.  method
    "crown-ibp": max(IBP, CROWN-IBP) per entry; "ibp": the interval bounds alone (no backward pass).  A row is certified at its eps
    when its smallest entry is > 0.  ``details=True`` also returns what the native call wrote, chunk after chunk of batch_limit rows
    (margin_ibp, margin_crown, slack, and the flat boxes lo / hi of lipasr_mlp_bounds)."""
    norm = _check(estimator, norm, method)
    xt = estimator.rows_device(x)
    if xt.shape[0] == 0:
        out = torch.empty(0, estimator.nb_classes, device=xt.device)
        return (out, {}) if details else out
    et = _eps_device(eps, xt.shape[0], xt.device)
    yt = _labels_device(estimator, xt, y)
    return _margins(estimator, xt, et, yt, norm, _clip(estimator, clip_values), method, _Workspace(estimator.model), details)


def certified_radius(estimator, x, norm=float("inf"), y=None, eps_max=1.0, steps=12, method="crown-ibp", clip_values=None):
    """Per row (device tensor [B], float32) the largest eps the bisection tested at which the row was certified: every row carries
    its own bracket [lo, hi], starting at [0, eps_max] with the first test at eps_max; each of the ``steps`` steps is ONE
    lipasr_mlp_bounds call per chunk over the whole batch at the rows' current eps.  0 if no tested eps was certified, and 0 for a
    row that the classifier does not give the class y (with y=None no row is)."""
    norm = _check(estimator, norm, method)
    if not (float(eps_max) > 0 and np.isfinite(eps_max)) or int(steps) < 1:
        raise ValueError("eps_max must be a positive finite number and steps >= 1")
    xt = estimator.rows_device(x)
    b = xt.shape[0]
    if b == 0:
        return torch.zeros(0, device=xt.device)
    yt = _labels_device(estimator, xt, y)
    right = estimator.own_labels_device(xt).argmax(dim=1).to(torch.int32) == yt
    clip, ws = _clip(estimator, clip_values), _Workspace(estimator.model)
    lo = torch.zeros(b, device=xt.device)
    hi = torch.full((b,), float(eps_max), device=xt.device)
    best = torch.zeros(b, device=xt.device)
    eps = hi.clone()
    for _ in range(int(steps)):
        mm = _margins(estimator, xt, eps, yt, norm, clip, method, ws).amin(dim=1)
        cert = (mm > 0) & right
        best = torch.where(cert, torch.maximum(best, eps), best)
        lo = torch.where(cert, eps, lo)
        hi = torch.where(cert, hi, eps)
        eps = ((lo.double() + hi.double()) / 2).float()
    return best


def certified_accuracy(estimator, x, labels, grid, norm=float("inf"), method="crown-ibp", clip_values=None):
    """float64 NumPy array, one entry per eps of ``grid``: the share of rows that are classified as ``labels`` (ints or one-hot)
    and certified at that eps -- no perturbation within eps changes their class.  A lower bound of the robust accuracy at eps,
    as an attack's accuracy is an upper bound."""
    norm = _check(estimator, norm, method)
    xt = estimator.rows_device(x)
    yt = _labels_device(estimator, xt, labels)
    grid = [float(e) for e in grid]
    if xt.shape[0] == 0:
        return np.full(len(grid), np.nan)
    right = estimator.own_labels_device(xt).argmax(dim=1).to(torch.int32) == yt
    clip, ws = _clip(estimator, clip_values), _Workspace(estimator.model)
    out = []
    for e in grid:
        et = _eps_device(e, xt.shape[0], xt.device)
        mm = _margins(estimator, xt, et, yt, norm, clip, method, ws).amin(dim=1)
        out.append(float(((mm > 0) & right).double().mean().item()))
    return np.array(out)
