"""The Python side of the attack kernels' row contract (csrc/row.h): what every low-level wrapper checks before it hands device
tensors to a kernel, and what every attack class does around its own loop -- resolve the clip range, check the estimator, turn
``y`` into int32 labels, and take NumPy in and give NumPy out.  Functions, not a base class: the restart and bookkeeping loops of
the attacks differ in what "best" means and stay in their classes."""
from __future__ import annotations

import math

import numpy as np
import torch

from .estimators import _as_given, _Estimator, _to_dev


def _dev_tensor(t, dtype, shape, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} device tensor {list(shape)}")
    return t


def rows2d(x, what, dims="[B, n]"):
    """The shape of ``x``, a contiguous float32 device tensor with two dimensions (``dims`` names them in the message)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous float32 device tensor {dims}")
    return x.shape


def clip_pair(clip_values):
    """(lo, hi) as floats for a kernel's clip_lo / clip_hi; None: no clamp."""
    return (-math.inf, math.inf) if clip_values is None else (float(clip_values[0]), float(clip_values[1]))


def resolve_clip_values(estimator, clip_values, unset):
    """An attack's ``clip_values`` keyword: ``unset`` (the class's default) takes the estimator's; None or (lo, hi) floats."""
    if clip_values is unset:
        clip_values = estimator.clip_values
    if clip_values is not None and not float(clip_values[0]) <= float(clip_values[1]):
        raise ValueError(f"clip_values = {clip_values}")
    return None if clip_values is None else (float(clip_values[0]), float(clip_values[1]))


def check_estimator(estimator, types=_Estimator, what="estimator"):
    """The estimator an attack runs over: one of ``types``, with the 1 to 32 classes the kernels read per row."""
    if not isinstance(estimator, types):
        raise TypeError(f"{what} must be a lipasr TensorFlowV2Classifier or WaveformClassifier")
    if not 1 <= estimator.nb_classes <= 32:
        raise ValueError(f"{estimator.nb_classes} classes; 1 to 32 are supported")


def labels_device(xt, yt, targeted, own):
    """int32 labels [B] on xt's device from ``yt``, one-hot [B, classes] or class indices [B]; None: ``own()`` (untargeted only),
    the attack's own default in either form -- who runs which forward pass for it, and when, stays with the attack."""
    if yt is None:
        if targeted:
            raise ValueError("Target labels `y` need to be provided for a targeted attack.")
        yt = own()
    yt = yt.to(xt.device)
    lab = yt.argmax(dim=1) if yt.dim() == 2 else yt
    if tuple(lab.shape) != (xt.shape[0],):
        raise ValueError(f"y must be one-hot [B, classes] or class indices [B], got {tuple(yt.shape)}")
    return lab.to(torch.int32).contiguous()


def generate_host(attack, x, y, *args):
    """``generate`` over ``attack.generate_device(xt, yt, *args)``: NumPy (or a tensor) in, the same kind out."""
    xt = _to_dev(x)
    yt = None if y is None else (y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y)))
    return _as_given(attack.generate_device(xt, yt, *args), x)
