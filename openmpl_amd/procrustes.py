"""Procrustes alignment of predicted poses onto their targets: the transform behind PA-MPJPE (Protocol 2).

Reference: lib/utils/pose_utils.py:61-143 PoseUtils.procrustes (a numpy port of MATLAB's procrustes: one 3x3 SVD per pose, on the
host).  Row vectors as there: aligned = scale * pred @ rotation + translation.  One HIP kernel through the C ABI
(mpl_procrustes_align, csrc/procrustes.hip) on the current stream; no synchronisation, no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import cabi
from ._marshal import ptr, vec3
from .evaluate import _wrap

REFLECTION = {"best": cabi.REFLECT_BEST, False: cabi.REFLECT_OFF, True: cabi.REFLECT_ON}


class ProcrustesResult(NamedTuple):
    aligned: torch.Tensor        # (B,J,3)
    d: torch.Tensor              # (B,)
    rotation: torch.Tensor       # (B,3,3)
    scale: torch.Tensor          # (B,)
    translation: torch.Tensor    # (B,3)


def _reflection(reflection) -> int:
    if isinstance(reflection, (str, bool)) and reflection in REFLECTION:
        return REFLECTION[reflection]
    raise ValueError("reflection must be 'best', False or True (got %r)" % (reflection,))


def _checked(pred, target, conf, joints):
    """Shapes first, then dtypes, then devices (so that each complaint names the argument it is about, with or without a GPU)
    -> contiguous float32 GPU tensors, the wrapped joint selection and the sizes."""
    if not isinstance(pred, torch.Tensor) or pred.ndim != 3 or pred.shape[2] != 3 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise RuntimeError("pred: expected shape (B,J,3), got %s" % (tuple(pred.shape) if isinstance(pred, torch.Tensor) else type(pred),))
    B, J, _ = pred.shape
    named = [("pred", pred, (B, J, 3)), ("target", target, (B, J, 3))]
    if conf is not None:
        if isinstance(conf, torch.Tensor) and conf.ndim == 3 and tuple(conf.shape) == (B, J, 1):
            conf = conf.reshape(B, J)
        named.append(("conf", conf, (B, J)))
    for what, t, shape in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise RuntimeError("%s: expected shape %s, got %s" % (what, shape, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    sel = None if joints is None else _wrap(joints, J, "joint")
    for what, t, _ in named:
        if t.dtype != torch.float32:
            raise RuntimeError("float32 tensors required (%s is %s)" % (what, t.dtype))
    for what, t, _ in named:
        if t.device.type != "cuda":
            raise RuntimeError("procrustes_align has no CPU path: %s must live on a GPU" % what)
        if t.device != pred.device:
            raise RuntimeError("%s is on %s, pred on %s" % (what, t.device, pred.device))
    if J > 64 or (sel is not None and not 1 <= len(sel) <= 64):
        raise NotImplementedError("at most 64 joints and a selection of 1 to 64 entries (got %d, %s)"
                                  % (J, "none" if sel is None else len(sel)))
    out = [t.contiguous() for _, t, _ in named]
    return out[0], out[1], (out[2] if conf is not None else None), sel, B, J


def _launch(pred, target, conf, sel, scaling, reflection, scale3, offset3, B, J, aligned, d, rotation, scale, translation):
    """mpl_procrustes_align on the current stream of pred's device; outputs are tensors or None."""
    sel_c = None if sel is None else (C.c_int * len(sel))(*sel)
    cabi.launch("procrustes_align", pred.device, pred.data_ptr(), target.data_ptr(), ptr(conf), sel_c, 0 if sel is None else len(sel),
                (C.c_float * 3)(*scale3), (C.c_float * 3)(*offset3), int(bool(scaling)), reflection, B, J, ptr(aligned), ptr(d), ptr(rotation),
                ptr(scale), ptr(translation))


def procrustes_align(pred: torch.Tensor, target: torch.Tensor, conf: Optional[torch.Tensor] = None,
                     joints: Optional[Sequence[int]] = None, scaling: bool = True, reflection="best", scale=None, offset=None
                     ) -> ProcrustesResult:
    """PoseUtils.procrustes(target[b], pred[b], scaling, reflection) for every pose of a batch: (aligned (B,J,3), d (B,), rotation
    (B,3,3), scale (B,), translation (B,3)) with aligned = scale * pred @ rotation + translation, d the residual sum of squares
    over the target's own spread.  The fit is over the joints of `joints` (default: all; negative indices wrap) whose `conf` (B,J)
    is > 0 and finite; `aligned` holds all J joints.  scale / offset: the room de-normalisation (a number or 3 values), applied to
    both tensors before the fit; the results are in the de-normalised frame.  scaling=False fits a rigid motion (scale 1).
    A pose with fewer than 3 joints taking part, with all its points equal, or with collinear points is NaN in every output.
    Coplanar points under reflection="best" give the proper rotation (det +1), where numpy's sign is arbitrary."""
    mode = _reflection(reflection)
    scale3, offset3 = vec3(scale, 1.0), vec3(offset, 0.0)
    pred, target, conf, sel, B, J = _checked(pred, target, conf, joints)
    dev = pred.device
    out = ProcrustesResult(torch.empty((B, J, 3), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                           torch.empty((B, 3, 3), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                           torch.empty((B, 3), dtype=torch.float32, device=dev))
    _launch(pred, target, conf, sel, scaling, mode, scale3, offset3, B, J, *out)
    return out
