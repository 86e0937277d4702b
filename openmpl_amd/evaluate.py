"""Device-resident evaluator of a whole validation run: the host epilogue of OpenMPL's validate(), accumulated on the GPU.

Reference: lib/core/function_mpl.py:387-399 (criterion, four `.item()` per batch, AverageMeter), :474-494 (D2H copy, room
de-normalisation, all_preds / all_gts / all_3d_confs), :612-634 + evaluate() :670-785 (relative and absolute pass, conf_3d mask,
OUTPUT_IN_METER, per-action breakdown), lib/core/loss.py:39-146 (the criteria).  HIP kernels through the C ABI (mpl_eval_*,
csrc/evaluate.hip); no CPU path.  update() never synchronises; compute() is the one call that does.
With aligned="similarity" / "rigid" the run is also scored after a Procrustes alignment of every pose (PA-MPJPE, Protocol 2;
lib/utils/pose_utils.py:61-143, which nothing in the reference calls): mpl_procrustes_align, csrc/procrustes.hip.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import cabi
from ._marshal import ptr, vec3

CRITERIA = {"mpjpe": cabi.CRIT_MPJPE, "weighted_mpjpe": cabi.CRIT_WEIGHTED_MPJPE, "l1": cabi.CRIT_L1, "mse": cabi.CRIT_MSE,
            "mpjpe_kadkhoda": cabi.CRIT_MPJPE_KADKHODA}
ALIGNED = {None: None, "similarity": True, "rigid": False}         # -> scaling of procrustes_align


def _wrap(indices, n, what):
    out = []
    for k in indices:
        if not -n <= int(k) < n:
            raise IndexError("%s index %d is out of bounds for axis with size %d" % (what, int(k), n))     # what numpy raises
        out.append(int(k) % n)
    return out


class PoseEvaluator:
    """num_joints: J of the model's poses.  criterion: which loss.py module validate() was given; weight_axis: LOSS.WEIGHT_AXIS.
    joints: the selection `u` of `all_preds[:, u, :]` (default: all joints in order; entry 0 is the root of the relative pass).
    groups: the largest class id (Human3.6M actions: 16): a sample with id 1..groups is also scored in its own class.
    output_in_meter: DATASET.OUTPUT_IN_METER.  not_consider_kp: SELECTED joints deleted from mpjpe (np.delete semantics).
    keep_poses: capacity, in samples, of the device copy of all_preds / all_gts (0: none is kept).
    aligned: None, "similarity" or "rigid": also score every pose after PoseUtils.procrustes(target, output, scaling = True /
    False, reflection="best") over the selected joints whose conf_3d is > 0, in the de-normalised frame (PA-MPJPE): compute()
    gains "aligned".  A pose whose alignment is degenerate (fewer than 3 joints left, all points equal, collinear points) is NaN
    there, which the nan-aware sums skip joint by joint, exactly as they skip a masked joint: it adds 0 to pjpe and nothing to
    dist, and still counts in n_samples.  None (the default) changes nothing: state, launches and results are as without it."""

    def __init__(self, num_joints: int, criterion: str = "mpjpe", weight_axis: Optional[Sequence[float]] = None,
                 joints: Optional[Sequence[int]] = None, groups: Optional[int] = None, output_in_meter: bool = False,
                 not_consider_kp: Optional[Sequence[int]] = None, keep_poses: int = 0, device=None, aligned: Optional[str] = None):
        if criterion not in CRITERIA:
            raise ValueError("criterion must be one of %s" % ", ".join(sorted(CRITERIA)))
        if not (aligned is None or isinstance(aligned, str)) or aligned not in ALIGNED:
            raise ValueError("aligned must be None, 'similarity' or 'rigid' (got %r)" % (aligned,))
        self.aligned = aligned
        J = int(num_joints)
        if not 1 <= J <= 64:
            raise NotImplementedError("1 <= num_joints <= 64")
        self.num_joints = J
        self.sel = _wrap(joints, J, "joint") if joints is not None else list(range(J))
        if not 1 <= len(self.sel) <= 64:
            raise NotImplementedError("the joint selection holds 1 to 64 entries")
        self.n_groups = 1 + (int(groups) if groups else 0)
        if not 1 <= self.n_groups <= cabi.EVAL_MAX_GROUPS:
            raise NotImplementedError("group ids 1..%d at most" % (cabi.EVAL_MAX_GROUPS - 1))
        S = len(self.sel)
        self.skip_mask = 0
        for k in _wrap(not_consider_kp if not_consider_kp is not None else (), S, "not_consider_kp"):
            self.skip_mask |= 1 << k
        self.criterion = criterion
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PoseEvaluator has no CPU path: device must be a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._opt = cabi.EvalOptions()
        self._opt.criterion = CRITERIA[criterion]
        self._opt.has_weight_axis = int(weight_axis is not None)
        self._opt.weight_axis[:] = vec3(weight_axis, 1.0)
        self._opt.metre_factor = 100.0 if output_in_meter else 1.0
        self._opt.n_sel, self._opt.n_groups = S, self.n_groups
        for i, j in enumerate(self.sel):
            self._opt.sel[i] = j
        self._lib = cabi.load()
        nbytes = self._lib.mpl_eval_state_bytes(S, self.n_groups)
        if nbytes == 0:
            raise NotImplementedError("mpl_eval_state_bytes refused (n_sel %d, n_groups %d)" % (S, self.n_groups))
        self.keep_poses = int(keep_poses)
        self._alloc(nbytes)
        self._state_aligned = None
        if aligned is not None:
            # the aligned poses are scored by a second, separate state: plain MPJPE on poses that are de-normalised already
            self._opt_aligned = cabi.EvalOptions()
            self._opt_aligned.criterion = cabi.CRIT_MPJPE
            self._opt_aligned.weight_axis[:] = [1.0] * 3
            self._opt_aligned.scale[:] = [1.0] * 3
            self._opt_aligned.offset[:] = [0.0] * 3
            self._opt_aligned.metre_factor = self._opt.metre_factor
            self._opt_aligned.n_views = 1
            self._opt_aligned.n_sel, self._opt_aligned.n_groups = S, self.n_groups
            for i, j in enumerate(self.sel):
                self._opt_aligned.sel[i] = j
            self._alloc_aligned(nbytes)
        self.reset()

    def _alloc(self, nbytes):
        """State and kept poses (hook of the tests, which put a canary behind each)."""
        self._state = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
        self._keep = torch.zeros((2, self.keep_poses, self.num_joints, 3), dtype=torch.float32, device=self.device) \
            if self.keep_poses > 0 else None

    def _alloc_aligned(self, nbytes):
        """State of the aligned pass (only with aligned=...; the tests' hook like _alloc)."""
        self._state_aligned = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)

    def reset(self):
        for state in (self._state, self._state_aligned):
            if state is not None:
                cabi.launch("eval_reset", self.device, state.data_ptr(), len(self.sel), self.n_groups)
        self._fed = 0

    def _pose(self, t, shape, what):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise RuntimeError("PoseEvaluator has no CPU path: %s must live on %s" % (what, self.device))
        if t.dtype != torch.float32:
            raise RuntimeError("float32 tensors required (%s is %s)" % (what, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("%s: expected shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
        return t.contiguous()

    def update(self, output, target, weight=None, conf_3d=None, group=None, scale=None, offset=None, n_views: int = 1):
        """One batch, on the current stream, without any host synchronisation.  output: (B,J,3) float32, or the kadkhod tuple
        (poses, [x1, x2]) as the model returns it; target (B,J,3); weight (B,J) or (B,J,1); conf_3d (B,J) or (B,J,1): joints with
        conf_3d <= 0 are masked (indexed through the joint selection like the poses); group (B,) int32 class ids;
        scale / offset: room de-normalisation, a number or 3 values; n_views: len(input), the AverageMeter weight.
        With aligned=..., the poses (of the kadkhod tuple: the final ones) are also aligned to their targets and scored."""
        x1 = x2 = None
        if isinstance(output, (tuple, list)):
            output, inter = output
            if self.criterion == "mpjpe_kadkhoda":
                if len(inter) != 2:
                    raise RuntimeError("the kadkhod tuple is (poses, [x1, x2])")
                x1, x2 = inter
        elif self.criterion == "mpjpe_kadkhoda":
            raise RuntimeError("criterion mpjpe_kadkhoda scores the tuple (poses, [x1, x2])")
        if not isinstance(output, torch.Tensor) or output.ndim != 3 or output.shape[1:] != (self.num_joints, 3):
            if isinstance(output, torch.Tensor) and output.device != self.device:
                raise RuntimeError("PoseEvaluator has no CPU path: output must live on %s" % (self.device,))
            raise RuntimeError("expected (B,%d,3) poses" % self.num_joints)
        B, J = output.shape[0], self.num_joints
        if B < 1:
            raise RuntimeError("empty batch")
        output = self._pose(output, (B, J, 3), "output")
        target = self._pose(target, (B, J, 3), "target")
        if x1 is not None:
            x1, x2 = self._pose(x1, (B, J, 3), "x1"), self._pose(x2, (B, J, 3), "x2")
        needs_w = self.criterion == "weighted_mpjpe" or (self.criterion == "mpjpe" and self._opt.has_weight_axis)
        if needs_w:
            if weight is None:
                raise RuntimeError("criterion %s needs the weight tensor" % self.criterion)
            weight = self._pose(weight.reshape(B, J) if isinstance(weight, torch.Tensor) and weight.numel() == B * J else weight,
                                (B, J), "weight")
            if self.criterion == "mpjpe" and not (B == 1 or J == 1 or B == J):
                # loss.py:56: (B,J,1) * (B,J) does not broadcast -- torch raises this in the reference
                raise RuntimeError("The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1" % (J, B))
        else:
            weight = None
        if conf_3d is not None:
            conf_3d = self._pose(conf_3d.reshape(B, J) if isinstance(conf_3d, torch.Tensor) and conf_3d.numel() == B * J else conf_3d,
                                 (B, J), "conf_3d")
        if group is not None:
            if not isinstance(group, torch.Tensor) or group.device != self.device:
                raise RuntimeError("PoseEvaluator has no CPU path: group must live on %s" % (self.device,))
            if group.dtype != torch.int32:
                raise RuntimeError("group ids are int32 (got %s)" % group.dtype)
            if tuple(group.shape) != (B,):
                raise RuntimeError("group: expected shape (%d,), got %s" % (B, tuple(group.shape)))
            group = group.contiguous()
        elif self.n_groups > 1:
            raise RuntimeError("this evaluator scores groups: update() needs the group ids")
        if self._keep is not None and self._fed + B > self.keep_poses:
            raise RuntimeError("keep_poses=%d is too small for %d samples" % (self.keep_poses, self._fed + B))
        self._opt.scale[:] = vec3(scale, 1.0)
        self._opt.offset[:] = vec3(offset, 0.0)
        self._opt.n_views = int(n_views)
        if self._opt.n_views < 1:
            raise RuntimeError("n_views >= 1")

        keep = (None, None) if self._keep is None else self._keep
        cabi.launch("eval_accumulate", self.device, self._state.data_ptr(), C.byref(self._opt), output.data_ptr(), ptr(x1), ptr(x2),
                    target.data_ptr(), ptr(weight), ptr(conf_3d), ptr(group), B, J, ptr(keep[0]), ptr(keep[1]), self.keep_poses)
        if self._state_aligned is not None:
            self._update_aligned(output, target, conf_3d, group, B, J)
        self._fed += B

    def _update_aligned(self, output, target, conf_3d, group, B, J):
        """Align the batch to its targets with the selection, conf_3d and de-normalisation of this call (temporaries from the
        caching allocator, no host synchronisation) and accumulate it against the de-normalised targets."""
        from . import procrustes
        sc, of = list(self._opt.scale), list(self._opt.offset)
        z = torch.empty_like(output)
        d = torch.empty((B,), dtype=torch.float32, device=self.device)
        procrustes._launch(output, target, conf_3d, self.sel, ALIGNED[self.aligned], cabi.REFLECT_BEST, sc, of, B, J, z, d, None, None, None)
        if sc != [1.0] * 3 or of != [0.0] * 3:
            tgt = torch.empty_like(target)              # x * scale + offset per axis, as the kernels de-normalise (Python scalars:
            for a in range(3):                          # no host-to-device copy)
                torch.mul(target[..., a], sc[a], out=tgt[..., a]).add_(of[a])
            target = tgt
        cabi.launch("eval_accumulate", self.device, self._state_aligned.data_ptr(), C.byref(self._opt_aligned), z.data_ptr(), None, None,
                    target.data_ptr(), None, ptr(conf_3d), ptr(group), B, J, None, None, 0)

    def _report(self, state=None) -> torch.Tensor:
        """The raw report on the device (stream-ordered, no synchronisation)."""
        S = len(self.sel)
        state = self._state if state is None else state
        rep = torch.empty(self._lib.mpl_eval_report_size(S, self.n_groups), dtype=torch.float64, device=self.device)
        cabi.launch("eval_report", self.device, state.data_ptr(), S, self.n_groups, self.skip_mask, rep.data_ptr())
        return rep

    def compute(self) -> Dict:
        """What validate() logs and evaluate() returns, as numpy float64: {"relative": ..., "absolute": ...} each with pjpe (S),
        mpjpe, dist (S,3), dist_mean (3), n_samples and per_group {id: the same fields} (empty groups omitted, as the reference
        skips actions without samples); loss, loss_axis (3), n_samples.  With aligned=..., also "aligned": the fields of the
        absolute pass on the Procrustes-aligned poses (PA-MPJPE).  The one call that synchronises."""
        S, G = len(self.sel), self.n_groups
        ra = self._report(self._state_aligned) if self._state_aligned is not None else None
        r = self._report().cpu().numpy()
        # NaN poses of a failed forward would be skipped by nansum / nanmean: a poisoned state reports NaN, and a failure that is
        # still pending raises here, with the results it spoiled
        cabi.raise_if_device_error(self.device.index)
        out = dict(loss=r[0], loss_axis=r[1:4].copy(), n_samples=int(r[4]), poisoned=bool(r[5]))
        w = 4 * S + 5

        def fields(b):
            return dict(pjpe=b[:S].copy(), mpjpe=b[S], dist=b[S + 1:S + 1 + 3 * S].reshape(S, 3).copy(),
                        dist_mean=b[4 * S + 1:4 * S + 4].copy(), n_samples=int(b[4 * S + 4]))

        for p, name in enumerate(("absolute", "relative")):
            blocks = [r[8 + (p * G + g) * w:8 + (p * G + g + 1) * w] for g in range(G)]
            e = fields(blocks[0])
            e["per_group"] = {g: fields(blocks[g]) for g in range(1, G) if blocks[g][4 * S + 4] > 0}
            out[name] = e
        if ra is not None:
            ra = ra.cpu().numpy()
            blocks = [ra[8 + g * w:8 + (g + 1) * w] for g in range(G)]
            out["aligned"] = fields(blocks[0])
            out["aligned"]["per_group"] = {g: fields(blocks[g]) for g in range(1, G) if blocks[g][4 * S + 4] > 0}
        return out

    def poses(self):
        """The kept de-normalised (predictions, targets) of the run so far, (n,J,3) device tensors (views of the buffer)."""
        if self._keep is None:
            raise RuntimeError("keep_poses=0: no poses are kept")
        return self._keep[0, :self._fed], self._keep[1, :self._fed]
