"""FusedAdam / FusedAdamW: the optimizer step of the reference's four training scripts -- clip_grad_norm_ + AdamW (train2.py),
Adam with L2 weight decay (train_pseudo.py, train_fundamental.py), GradScaler.step(optimizer) (train.py) -- as three HIP launches
over all parameters (csrc/pwc_optim.hip): the square sum of the gradients, a one-workgroup finish pass, the update.  No host
synchronisation in step().

Differences from torch.optim.Adam / AdamW + clip_grad_norm_, all deliberate:
  * max_grad_norm replaces the call of clip_grad_norm_: the clip coefficient is applied inside the update and p.grad is left
    UNMODIFIED (clip_grad_norm_ scales it in place).  last_grad_norm is the pre-clip total norm clip_grad_norm_ would have returned,
    as a 0-dim device tensor that the next step overwrites.
  * one step count per parameter group, kept on the device with beta1^step and beta2^step as running products in float64 (torch
    keeps a count per parameter and calls pow).  A parameter that gets its first gradient later than the rest of its group joins
    the group's count.  state_dict() writes the count into every parameter's `step` (one host read); load_state_dict() rebuilds
    the powers from it and refuses a group whose parameters disagree.
  * the kernels write through raw pointers; step() then bumps the version counter of every parameter it updated, so autograd's
    saved-tensor checks and PWCDCNet's cached inference plans see the update.
  * float32 ROCm-device parameters only; amsgrad, maximize, sparse and complex parameters are refused, and there is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.graph import increment_version
from torch.optim import Optimizer

from . import ops
from ._lib import PwcHipError

__all__ = ["FusedAdam", "FusedAdamW", "chunk_table"]


def chunk_table(numels: Sequence[int], chunk_elems: int) -> np.ndarray:
    """int32 [nchunks, 2] = (tensor, chunk): tensor i cut into ceil(numel / chunk_elems) chunks, in tensor order (an empty tensor has
    none).  One workgroup of the optimizer kernels takes one row."""
    if chunk_elems <= 0:
        raise ValueError("chunk_elems must be positive")
    rows = []
    for i, n in enumerate(numels):
        if n < 0:
            raise ValueError("negative numel")
        k = (int(n) + chunk_elems - 1) // chunk_elems
        if k >= 2 ** 31:
            raise ValueError("tensor %d has too many chunks" % i)
        if k:
            rows.append(np.stack([np.full(k, i, dtype=np.int32), np.arange(k, dtype=np.int32)], axis=1))
    if not rows:
        return np.zeros((0, 2), dtype=np.int32)
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def _check_param(p: torch.Tensor) -> None:
    if p.is_sparse or p.layout != torch.strided:
        raise TypeError("FusedAdam: sparse parameters are not supported")
    if p.is_complex():
        raise TypeError("FusedAdam: complex parameters are not supported")
    if p.dtype != torch.float32:
        raise TypeError("FusedAdam: parameters must be float32, got %s" % p.dtype)


class _Tables:
    """Device tables of one parameter set: everything but the gradient pointers stays until the set changes."""

    def __init__(self, params: List[torch.Tensor], group_sizes: List[int], state, chunk_elems: int):
        dev = params[0].device
        for p in params:
            if not p.is_cuda:
                raise PwcHipError("FusedAdam: parameter on %s: the HIP path needs device tensors and has no CPU fallback" % p.device)
            if p.device != dev:
                raise ValueError("FusedAdam: all parameters must be on one device (%s and %s)" % (dev, p.device))
            if not p.is_contiguous():
                raise ValueError("FusedAdam: parameters must be contiguous")
        self.device = dev
        self.pptrs = [p.data_ptr() for p in params]
        rec = np.zeros((len(params), 4), dtype=np.int64)
        for i, p in enumerate(params):
            st = state.get(p)
            rec[i, 0] = self.pptrs[i]
            if st:
                rec[i, 1], rec[i, 2] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            rec[i, 3] = p.numel()
        chunks = chunk_table([p.numel() for p in params], chunk_elems)
        self.nchunks = int(chunks.shape[0])
        # chunks [begin, begin + count) of each group: the groups' tensors are consecutive, so are their chunks
        self.group_chunks: List[Tuple[int, int]] = []
        first = np.searchsorted(chunks[:, 0], np.cumsum([0] + list(group_sizes)), side="left")
        for gi in range(len(group_sizes)):
            self.group_chunks.append((int(first[gi]), int(first[gi + 1] - first[gi])))
        self.ngroups = len(group_sizes)
        self.tensors = torch.from_numpy(rec).to(dev)
        self.chunks = torch.from_numpy(chunks).to(dev) if self.nchunks else None
        self.grads = torch.zeros(len(params), dtype=torch.int64, device=dev)
        self.gptrs: List[int] = [0] * len(params)
        nbytes = ops.optim_workspace_bytes(max(self.nchunks, 1), self.ngroups)
        self.workspace = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)


class _FusedAdamBase(Optimizer):
    _step_supports_amp_scaling = True     # GradScaler.step() hands grad_scale / found_inf over instead of unscaling and syncing
    _decoupled = False

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, *, amsgrad: bool = False,
                 maximize: bool = False):
        if amsgrad:
            raise ValueError("%s: amsgrad is not supported" % type(self).__name__)
        if maximize:
            raise ValueError("%s: maximize is not supported" % type(self).__name__)
        if isinstance(lr, torch.Tensor):
            raise TypeError("%s: lr must be a number (a tensor lr would need a host read every step)" % type(self).__name__)
        if not lr >= 0.0 or not eps >= 0.0 or not weight_decay >= 0.0:
            raise ValueError("lr, eps and weight_decay must be >= 0")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("betas must be in [0, 1)")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None = no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._tables: Optional[_Tables] = None
        self._steprec: Optional[torch.Tensor] = None      # device float64 [ngroups, 3] = (step, beta1^step, beta2^step)
        self._steprec_host: List[List[float]] = []        # what _steprec is (re)built from while it is None
        self._norm: Optional[torch.Tensor] = None
        self._chunk_elems: Optional[int] = None
        # the keys torch.optim.Adam's groups have, so that a state_dict of this class loads into Adam / AdamW and steps there
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=self._decoupled)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------ parameter set
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            _check_param(p)
        self._pull_steps()
        self._steprec_host.append([0.0, 1.0, 1.0])
        self._steprec = None
        self._tables = None

    def _pull_steps(self) -> None:
        """Device step records -> host (one synchronising read; only where the caller asks for state or changes the groups)."""
        if self._steprec is not None:
            self._steprec_host = self._steprec.cpu().tolist()

    def _flat_params(self) -> Tuple[List[torch.Tensor], List[int]]:
        params, sizes = [], []
        for group in self.param_groups:
            params.extend(group["params"])
            sizes.append(len(group["params"]))
        return params, sizes

    def _collect(self, params: List[torch.Tensor]):
        """This step's gradient addresses (0 = parameter left out), the tensors that must stay alive until the launches are queued,
        and whether the static tables have to be rebuilt (new state, or a parameter whose storage moved)."""
        t = self._tables
        dirty = t is None or len(t.pptrs) != len(params)
        gptrs, keep = [0] * len(params), []
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                continue
            if g.layout is not torch.strided:
                raise TypeError("FusedAdam: sparse gradients are not supported")
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                raise TypeError("FusedAdam: gradient must be float32 %s on %s, got %s %s on %s"
                                % (tuple(p.shape), p.device, g.dtype, tuple(g.shape), g.device))
            if not g.is_contiguous():
                g = g.contiguous()          # p.grad is only read, so a dense copy serves
                keep.append(g)
            if not self.state[p]:
                st = self.state[p]
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                dirty = True
            if not dirty and t.pptrs[i] != p.data_ptr():
                dirty = True
            gptrs[i] = g.data_ptr()
        return gptrs, keep, dirty

    def _hyper(self, group) -> Tuple[float, float, float, float, float, bool]:
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("%s: amsgrad / maximize are not supported" % type(self).__name__)
        lr = group["lr"]
        if isinstance(lr, torch.Tensor):
            raise TypeError("%s: lr must be a number" % type(self).__name__)
        b1, b2 = group["betas"]
        return (float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                bool(group.get("decoupled_weight_decay", self._decoupled)))

    # ------------------------------------------------------------------ the step
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Total norm of the gradients before clipping in the last step (what clip_grad_norm_ returns), a 0-dim float32 device
        tensor that the next step overwrites; None before the first clipped step.  Reading it is the caller's synchronisation."""
        return self._norm

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        hypers = [self._hyper(g) for g in self.param_groups]     # read at every step: schedulers and manual changes are seen
        params, sizes = self._flat_params()
        if not params:
            return loss
        gptrs, keep, dirty = self._collect(params)
        if not any(gptrs):
            return loss
        if dirty:
            if self._chunk_elems is None:
                self._chunk_elems = ops.optim_chunk_elems()
            self._tables = _Tables(params, sizes, self.state, self._chunk_elems)
        t = self._tables
        if t.nchunks == 0:
            return loss
        dev = t.device
        if self._steprec is None or self._steprec.device != dev:
            self._pull_steps()
            self._steprec = torch.tensor(self._steprec_host, dtype=torch.float64, device=dev).reshape(len(sizes), 3)
        if self._norm is None and self.max_grad_norm is not None:
            self._norm = torch.zeros((), dtype=torch.float32, device=dev)
        if gptrs != t.gptrs:
            # a NEW pinned block for every upload: torch's host allocator hands a block out again only after the copy that reads it
            # has finished, so no staging memory an earlier asynchronous copy may still read is ever overwritten
            stage = torch.empty(len(gptrs), dtype=torch.int64, pin_memory=True)
            stage.numpy()[:] = gptrs
            t.grads.copy_(stage, non_blocking=True)
            t.gptrs = gptrs
        found_inf, grad_scale = getattr(self, "found_inf", None), getattr(self, "grad_scale", None)
        clip = self.max_grad_norm
        if clip is not None:
            ops.optim_grad_sqsum(t.grads, t.tensors, t.chunks, t.nchunks, t.ngroups, t.workspace)
        for gi, (lr, b1, b2, eps, wd, decoupled) in enumerate(hypers):
            begin, count = t.group_chunks[gi]
            if count == 0:
                continue
            ops.optim_finish(t.workspace, t.nchunks, t.ngroups, gi, clip, found_inf, grad_scale, lr, b1, b2, self._steprec,
                             self._norm if clip is not None else None)
            ops.optim_adam_update(t.grads, t.tensors, t.chunks, t.nchunks, begin, count, t.ngroups, gi, t.workspace, lr, b1, b2,
                                  eps, wd, decoupled)
        # the kernels write through raw pointers: tell autograd (saved-tensor checks) and whoever caches by _version -- PWCDCNet's
        # inference plans are rebuilt from it -- that these parameters changed, as torch's own in-place updates do
        increment_version([p for p, g in zip(params, gptrs) if g])
        del keep
        return loss

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.Adam / AdamW's format: per parameter `step` (the group's count), `exp_avg`, `exp_avg_sq`."""
        self._pull_steps()
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = torch.tensor(float(self._steprec_host[gi][0]), dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        recs = []
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)
            _, b1, b2, _, _, _ = self._hyper(group)
            steps = set()
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                if "max_exp_avg_sq" in st:
                    raise ValueError("%s: the loaded state is an amsgrad one" % type(self).__name__)
                steps.add(float(st["step"]))
                for k in ("exp_avg", "exp_avg_sq"):
                    m = st[k]
                    if m.dtype != torch.float32 or m.shape != p.shape or m.device != p.device:
                        raise ValueError("%s: loaded %s does not match its parameter" % (type(self).__name__, k))
                    st[k] = m.contiguous()
            if len(steps) > 1:
                raise ValueError("%s: the parameters of a group were loaded with unequal step counts %s; this optimizer keeps one "
                                 "count per group" % (type(self).__name__, sorted(steps)))
            s = steps.pop() if steps else 0.0
            recs.append([s, b1 ** s, b2 ** s])       # the powers are rebuilt from the count
        self._steprec_host = recs
        self._steprec = None
        self._tables = None


class FusedAdam(_FusedAdamBase):
    """torch.optim.Adam (weight_decay = L2 term added to the gradient) with optional global-norm clipping, as HIP launches."""
    _decoupled = False


class FusedAdamW(_FusedAdamBase):
    """torch.optim.AdamW (decoupled weight decay) with optional global-norm clipping, as HIP launches."""
    _decoupled = True

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None, *, amsgrad: bool = False,
                 maximize: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, amsgrad=amsgrad, maximize=maximize)
