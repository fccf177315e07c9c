"""The head of the reference's model step, backed by libdqrm's kernels (csrc/dqrm_loss.hip; no
CPU fallback): ``DLRM_Net.forward``'s ``torch.clamp(p, min=loss_threshold, max=1.0 -
loss_threshold)`` (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:837-839, :877-879) and
``loss_fn_wrap`` (:193-212), ``BCELoss`` / ``MSELoss(reduction="mean")`` or, for ``wbce``,
``(loss_ws[T.long()] * BCELoss(reduction="none")(Z, T)).mean()``.

  * forward (1 launch, no memset): dqrm_loss_fwd clamps, forms the per-sample terms, sums them in
    an order that depends on the batch size alone (include/dqrm.h: 256 slots, then a fold) and
    writes the 0-dim loss; the same launch writes the gradient, so the backward recomputes nothing;
  * backward (1 launch; none when ``p`` needs no gradient): dqrm_loss_bwd, ``dp = grad_output * g``
    with the clamp's mask already in ``g``. ``grad_output`` is read on the device.

All arithmetic is float32. The reference keeps ``loss_ws`` in float64, so its wbce loss is a
float64 tensor; here the weights are cast to float32 once and the loss is float32. A wbce target
outside ``[0, len(loss_weights))`` reads no memory: the loss and that sample's gradient are NaN
(the reference raises an IndexError, or wraps a negative class around).
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .tables import _stream_handle

_KINDS = {"bce": L.DQRM_LOSS_BCE, "mse": L.DQRM_LOSS_MSE, "wbce": L.DQRM_LOSS_WBCE}


def _on(device):
    """The launch goes to the tensor's device, not to the current one."""
    if device.index != torch.cuda.current_device():
        return torch.cuda.device(device)
    return contextlib.nullcontext()


def parse_loss_weights(loss_weights) -> torch.Tensor:
    """A 1-D float32 tensor (on the CPU, or a tensor's own device) from a sequence, a tensor or
    the reference's ``--loss_weights`` string (``"1.0-1.0"``, parsed there with
    ``np.fromstring(..., dtype=float, sep="-")``)."""
    if isinstance(loss_weights, str):
        try:
            vals = [float(v) for v in loss_weights.split("-")]
        except ValueError:
            raise ValueError(f"loss_weights {loss_weights!r} is not numbers joined by '-'") from None
        w = torch.tensor(vals, dtype=torch.float64)
    elif isinstance(loss_weights, torch.Tensor):  # stays on its device: nothing is read back
        w = loss_weights.detach()
    else:
        w = torch.from_numpy(np.asarray(loss_weights, dtype=np.float64).copy())
    if w.dim() != 1 or w.numel() < 1:
        raise ValueError(f"loss_weights must be a non-empty 1-D list of class weights (got shape {tuple(w.shape)})")
    return w.to(torch.float32).contiguous()


class _LossFn(torch.autograd.Function):
    """Autograd bridge over dqrm_loss_fwd / _bwd: (E, Z) from (p, T); Z (None unless asked for)
    is not differentiable, and only p receives a gradient."""

    @staticmethod
    def forward(ctx, p, t, owner, want_z):
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        g = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        z = torch.empty_like(p) if want_z else None
        owner._run(p, t, loss, g, z, None)
        if g is not None:
            ctx.save_for_backward(g)
        if z is not None:
            ctx.mark_non_differentiable(z)
        return loss, z

    @staticmethod
    def backward(ctx, go, _gz):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        (g,) = ctx.saved_tensors
        if go.dtype != torch.float32 or go.device != g.device:
            go = go.to(device=g.device, dtype=torch.float32)
        go = go.contiguous()
        dp = torch.empty_like(g)
        with _on(g.device):
            L.check(L.load().dqrm_loss_bwd(g.data_ptr(), go.data_ptr(), g.numel(), dp.data_ptr(), _stream_handle()),
                    "dqrm_loss_bwd")
        return dp, None, None, None


class DLRMLoss(nn.Module):
    """The clamp and the mean loss of the DLRM drivers as one forward and one backward launch.

    ``loss_function``: "bce", "mse" or "wbce"; ``loss_weights`` (wbce): a sequence, a tensor or the
    reference's ``"1.0-1.0"`` string; ``loss_threshold``: the clamp is active only when
    ``0.0 < loss_threshold < 1.0``, as in ``DLRM_Net.forward``."""

    def __init__(self, loss_function="bce", loss_weights=None, loss_threshold=0.0):
        super().__init__()
        if loss_function not in _KINDS:
            raise ValueError(f"unknown loss_function {loss_function!r}: one of 'bce', 'mse', 'wbce'")
        if loss_function == "wbce" and loss_weights is None:
            raise ValueError("loss_function='wbce' needs loss_weights")
        self.loss_function = loss_function
        self.loss_threshold = float(loss_threshold)
        self.register_buffer("loss_ws", None if loss_weights is None else parse_loss_weights(loss_weights),
                             persistent=False)

    def extra_repr(self):
        return f"loss_function={self.loss_function!r}, loss_threshold={self.loss_threshold}"

    # ------------------------------------------------------------ the C call
    def _config(self) -> L.Loss:
        c = L.Loss()
        c.kind = _KINDS[self.loss_function]
        th = self.loss_threshold
        c.clamp = int(0.0 < th < 1.0)
        c.lo = th        # rounded to float once, from the double, by ctypes: what torch.clamp
        c.hi = 1.0 - th  # compares an f32 tensor with for these Python scalars
        if self.loss_function == "wbce":
            c.num_weights = self.loss_ws.numel()
            c.weights = self.loss_ws.data_ptr()
        return c

    def _run(self, p, t, loss, g, z, terms) -> None:
        c = self._config()
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        with _on(p.device):
            L.check(L.load().dqrm_loss_fwd(C.byref(c), p.data_ptr(), t.data_ptr(), p.numel(), loss.data_ptr(), ptr(g),
                                           ptr(z), ptr(terms), _stream_handle()), "dqrm_loss_fwd")

    def _check(self, p, t) -> None:
        if not isinstance(p, torch.Tensor) or not isinstance(t, torch.Tensor):
            raise TypeError("DLRMLoss needs two tensors (the prediction and the target)")
        for name, x in (("prediction", p), ("target", t)):
            if x.dtype != torch.float32 or not x.is_contiguous():
                raise ValueError(f"DLRMLoss needs a contiguous float32 {name} (got {x.dtype}, "
                                 f"contiguous={x.is_contiguous()})")
        if not (p.dim() == 1 or (p.dim() == 2 and p.shape[1] == 1)):
            raise ValueError(f"DLRMLoss needs a [B, 1] or [B] prediction (got {tuple(p.shape)})")
        if t.numel() != p.numel():
            raise ValueError(f"prediction has {p.numel()} elements, target {t.numel()}")
        if not 1 <= p.numel() <= L.DQRM_LOSS_MAX_BATCH:
            raise ValueError(f"DLRMLoss takes 1..{L.DQRM_LOSS_MAX_BATCH} samples (got {p.numel()})")
        if p.device.type != "cuda":
            raise L.DQRMError(f"DLRMLoss runs on libdqrm's HIP kernels: the prediction must be on a GPU "
                              f"(got {p.device}); there is no CPU path")
        if t.device != p.device:
            raise ValueError(f"prediction on {p.device} but target on {t.device}: move the target first")
        if self.loss_function == "wbce":
            w = self.loss_ws
            if w is None or w.dtype != torch.float32 or w.dim() != 1 or w.numel() < 1 or not w.is_contiguous():
                raise ValueError("DLRMLoss.loss_ws must be a non-empty contiguous 1-D float32 tensor")
            if w.device != p.device:
                raise ValueError(f"prediction on {p.device} but DLRMLoss.loss_ws on {w.device}: move the module "
                                 "first")

    # ------------------------------------------------------------ forward
    def forward(self, p, T, return_clamped=False):
        """E, the 0-dim float32 loss; (E, Z) with return_clamped, Z the clamped prediction
        (``DLRM_Net.forward``'s return value), detached."""
        self._check(p, T)
        E, Z = _LossFn.apply(p, T, self, bool(return_clamped))
        return (E, Z) if return_clamped else E


def loss_fn_wrap(Z, T, loss_function="bce", loss_ws=None, loss_threshold=0.0):
    """The functional form under the reference's name (loss_fn_wrap, :193-212): the loss of Z
    against T (moved to Z's device, as the reference's ``T.to(device)``). With the default
    ``loss_threshold=0`` the clamp stays where the reference has it, in ``DLRM_Net.forward``."""
    if loss_function not in _KINDS:
        raise ValueError(f"unknown loss_function {loss_function!r}: one of 'bce', 'mse', 'wbce'")
    if loss_function == "wbce" and loss_ws is None:
        raise ValueError("loss_function='wbce' needs loss_ws")
    head = DLRMLoss(loss_function, loss_ws if loss_function == "wbce" else None, loss_threshold)
    if isinstance(Z, torch.Tensor) and isinstance(T, torch.Tensor):
        head = head.to(Z.device)
        T = T.to(Z.device)
    return head(Z, T)


__all__ = ["DLRMLoss", "loss_fn_wrap", "parse_loss_weights"]
