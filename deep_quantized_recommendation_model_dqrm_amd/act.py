"""Drop-in for the reference's ``QuantAct`` (quantization_supp/
quant_modules_not_quantize_grad.py:541-725), backed by libdqrm's kernels (csrc/dqrm_act.hip; no
CPU fallback).

The DLRM drivers build two of these when ``--quantize_activation`` is set
(dlrm_s_pytorch_tb_dp_one_parallel_comm.py:475-476): ``quant_input`` on the dense features and
``quant_feature_outputs`` (``fixed_point_quantization=True``) on the interaction's output; each
returns ``(y, act_scaling_factor)`` and the scale goes into the MLP stack that follows as its
first ``prev_act_scaling_factor`` (:857-876). This module keeps the reference's constructor,
buffer names, shapes and state-dict keys, ``__repr__``, ``fix`` / ``unfix`` and the tuple input:

  * forward (at most 3 launches, 1 for a fixed module): dqrm_act_quant_fwd updates the running
    range ``x_min`` / ``x_max`` from the batch ON THE DEVICE (the reference's
    ``if self.x_min == self.x_max`` reads the device back; this does not), forms
    ``act_scaling_factor`` and writes ``clamp(round(1/s * x), -n-1, n) * s``;
  * backward (1 launch; none for an input that needs no gradient, as ``quant_input``'s):
    dqrm_act_quant_bwd, ``(dy * s) / s``.

``x_min`` / ``x_max`` are updated in place. ``act_scaling_factor`` is a fresh ``[1]`` tensor on
every forward (the reference rebinds the buffer too), so a scale a later layer saved for its
backward is never overwritten.

Not built (NotImplementedError): ``act_percentile != 0``, ``quant_mode="asymmetric"``, the
integer-only ``fixedpoint_fn`` requantization of the CNN models (a ``pre_act_scaling_factor``
without ``fixed_point_quantization``) and its ``identity`` branch. The DLRM drivers use none of
them.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib as L
from .tables import _stream_handle


class _ActFn(torch.autograd.Function):
    """Autograd bridge over dqrm_act_quant_fwd / _bwd. ``scale`` is the fresh [1] tensor the
    forward writes the scale to; the backward reads it."""

    @staticmethod
    def forward(ctx, x, owner, scale):
        y = torch.empty_like(x)
        owner._run(x, y, scale)
        ctx.save_for_backward(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (scale,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        L.check(L.load().dqrm_act_quant_bwd(scale.data_ptr(), dy.data_ptr(), dy.numel(), dx.data_ptr(),
                                            _stream_handle()), "dqrm_act_quant_bwd")
        return dx, None, None


class QuantAct(nn.Module):
    """quant_modules_not_quantize_grad.py:541-725 on libdqrm: constructor arguments, defaults,
    buffers and forward signature of the reference."""

    def __init__(self, activation_bit=4, act_range_momentum=0.95, full_precision_flag=False, running_stat=True,
                 quant_mode="symmetric", fix_flag=False, act_percentile=0, fixed_point_quantization=False):
        super().__init__()
        self.activation_bit = activation_bit
        self.act_range_momentum = act_range_momentum
        self.full_precision_flag = full_precision_flag
        self.running_stat = running_stat
        self.quant_mode = quant_mode
        self.fix_flag = fix_flag
        self.act_percentile = act_percentile
        self.fixed_point_quantization = fixed_point_quantization

        self.register_buffer("x_min", torch.zeros(1))
        self.register_buffer("x_max", torch.zeros(1))
        self.register_buffer("act_scaling_factor", torch.zeros(1))

        self.register_buffer("pre_weight_scaling_factor", torch.ones(1))
        self.register_buffer("identity_weight_scaling_factor", torch.ones(1))
        self.__dict__["_ws"] = None  # the range pass's scratch (dqrm_act_quant_workspace_bytes)

    def __repr__(self):
        return "{0}(activation_bit={1}, " \
               "full_precision_flag={2}, quant_mode={3}, Act_min: {4:.2f}, " \
               "Act_max: {5:.2f})".format(self.__class__.__name__, self.activation_bit,
                                          self.full_precision_flag, self.quant_mode, self.x_min.item(),
                                          self.x_max.item())

    def fix(self):
        """fix the activation range by setting running stat to False"""
        self.running_stat = False
        self.fix_flag = True

    def unfix(self):
        """unfix the activation range by setting running stat to True"""
        self.running_stat = True
        self.fix_flag = False

    # ------------------------------------------------------------ the C call
    def _workspace(self, numel: int, device) -> torch.Tensor | None:
        need = int(L.load().dqrm_act_quant_workspace_bytes(numel))
        if need <= 0:
            return None
        ws = self.__dict__.get("_ws")
        if ws is None or ws.device != device or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
            self.__dict__["_ws"] = ws
        return ws

    def _run(self, x: torch.Tensor, y: torch.Tensor | None, scale: torch.Tensor) -> None:
        """dqrm_act_quant_fwd on x: the running range in place, y and scale written (y None: the
        range alone)."""
        c = L.ActQuant()
        c.activation_bit = int(self.activation_bit)
        c.running_stat = int(bool(self.running_stat))
        m = float(self.act_range_momentum)
        c.momentum = m
        c.one_minus_momentum = 1.0 - m  # rounded to float once, from the double, by ctypes
        c.x_min, c.x_max, c.scale = self.x_min.data_ptr(), self.x_max.data_ptr(), scale.data_ptr()
        ws = self._workspace(x.numel(), x.device) if self.running_stat else None
        L.check(L.load().dqrm_act_quant_fwd(C.byref(c), x.data_ptr(), x.numel(), None if y is None else y.data_ptr(),
                                            None if ws is None else ws.data_ptr(), _stream_handle()),
                "dqrm_act_quant_fwd")

    def _check_input(self, x: torch.Tensor) -> None:
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"QuantAct needs a tensor (got {type(x).__name__})")
        if x.device.type != "cuda":
            raise L.DQRMError(f"QuantAct runs on libdqrm's HIP kernels: the input must be on a GPU (got {x.device}); "
                              "there is no CPU path")
        for name in ("x_min", "x_max", "act_scaling_factor"):
            b = getattr(self, name)
            if b.device != x.device:
                raise ValueError(f"input on {x.device} but QuantAct.{name} on {b.device}: move the module first")
            if b.dtype != torch.float32 or b.numel() != 1:
                raise ValueError(f"QuantAct.{name} must be one float32")
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"QuantAct needs a contiguous float32 input (got {x.dtype}, "
                             f"contiguous={x.is_contiguous()})")

    # ------------------------------------------------------------ forward
    def forward(self, x, pre_act_scaling_factor=None, pre_weight_scaling_factor=None, identity=None,
                identity_scaling_factor=None, identity_weight_scaling_factor=None):
        """(y, act_scaling_factor); x itself with full_precision_flag (the range still follows)."""
        if type(x) is tuple:
            pre_act_scaling_factor = x[1]
            x = x[0]
        if self.quant_mode == "asymmetric":
            raise NotImplementedError("QuantAct: quant_mode='asymmetric' is not built (the DLRM drivers "
                                      "use symmetric activation quantization)")
        if self.quant_mode != "symmetric":
            raise ValueError("unknown quant mode: {}".format(self.quant_mode))
        if self.act_percentile != 0:
            raise NotImplementedError("QuantAct: act_percentile != 0 (a percentile range) is not built; "
                                      "the range is min / max of the batch")
        if identity is not None:
            raise NotImplementedError("QuantAct: the identity branch (fixedpoint_fn of the CNN models) is not built")
        if (not self.full_precision_flag and pre_act_scaling_factor is not None
                and not self.fixed_point_quantization):
            raise NotImplementedError("QuantAct: a pre_act_scaling_factor without fixed_point_quantization=True "
                                      "(the integer-only fixedpoint_fn requantization of the CNN models) is not "
                                      "built")
        self._check_input(x)
        if x.device.index != torch.cuda.current_device():
            with torch.cuda.device(x.device):
                return self._forward(x)
        return self._forward(x)

    def _forward(self, x):
        if self.full_precision_flag:
            if self.running_stat and x.numel():
                self._run(x, None, self.act_scaling_factor)
            return x
        # a fresh scale per forward: what a later layer saved for its backward stays as it was
        scale = torch.empty(1, dtype=torch.float32, device=x.device)
        if x.numel() == 0:  # nothing launched: the scale of the range as it stands
            scale.copy_(self.act_scaling_factor)
        y = _ActFn.apply(x, self, scale)
        self._buffers["act_scaling_factor"] = scale
        return y, scale


__all__ = ["QuantAct"]
