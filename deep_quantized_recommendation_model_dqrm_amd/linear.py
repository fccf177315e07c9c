"""Drop-in for the reference's ``QuantLinear`` (quantization_supp/
quant_modules_not_quantize_grad.py:20-211), backed by libdqrm's f32-MFMA kernels
(csrc/dqrm_linear.hip; no CPU fallback).

The reference's drivers build every bot_l / top_l layer as
``QuantLinear(weight_bit, bias_bit, full_precision_flag, per_channel, quantize_activation)``
followed by ``set_param(nn.Linear)`` and call it as ``x, prev = layer(x, prev)``
(dlrm_s_pytorch_comm_grad.py:279-343, :574-612). This module keeps that constructor, the
buffer names and state-dict keys of ``set_param`` (:70-97), ``__repr__`` (:64-68) and the
``(y, None)`` return of the weight-only forward (:209, :211):

  * quantized forward (2 launches with per_channel, 3 without): dqrm_linear_wquant refreshes
    ``fc_scaling_factor``, ``weight_integer`` and ``bias_integer`` from the current weights
    (symmetric, the bias with the weight's scale), then dqrm_linear_fwd computes
    ``(x @ weight_integer.T + bias_integer) * fc_scaling_factor``;
  * full_precision_flag: ``x @ weight.T + bias`` on the same kernel;
  * backward (2 launches, 1 for a layer whose input needs no gradient): the STE of
    SymmetricQuantFunction (quant_utils.py:349-363), dqrm_linear_bwd.

Every sum is an f32 fmaf chain in ascending index (include/dqrm.h), so a row's output does not
depend on the batch it is part of and every data-parallel replica computes the same bits.

``QuantLinear.activation`` (None, "relu" or "sigmoid"; mlp.fuse_activations sets it) fuses the
activation that follows the layer in ``create_mlp`` into the same launches: dqrm_linear_fwd_act
applies it in the forward's epilogue and dqrm_linear_bwd_act multiplies ``dy`` by its derivative,
read from the saved output, where the STE's scale is applied.

Activation quantization (``quantize_activation=True`` with a one-element
``prev_act_scaling_factor`` p, from ``QuantAct`` or the layer before; q_m_n_q_g.py:150-161,
:193-196) runs the same launch counts on dqrm_linear_wquant_qact / _fwd_qact / _bwd_qact: the bias
is quantized with ``fc_scaling_factor * p``, which is also the ``correct_output_scale`` buffer
([1, out_features] with per_channel, [1, 1] without, a fresh tensor per forward), the operand is
``x / p`` and the layer returns ``(round(x/p @ weight_integer.T + bias_integer) *
correct_output_scale, correct_output_scale)``. A per-channel ``correct_output_scale`` cannot be
the next layer's p (more than one element): the reference fails there too.

Not built: asymmetric weights (the reference raises there too) and a ``prev_act_scaling_factor``
on a layer without ``quantize_activation`` (the drivers never pass one).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.nn import Parameter

from . import _lib as L
from .tables import _stream_handle


_ACTS = {None: L.DQRM_ACT_NONE, "relu": L.DQRM_ACT_RELU, "sigmoid": L.DQRM_ACT_SIGMOID}

# Counts the package's writes to a QuantLinear weight or bias through a raw pointer (a kernel
# handed ``data_ptr()``): torch's version counters do not see those, so mlp.MLPStack compares this
# epoch as well before it trusts the integers a layer holds.
_raw_write_epoch = 0


def note_raw_write() -> None:
    """Called by every place in the package that lets a kernel write a dense parameter in place."""
    global _raw_write_epoch
    _raw_write_epoch += 1


def raw_write_epoch() -> int:
    return _raw_write_epoch


def _check_input(x: torch.Tensor, layer: "QuantLinear") -> None:
    w = layer.weight
    if x.device.type != "cuda" or w.device.type != "cuda":
        raise L.DQRMError(f"QuantLinear runs on libdqrm's HIP kernels: input and layer must be on a GPU "
                          f"(got {x.device} / {w.device}); there is no CPU path")
    if x.device != w.device:
        raise ValueError(f"input on {x.device} but the layer on {w.device}")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != layer.in_features or not x.is_contiguous():
        raise ValueError(f"QuantLinear needs a contiguous float32 [B, {layer.in_features}] input "
                         f"(got {x.dtype} {tuple(x.shape)}, contiguous={x.is_contiguous()})")


class _LinearFn(torch.autograd.Function):
    """Autograd bridge over dqrm_linear_wquant / _fwd / _bwd (act == DQRM_ACT_NONE) or
    _fwd_act / _bwd_act. The backward reads the integers and scale the layer's latest forward
    wrote (the same ones unless the weights changed in between); with an activation it also reads
    the output, saved with x so that autograd's version check catches an in-place write to it."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner, quantized, act=L.DQRM_ACT_NONE):
        lib, c, st = owner._lib, owner._c_struct(), _stream_handle()
        if quantized:
            L.check(lib.dqrm_linear_wquant(C.byref(c), st), "dqrm_linear_wquant")
        y = torch.empty((x.shape[0], owner.out_features), dtype=torch.float32, device=x.device)
        if act == L.DQRM_ACT_NONE:
            L.check(lib.dqrm_linear_fwd(C.byref(c), int(quantized), x.data_ptr(), x.shape[0], y.data_ptr(), st),
                    "dqrm_linear_fwd")
            ctx.save_for_backward(x)
        else:
            L.check(lib.dqrm_linear_fwd_act(C.byref(c), int(quantized), act, x.data_ptr(), x.shape[0],
                                            y.data_ptr(), st), "dqrm_linear_fwd_act")
            ctx.save_for_backward(x, y)
        ctx.owner = owner
        ctx.quantized = quantized
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, *ys = ctx.saved_tensors
        owner = ctx.owner
        dy = dy.contiguous()
        B = x.shape[0]
        dw = torch.empty_like(owner.weight)
        db = torch.empty_like(owner.bias)
        if B == 0:
            return ((torch.empty_like(x) if ctx.needs_input_grad[0] else None), dw.zero_(), db.zero_(), None, None,
                    None)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        if ctx.act == L.DQRM_ACT_NONE:
            L.check(owner._lib.dqrm_linear_bwd(C.byref(owner._c_struct()), int(ctx.quantized), x.data_ptr(),
                                               dy.data_ptr(), B, None if dx is None else dx.data_ptr(),
                                               dw.data_ptr(), db.data_ptr(), _stream_handle()),
                    "dqrm_linear_bwd")
        else:
            L.check(owner._lib.dqrm_linear_bwd_act(C.byref(owner._c_struct()), int(ctx.quantized), ctx.act,
                                                   x.data_ptr(), ys[0].data_ptr(), dy.data_ptr(), B,
                                                   None if dx is None else dx.data_ptr(), dw.data_ptr(),
                                                   db.data_ptr(), _stream_handle()),
                    "dqrm_linear_bwd_act")
        return dx, dw, db, None, None, None


class MissingActScale(ValueError, NotImplementedError):
    """quantize_activation=True without a prev_act_scaling_factor (the reference hits a NameError
    there). A ValueError; also a NotImplementedError, which this call raised while the
    activation-quantized path did not exist."""


class _LinearQActFn(torch.autograd.Function):
    """Autograd bridge over dqrm_linear_wquant_qact / _fwd_qact / _bwd_qact. ``cos`` is the fresh
    correct_output_scale tensor the forward writes; the backward reads it, the saved ``prev`` and
    the integers and fc_scaling_factor the layer's latest forward wrote."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner, act, prev, cos):
        lib, c, st = owner._lib, owner._c_struct(), _stream_handle()
        L.check(lib.dqrm_linear_wquant_qact(C.byref(c), prev.data_ptr(), cos.data_ptr(), st),
                "dqrm_linear_wquant_qact")
        y = torch.empty((x.shape[0], owner.out_features), dtype=torch.float32, device=x.device)
        L.check(lib.dqrm_linear_fwd_qact(C.byref(c), act, x.data_ptr(), prev.data_ptr(), cos.data_ptr(), x.shape[0],
                                         y.data_ptr(), st), "dqrm_linear_fwd_qact")
        if act == L.DQRM_ACT_NONE:
            ctx.save_for_backward(x, prev, cos)
        else:
            ctx.save_for_backward(x, prev, cos, y)
        ctx.owner = owner
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, prev, cos, *ys = ctx.saved_tensors
        owner = ctx.owner
        dy = dy.contiguous()
        B = x.shape[0]
        dw = torch.empty_like(owner.weight)
        db = torch.empty_like(owner.bias)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        if B == 0:
            return dx, dw.zero_(), db.zero_(), None, None, None, None
        L.check(owner._lib.dqrm_linear_bwd_qact(C.byref(owner._c_struct()), ctx.act, x.data_ptr(),
                                                ys[0].data_ptr() if ys else None, dy.data_ptr(), prev.data_ptr(),
                                                cos.data_ptr(), B, None if dx is None else dx.data_ptr(),
                                                dw.data_ptr(), db.data_ptr(), _stream_handle()),
                "dqrm_linear_bwd_qact")
        return dx, dw, db, None, None, None, None


class QuantLinear(nn.Module):
    """quant_modules_not_quantize_grad.py:20-211 on libdqrm: constructor arguments, defaults,
    buffers and forward signature of the reference. ``activation`` (not a constructor argument:
    None, "relu" or "sigmoid") is the activation fused into the layer's kernels."""

    activation = None  # class default: a layer pickled before the attribute existed reads None

    def __init__(self, weight_bit=4, bias_bit=None, full_precision_flag=False, quant_mode="symmetric",
                 per_channel=False, fix_flag=False, weight_percentile=0, quantize_activation=False):
        super().__init__()
        self.full_precision_flag = full_precision_flag
        self.weight_bit = weight_bit
        self.quant_mode = quant_mode
        self.per_channel = per_channel
        self.fix_flag = fix_flag
        self.weight_percentile = weight_percentile
        self.bias_bit = bias_bit
        self.quantize_bias = bias_bit is not None
        self.counter = 0
        self.quantize_activation = quantize_activation
        self.__dict__["_c"] = None  # (key, L.Linear): rebuilt when a tensor's storage moves

    def __repr__(self):
        s = super().__repr__()
        return "(" + s + " weight_bit={}, full_precision_flag={}, quantize_fn={})".format(
            self.weight_bit, self.full_precision_flag, self.quant_mode)

    def set_param(self, linear):
        """q_m_n_q_g.py:70-97: take a Linear layer's weights; the buffers live where they do."""
        if getattr(linear, "bias", None) is None:
            raise ValueError("QuantLinear.set_param needs a Linear layer with a bias (the reference "
                             "quantizes it with the weight's scale)")
        self.in_features = linear.in_features
        self.out_features = linear.out_features
        dev = linear.weight.device
        self.register_buffer("fc_scaling_factor", torch.zeros(self.out_features, device=dev))
        self.register_buffer("correct_output_scale", torch.ones(self.out_features, device=dev))
        self.weight = Parameter(linear.weight.data.clone().float().contiguous())
        self.register_buffer("weight_integer", torch.zeros_like(self.weight), persistent=False)
        self.register_buffer("bias_integer", torch.zeros_like(linear.bias, dtype=torch.float32), persistent=False)
        self.register_buffer("weight_scaling_factor", torch.zeros(self.out_features, device=dev))
        self.register_buffer("error_compensation_weight", torch.zeros_like(self.weight), persistent=False)
        self.bias = Parameter(linear.bias.data.clone().float().contiguous())
        self.register_buffer("bias_scaling_factor", torch.zeros(self.out_features, device=dev))
        self.register_buffer("error_compensation_bias", torch.zeros_like(self.bias), persistent=False)
        self.__dict__["_c"] = None

    def fix(self):
        self.fix_flag = True

    def unfix(self):
        self.fix_flag = False

    # ------------------------------------------------------------ the C view of the layer
    @property
    def _lib(self):
        return L.load()

    def _c_struct(self) -> L.Linear:
        ts = (self.weight, self.bias, self.weight_integer, self.bias_integer, self.fc_scaling_factor)
        key = tuple(t.data_ptr() for t in ts) + (self.weight_bit, self.bias_bit, bool(self.per_channel))
        ent = self.__dict__["_c"]
        if ent is not None and ent[0] == key:
            return ent[1]
        for t in ts:
            if t.device != self.weight.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("QuantLinear needs contiguous float32 parameters and buffers on one device")
        c = L.Linear()
        c.in_features, c.out_features = self.in_features, self.out_features
        c.weight_bit = int(self.weight_bit)
        c.bias_bit = int(self.bias_bit) if self.bias_bit is not None else 0
        c.per_channel = int(bool(self.per_channel))
        c.weight, c.bias, c.weight_integer, c.bias_integer, c.scale = key[:5]
        self.__dict__["_c"] = (key, c)
        return c

    def _scale_buffer(self) -> None:
        """fc_scaling_factor as the reference leaves it: [out_features] with per_channel, [1]
        without (q_m_n_q_g.py:124-144), on the weight's device."""
        n = self.out_features if self.per_channel else 1
        s = self.fc_scaling_factor
        if s.numel() != n or s.device != self.weight.device:
            self.fc_scaling_factor = torch.zeros(n, dtype=torch.float32, device=self.weight.device)

    # ------------------------------------------------------------ forward
    def forward(self, x, prev_act_scaling_factor=None):
        """(y, None), as the reference's weight-only QuantLinear returns; with quantize_activation
        (y, correct_output_scale)."""
        if type(x) is tuple:
            prev_act_scaling_factor = x[1]
            x = x[0]
        quantized = not self.full_precision_flag
        if quantized:
            if self.quant_mode == "asymmetric":
                raise Exception("For weight, we only support symmetric quantization.")
            if self.quant_mode != "symmetric":
                raise ValueError("unknown quant mode: {}".format(self.quant_mode))
            if self.quantize_activation and prev_act_scaling_factor is None:
                raise MissingActScale("QuantLinear(quantize_activation=True) needs a prev_act_scaling_factor "
                                      "(QuantAct's act_scaling_factor or the previous layer's "
                                      "correct_output_scale)")
            if prev_act_scaling_factor is not None and not self.quantize_activation:
                raise NotImplementedError("a prev_act_scaling_factor on a QuantLinear without "
                                          "quantize_activation=True is not built (the reference's drivers never "
                                          "pass one)")
            if prev_act_scaling_factor is not None and (not isinstance(prev_act_scaling_factor, torch.Tensor)
                                                        or prev_act_scaling_factor.numel() != 1):
                got = (tuple(prev_act_scaling_factor.shape) if isinstance(prev_act_scaling_factor, torch.Tensor)
                       else type(prev_act_scaling_factor).__name__)
                raise ValueError(f"prev_act_scaling_factor must be a tensor of ONE element (got {got}); a "
                                 "per-channel correct_output_scale cannot feed the next layer, in the reference "
                                 "either")
            if self.bias_bit is None:
                raise TypeError("QuantLinear quantizes its bias: bias_bit must be an int")
        if "weight" not in self._parameters:
            raise RuntimeError("QuantLinear.set_param(linear) has not been called")
        activation = getattr(self, "activation", None)
        if not (activation is None or isinstance(activation, str)) or activation not in _ACTS:
            raise ValueError(f"QuantLinear.activation must be None, 'relu' or 'sigmoid' (got {activation!r})")
        act = _ACTS[activation]
        _check_input(x, self)
        if quantized:
            self._scale_buffer()
        if x.device.index != torch.cuda.current_device():
            with torch.cuda.device(x.device):
                return self._run_layer(x, quantized, act, prev_act_scaling_factor)
        return self._run_layer(x, quantized, act, prev_act_scaling_factor)

    def _run_layer(self, x, quantized, act, prev):
        if not (quantized and self.quantize_activation):
            return _LinearFn.apply(x, self.weight, self.bias, self, quantized, act), None
        if prev.dtype != torch.float32 or prev.device != x.device:
            raise ValueError(f"prev_act_scaling_factor must be float32 on the input's device (got {prev.dtype} on "
                             f"{prev.device})")
        # [1, O] / [1, 1] as q_m_n_q_g.py:161 leaves it; fresh per forward, so the scale the next
        # layer saved for its backward is never overwritten
        cos = torch.empty((1, self.out_features if self.per_channel else 1), dtype=torch.float32, device=x.device)
        y = _LinearQActFn.apply(x, self.weight, self.bias, self, act, prev.detach(), cos)
        self._buffers["correct_output_scale"] = cos
        return y, cos


__all__ = ["QuantLinear"]
