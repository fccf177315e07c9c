"""The reference's MLP stacks (DLRM_Net.create_mlp / apply_mlp, dlrm_s_pytorch_comm_grad.py:279-343,
:574-612) on package QuantLinear layers, with the activation after each layer fused into the
layer's own kernels.

create_mlp returns a ModuleList ``[QuantLinear, ReLU, QuantLinear, ReLU, ..., QuantLinear,
Sigmoid]``. The activations run between libdqrm's forward launches and their backward between its
backward launches: one elementwise kernel each way per layer, reading and writing a [B, out]
tensor the layer's epilogue had in registers. ``fuse_activations`` sets ``QuantLinear.activation``
(dqrm_linear_fwd_act / _bwd_act apply it, see linear.py) and puts a ``FusedActivation`` placeholder
where the torch module was, so positions, state-dict keys (``bot_l.0.weight``, ``bot_l.2.weight``,
...) and the reference's apply_mlp loop stay as they are. A training step of a bottom and a top
stack of 7 layers goes from 41 launches to 27.

A model built by the reference's own create_mlp is converted in place:

    fuse_activations(dlrm.bot_l); fuse_activations(dlrm.top_l)
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .linear import QuantLinear

_KINDS = {"relu": nn.ReLU, "sigmoid": nn.Sigmoid}


class FusedActivation(nn.Module):
    """Stands where an nn.ReLU / nn.Sigmoid stood whose work the preceding QuantLinear now does.
    No parameters, no buffers, no launch: forward returns its input."""

    def __init__(self, kind: str):
        super().__init__()
        if kind not in _KINDS:
            raise ValueError(f"FusedActivation kind must be 'relu' or 'sigmoid' (got {kind!r})")
        self.kind = kind

    def forward(self, x):
        return x

    def extra_repr(self):
        return f"{self.kind}, fused into the preceding QuantLinear"


def _kind_of(module):
    for kind, cls in _KINDS.items():
        if type(module) is cls:
            return kind
    return None


def fuse_activations(layers) -> int:
    """In place on a ModuleList or list: every nn.ReLU / nn.Sigmoid directly after a package
    QuantLinear without an activation becomes a FusedActivation and the layer's ``activation`` is
    set. Everything else is left alone. Returns the number of pairs fused (0 on a second call)."""
    fused = 0
    for i in range(1, len(layers)):
        prev, kind = layers[i - 1], _kind_of(layers[i])
        if kind is None or not isinstance(prev, QuantLinear) or getattr(prev, "activation", None) is not None:
            continue
        prev.activation = kind
        layers[i] = FusedActivation(kind)
        fused += 1
    return fused


def unfuse_activations(layers) -> int:
    """The inverse of fuse_activations: every FusedActivation directly after a QuantLinear carrying
    that activation becomes the torch module again and the layer's ``activation`` None. Returns the
    number of pairs restored."""
    restored = 0
    for i in range(1, len(layers)):
        prev, cur = layers[i - 1], layers[i]
        if not isinstance(cur, FusedActivation) or not isinstance(prev, QuantLinear):
            continue
        if getattr(prev, "activation", None) != cur.kind:
            continue
        prev.activation = None
        layers[i] = _KINDS[cur.kind]()
        restored += 1
    return restored


def create_mlp(ln, sigmoid_layer, weight_bit=4, full_precision_flag=False, per_channel=False, fused=True,
               quantize_activation=False):
    """DLRM_Net.create_mlp with every layer a package QuantLinear (bias_bit = weight_bit). Layer i
    maps ln[i] -> ln[i + 1] features; its weight is drawn from N(0, 2 / (m + n)) as an [m, n]
    array and then its bias from N(0, 1 / m), both from numpy's global generator and cast to
    float32, in that order, layer after layer (the reference's initialisation and draw sequence).
    A Sigmoid follows layer ``sigmoid_layer``, a ReLU every other. fused: fuse_activations.
    quantize_activation is passed to every layer (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:280,
    :323): the stack then needs apply_mlp's prev_act_scaling_factor, from a QuantAct."""
    ln = [int(v) for v in np.asarray(ln).reshape(-1)]
    layers = nn.ModuleList()
    for i, (n, m) in enumerate(zip(ln[:-1], ln[1:])):
        lin = nn.Linear(n, m, bias=True)
        W = np.random.normal(0.0, np.sqrt(2 / (m + n)), size=(m, n)).astype(np.float32)
        b = np.random.normal(0.0, np.sqrt(1 / m), size=m).astype(np.float32)
        lin.weight.data = torch.from_numpy(W)
        lin.bias.data = torch.from_numpy(b)
        q = QuantLinear(weight_bit=weight_bit, bias_bit=weight_bit, full_precision_flag=full_precision_flag,
                        per_channel=per_channel, quantize_activation=quantize_activation)
        q.set_param(lin)
        layers.append(q)
        layers.append(nn.Sigmoid() if i == sigmoid_layer else nn.ReLU())
    if fused:
        fuse_activations(layers)
    return layers


def apply_mlp(x, layers, prev_act_scaling_factor=None):
    """DLRM_Net.apply_mlp's loop (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:550, :592): a
    QuantLinear is called with, and returns, the activation scale beside the tensor; any other
    module maps the tensor. prev_act_scaling_factor: the scale of the QuantAct before the stack
    (layers built with quantize_activation), None for weight-only layers."""
    for layer in layers:
        if isinstance(layer, QuantLinear):
            x, prev_act_scaling_factor = layer(x, prev_act_scaling_factor)
        else:
            x = layer(x)
    return x


__all__ = ["FusedActivation", "fuse_activations", "unfuse_activations", "create_mlp", "apply_mlp"]
