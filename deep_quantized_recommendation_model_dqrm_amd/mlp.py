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

``MLPStack`` runs a fused stack as a whole: one host call for its forward, one for its backward
(dqrm_mlp_fwd / dqrm_mlp_bwd, which issue the per-layer launches), and ``sgd_step``, one launch
that updates every layer and requantizes it, so the next forward launches no quantization: the
same step goes from 27 launches plus the optimizer's to 22. A ``quantize_activation`` stack runs the
same way on dqrm_mlp_fwd_qact / dqrm_mlp_bwd_qact: ``y, out_scale = stack(x, prev_act_scaling_factor)``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .linear import _ACTS, MissingActScale, QuantLinear, _check_input, raw_write_epoch
from .tables import _stream_handle

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


# ------------------------------------------------------------------ the stack as one host call
def _on_device(dev, fn, *args):
    """fn(*args) with dev as torch's current device."""
    if dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return fn(*args)
    return fn(*args)


class _StackFn(torch.autograd.Function):
    """One autograd node for a whole stack, over (x, *weights, *biases): one dqrm_mlp_fwd and one
    dqrm_mlp_bwd. Every layer's output is a torch tensor saved for the backward (an activation's
    derivative is read from it, and it is the next layer's input)."""

    @staticmethod
    def forward(ctx, x, stack, c, fresh, *params):
        B = x.shape[0]
        ys = [torch.empty((B, l.out_features), dtype=torch.float32, device=x.device) for l in stack.layers]
        yp = stack._PtrArray(*[y.data_ptr() for y in ys])
        L.check(stack._lib.dqrm_mlp_fwd(C.byref(c), L.DQRM_MLP_FRESH if fresh else 0, x.data_ptr(), B, yp,
                                        _stream_handle()), "dqrm_mlp_fwd")
        ctx.save_for_backward(x, *ys)
        ctx.stack = stack
        return ys[-1]

    @staticmethod
    def backward(ctx, dy):
        x, *ys = ctx.saved_tensors
        stack = ctx.stack
        layers = stack.layers
        dy = dy.contiguous()
        B = x.shape[0]
        dws = [torch.empty_like(l.weight) for l in layers]
        dbs = [torch.empty_like(l.bias) for l in layers]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        if B == 0:
            return (dx, None, None, None, *[t.zero_() for t in dws], *[t.zero_() for t in dbs])
        scratch = torch.empty(2 * B * stack._max_hidden, dtype=torch.float32, device=x.device)
        A = stack._PtrArray
        L.check(stack._lib.dqrm_mlp_bwd(C.byref(stack._c_struct()), x.data_ptr(), A(*[y.data_ptr() for y in ys]),
                                        dy.data_ptr(), B, None if dx is None else dx.data_ptr(),
                                        A(*[t.data_ptr() for t in dws]), A(*[t.data_ptr() for t in dbs]),
                                        scratch.data_ptr(), scratch.numel() * 4, _stream_handle()),
                "dqrm_mlp_bwd")
        return (dx, None, None, None, *dws, *dbs)


class _StackQActFn(torch.autograd.Function):
    """_StackFn for a quantize_activation stack: one dqrm_mlp_fwd_qact and one dqrm_mlp_bwd_qact.
    ``scales`` are the fresh correct_output_scale tensors the forward writes, one per layer; the
    backward reads them and the saved ``prev``."""

    @staticmethod
    def forward(ctx, x, stack, c, fresh, prev, scales, *params):
        B = x.shape[0]
        ys = [torch.empty((B, l.out_features), dtype=torch.float32, device=x.device) for l in stack.layers]
        A = stack._PtrArray
        L.check(stack._lib.dqrm_mlp_fwd_qact(C.byref(c), L.DQRM_MLP_FRESH if fresh else 0, x.data_ptr(),
                                             prev.data_ptr(), A(*[s.data_ptr() for s in scales]), B,
                                             A(*[y.data_ptr() for y in ys]), _stream_handle()), "dqrm_mlp_fwd_qact")
        ctx.save_for_backward(x, prev, *scales, *ys)
        ctx.stack = stack
        return ys[-1]

    @staticmethod
    def backward(ctx, dy):
        stack = ctx.stack
        layers = stack.layers
        n = len(layers)
        x, prev, *rest = ctx.saved_tensors
        scales, ys = rest[:n], rest[n:]
        dy = dy.contiguous()
        B = x.shape[0]
        dws = [torch.empty_like(l.weight) for l in layers]
        dbs = [torch.empty_like(l.bias) for l in layers]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        if B == 0:
            return (dx, None, None, None, None, None, *[t.zero_() for t in dws], *[t.zero_() for t in dbs])
        scratch = torch.empty(2 * B * stack._max_hidden, dtype=torch.float32, device=x.device)
        A = stack._PtrArray
        L.check(stack._lib.dqrm_mlp_bwd_qact(C.byref(stack._c_struct()), x.data_ptr(), A(*[y.data_ptr() for y in ys]),
                                             dy.data_ptr(), prev.data_ptr(), A(*[s.data_ptr() for s in scales]), B,
                                             None if dx is None else dx.data_ptr(), A(*[t.data_ptr() for t in dws]),
                                             A(*[t.data_ptr() for t in dbs]), scratch.data_ptr(),
                                             scratch.numel() * 4, _stream_handle()), "dqrm_mlp_bwd_qact")
        return (dx, None, None, None, None, None, *dws, *dbs)


class MLPStack:
    """A ``create_mlp`` stack run as a whole: ``stack(x)`` is one host call each way
    (dqrm_mlp_fwd / dqrm_mlp_bwd, the per-layer launches and bits of ``apply_mlp``), and
    ``stack.sgd_step(lr)`` is one launch that applies SGD to every layer and leaves the layers'
    integers and scales current, so that the next forward quantizes nothing (dqrm_mlp_sgd).

    A plain object bound to a fused ModuleList or list; it owns nothing. The list, its modules,
    positions and state-dict keys stay as they are, ``apply_mlp`` and the DP hooks keep working on
    it, and ``fc_scaling_factor``, ``weight_integer`` and ``bias_integer`` of the layers are the
    buffers the kernels write.

        self.bot_stack = MLPStack(self.bot_l)      # after fuse_activations / create_mlp
        x = self.bot_stack(dense_x)                # in apply_mlp's place
        loss.backward()
        self.bot_stack.sgd_step(lr)                # the MLP parameters are in no torch optimizer

    Freshness. A forward skips the weight quantization only while the stack is fresh. Only
    ``sgd_step(requantize=True)`` and ``requantize()`` make it fresh, and they record every
    parameter's and buffer's ``data_ptr()``, every parameter's ``_version``, the bit widths and
    ``per_channel`` of the layers, and the package's raw-write epoch (linear.note_raw_write: the DP
    hooks' dense update and weight sync). A forward is fresh only if all of them still match, so an
    optimizer step, ``load_state_dict``, a replaced ``.data`` or a changed ``weight_bit`` is caught.
    The one hole: an in-place write through ``.data`` (``p.data.add_()``) does not bump
    ``p._version``; after such a write call ``invalidate()``.

    ``quantize_activation`` stacks (every layer quantized and built with
    ``quantize_activation=True``; only the last may be ``per_channel``) are called as ``apply_mlp``
    threads them: ``y, out_scale = stack(x, prev_act_scaling_factor)``, one dqrm_mlp_fwd_qact and
    one dqrm_mlp_bwd_qact. "Fresh" then means that the weight integers and ``fc_scaling_factor``
    are current: ``bias_integer`` and ``correct_output_scale`` depend on the activation scale and
    are rewritten by every forward, in ONE launch for all layers while the stack is fresh
    (dqrm_mlp_qact_prepare). ``sgd_step``, ``requantize`` and ``invalidate`` are the same calls.

    Not built: the CPU description of a ``quantize_activation`` stack (such a stack must be built
    from layers on a GPU; NotImplementedError otherwise), momentum, weight decay and other
    optimizers."""

    def __init__(self, layers):
        self.module_list = layers  # the list the stack is bound to, left as it is
        self.layers: list[QuantLinear] = []
        items = list(layers)
        for i, m in enumerate(items):
            if isinstance(m, QuantLinear):
                self.layers.append(m)
            elif isinstance(m, FusedActivation) and i > 0 and isinstance(items[i - 1], QuantLinear) \
                    and getattr(items[i - 1], "activation", None) == m.kind:
                continue
            else:
                raise ValueError(f"MLPStack needs a fused stack: element {i} is {type(m).__name__}, but every "
                                 "QuantLinear must be followed by a FusedActivation or nothing "
                                 "(call fuse_activations(layers) first)")
        if not self.layers:
            raise ValueError("MLPStack needs at least one QuantLinear")
        if len(self.layers) > L.DQRM_MLP_MAX_LAYERS:
            raise ValueError(f"MLPStack takes at most {L.DQRM_MLP_MAX_LAYERS} layers (got {len(self.layers)})")
        for i, l in enumerate(self.layers):
            if "weight" not in l._parameters:
                raise RuntimeError(f"layer {i}: QuantLinear.set_param(linear) has not been called")
            if i and l.in_features != self.layers[i - 1].out_features:
                raise ValueError(f"layer {i} takes {l.in_features} features but layer {i - 1} returns "
                                 f"{self.layers[i - 1].out_features}")
        n = len(self.layers)
        # an integer-activation stack: its quantized layers all take a prev_act_scaling_factor
        self._qact = any(l.quantize_activation and not l.full_precision_flag for l in self.layers)
        if self._qact:
            self._check_qact()
            if any(l.weight.device.type != "cuda" for l in self.layers):
                raise NotImplementedError("MLPStack: the CPU description of a quantize_activation=True stack is "
                                          "not built; move the layers to a GPU first")
        self._PtrArray = C.c_void_p * n
        self._max_hidden = max([l.out_features for l in self.layers[:-1]], default=0)
        self._c = None          # (key, L.MLP, the ctypes arrays it points into)
        self._fresh = None      # the freshness record, or None
        self._workspace = None  # dqrm_mlp_sgd's row maxima (per-tensor layers), allocated once

    def _check_qact(self):
        """What dqrm_mlp_fwd_qact rejects in the layers' settings, as Python errors."""
        for i, l in enumerate(self.layers):
            if l.full_precision_flag or not l.quantize_activation:
                raise ValueError(f"MLPStack: layer {i} is {'full precision' if l.full_precision_flag else 'weight-only'}"
                                 " in a quantize_activation stack: the activation scale is handed from layer to "
                                 "layer, so every layer must be quantized with quantize_activation=True")
            if l.per_channel and i + 1 < len(self.layers):
                raise ValueError(f"MLPStack: layer {i} is per_channel in a quantize_activation stack: only the last "
                                 "layer may be (a per-channel correct_output_scale cannot feed the next layer, in "
                                 "the reference either)")

    # ------------------------------------------------------------ the C view of the stack
    @property
    def _lib(self):
        return L.load()

    def _key(self):
        """Everything the C struct is built from: the layers' storage and settings."""
        k = []
        for l in self.layers:
            k += [l.weight.data_ptr(), l.bias.data_ptr(), l.weight_integer.data_ptr(), l.bias_integer.data_ptr(),
                  l.fc_scaling_factor.data_ptr(), l.weight_bit, l.bias_bit, bool(l.per_channel),
                  bool(l.full_precision_flag), l.quant_mode, bool(l.quantize_activation),
                  getattr(l, "activation", None)]
        return tuple(k)

    def _state(self, key=None):
        """The freshness record: the key, every parameter's version, the raw-write epoch."""
        return (self._key() if key is None else key,
                tuple(p._version for l in self.layers for p in (l.weight, l.bias)), raw_write_epoch())

    def _c_struct(self, key=None) -> L.MLP:
        key = self._key() if key is None else key  # a caller that has just computed it passes it on
        if self._c is not None and self._c[0] == key:
            return self._c[1]
        n = len(self.layers)
        lin, quantized, act = (L.Linear * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
        dev = self.layers[0].weight.device
        for i, l in enumerate(self.layers):
            q = not l.full_precision_flag
            if q:
                if l.quant_mode == "asymmetric":
                    raise Exception("For weight, we only support symmetric quantization.")
                if l.quant_mode != "symmetric":
                    raise ValueError("unknown quant mode: {}".format(l.quant_mode))
                if bool(l.quantize_activation) != self._qact:
                    raise ValueError(f"MLPStack: layer {i}'s quantize_activation changed since the stack was built")
                if l.bias_bit is None:
                    raise TypeError("QuantLinear quantizes its bias: bias_bit must be an int")
            a = getattr(l, "activation", None)
            if not (a is None or isinstance(a, str)) or a not in _ACTS:
                raise ValueError(f"QuantLinear.activation must be None, 'relu' or 'sigmoid' (got {a!r})")
            if l.weight.device != dev:
                raise ValueError(f"MLPStack needs its layers on one device (layer {i} on {l.weight.device}, "
                                 f"layer 0 on {dev})")
            lin[i] = l._c_struct()  # a copy; the layer checks dtype, device and contiguity
            quantized[i], act[i] = int(q), _ACTS[a]
        c = L.MLP()
        c.num_layers = n
        c.layers, c.quantized, c.act = lin, quantized, act
        self._c = (key, c, (lin, quantized, act))
        return c

    def _prepare(self, x=None):
        """QuantLinear.forward's checks for the whole stack; sizes the scale buffers."""
        dev = self.layers[0].weight.device
        if x is not None:
            _check_input(x, self.layers[0])
        elif dev.type != "cuda":
            raise L.DQRMError(f"MLPStack runs on libdqrm's HIP kernels: the layers must be on a GPU (got {dev}); "
                              "there is no CPU path")
        for l in self.layers:
            if l.weight.device.type != "cuda":
                raise L.DQRMError(f"MLPStack runs on libdqrm's HIP kernels: the layers must be on a GPU (got "
                                  f"{l.weight.device}); there is no CPU path")
            if not l.full_precision_flag:
                l._scale_buffer()
        return dev

    # ------------------------------------------------------------ forward
    def is_fresh(self, key=None) -> bool:
        """Whether the next forward will skip the weight quantization (key: ``_key()``, from a
        caller that has just computed it)."""
        return self._fresh is not None and self._fresh == self._state(key)

    def __call__(self, x, prev_act_scaling_factor=None):
        """``y``; for a quantize_activation stack ``(y, out_scale)``, the last layer's
        correct_output_scale, from ``prev_act_scaling_factor``, the one-element scale of the
        QuantAct in front of the stack."""
        self._prepare(x)
        prev = prev_act_scaling_factor
        if not self._qact:
            if prev is not None:
                raise NotImplementedError("a prev_act_scaling_factor on a stack without quantize_activation=True "
                                          "layers is not built (the reference's drivers never pass one)")
        else:
            if prev is None:
                raise MissingActScale("MLPStack: a quantize_activation stack needs a prev_act_scaling_factor "
                                      "(QuantAct's act_scaling_factor)")
            if not isinstance(prev, torch.Tensor) or prev.numel() != 1:
                got = tuple(prev.shape) if isinstance(prev, torch.Tensor) else type(prev).__name__
                raise ValueError(f"prev_act_scaling_factor must be a tensor of ONE element (got {got})")
            if prev.dtype != torch.float32 or prev.device != x.device:
                raise ValueError(f"prev_act_scaling_factor must be float32 on the input's device (got {prev.dtype} "
                                 f"on {prev.device})")
            self._check_qact()
        return _on_device(x.device, self._run, x, prev)

    def _run(self, x, prev=None):
        key = self._key()
        c = self._c_struct(key)  # raises on an unsupported layer before autograd is involved
        fresh = self.is_fresh(key)
        if not fresh:
            self._fresh = None
        ws = [l.weight for l in self.layers]
        bs = [l.bias for l in self.layers]
        if not self._qact:
            return _StackFn.apply(x, self, c, fresh, *ws, *bs)
        # [1, O] / [1, 1] as QuantLinear leaves them; fresh per forward, so the scales an earlier
        # forward saved for its backward are never overwritten
        scales = [torch.empty((1, l.out_features if l.per_channel else 1), dtype=torch.float32, device=x.device)
                  for l in self.layers]
        y = _StackQActFn.apply(x, self, c, fresh, prev.detach(), scales, *ws, *bs)
        for l, s in zip(self.layers, scales):
            l._buffers["correct_output_scale"] = s
        return y, scales[-1]

    # ------------------------------------------------------------ the update
    def sgd_step(self, lr, requantize=True, grad_scales=None):
        """``p += -lr * p.grad`` on every weight and bias in one dqrm_mlp_sgd (two launches when a
        quantized layer is per tensor and requantize is set). requantize: also refresh the layers'
        integers and scales, after which the stack is fresh. grad_scales: per layer an
        ``[out_features + 1]`` float32 tensor (the rows' scales, then the bias's) for the DP form
        ``p += (-lr * p.grad) * s``. Gradients are left in place: zeroing is the loop's business."""
        dev = self._prepare()
        n = len(self.layers)
        for i, l in enumerate(self.layers):
            for name, p in (("weight", l.weight), ("bias", l.bias)):
                g = p.grad
                if g is None:
                    raise ValueError(f"MLPStack.sgd_step: layer {i}'s {name}.grad is None")
                if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.shape != p.shape:
                    raise ValueError(f"MLPStack.sgd_step: layer {i}'s {name}.grad must be a contiguous float32 "
                                     f"tensor of the parameter's shape on {p.device} (got {g.dtype} "
                                     f"{tuple(g.shape)} on {g.device}, contiguous={g.is_contiguous()})")
        gs = None
        if grad_scales is not None:
            grad_scales = list(grad_scales)
            if len(grad_scales) != n:
                raise ValueError(f"grad_scales needs one tensor per layer ({n}), got {len(grad_scales)}")
            for i, (s, l) in enumerate(zip(grad_scales, self.layers)):
                if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or s.device != l.weight.device \
                        or s.numel() != l.out_features + 1 or not s.is_contiguous():
                    raise ValueError(f"grad_scales[{i}] must be a contiguous float32 tensor of "
                                     f"{l.out_features + 1} elements on {l.weight.device}")
            gs = self._PtrArray(*[s.data_ptr() for s in grad_scales])
        _on_device(dev, self._sgd, float(lr), bool(requantize), gs)

    def _sgd(self, lr, requantize, gs):
        key = self._key()
        c = self._c_struct(key)
        ws, need = self._workspace, 0
        if requantize:
            need = self._lib.dqrm_mlp_sgd_workspace_bytes(C.byref(c))
            if need and (ws is None or ws.numel() * 4 < need or ws.device != self.layers[0].weight.device):
                ws = self._workspace = torch.empty(need // 4, dtype=torch.float32, device=self.layers[0].weight.device)
        A = self._PtrArray
        self._fresh = None
        L.check(self._lib.dqrm_mlp_sgd(C.byref(c), L.DQRM_MLP_REQUANT if requantize else 0,
                                       A(*[l.weight.grad.data_ptr() for l in self.layers]),
                                       A(*[l.bias.grad.data_ptr() for l in self.layers]), gs, lr,
                                       ws.data_ptr() if need else None, need, _stream_handle()), "dqrm_mlp_sgd")
        for l in self.layers:  # the kernel wrote them: what autograd saved of them is stale
            torch.autograd.graph.increment_version(l.weight)
            torch.autograd.graph.increment_version(l.bias)
        if requantize:
            self._fresh = self._state(key)

    def requantize(self):
        """Run every quantized layer's dqrm_linear_wquant now and mark the stack fresh: an
        inference loop's forwards then launch no quantization at all."""
        dev = self._prepare()
        _on_device(dev, self._requantize)

    def _requantize(self):
        self._c_struct()
        self._fresh = None
        st = _stream_handle()
        for l in self.layers:
            if not l.full_precision_flag:
                L.check(self._lib.dqrm_linear_wquant(C.byref(l._c_struct()), st), "dqrm_linear_wquant")
        self._fresh = self._state()

    def invalidate(self):
        """Mark the stack not fresh: the next forward quantizes every layer again. Needed only
        after a write torch cannot see (``p.data.add_()``, a kernel of your own on ``data_ptr()``)."""
        self._fresh = None


__all__ = ["FusedActivation", "fuse_activations", "unfuse_activations", "create_mlp", "apply_mlp", "MLPStack"]
