"""INT8-quantized gradient exchange of the dense (MLP) layers of the data-parallel step.

Reference: sgd_quantized_gradients_parallel_comm.py
  quantize_linear_grad   :892-929  per-channel scale = max(|row min|, |row max|)/127,
                                   all_reduce(scale)/N, q = SymmetricQuantFunction(g),
                                   all_reduce(q)/N
  quantize_bias_grad     :931-961  the same, one scale per bias vector
  grad_update_parallel_comm      MLP branch :337-409   (2 layers x 2 tensors x 2 collectives each)
  weight_update_parallel_comm    MLP branch :630-668   W += (-lr * grad) * s

MI355X design: every weight row and every bias vector of all bot_l / top_l layers is one
channel of ONE channel table, so each phase is one libdqrm launch for all layers and the
reference's 4 blocking collectives per layer become two per step:
  1. all-gather of the per-channel local scales s_loc [C] -> every rank averages them in
     the same (descending-rank) order, bit-identical on all ranks;
  2. all-reduce(SUM) of the quantized wire: integer-valued fp16 (exact: N * 128 <= 2048
     for N <= 16; int32 beyond), half the bytes of an FP32 gradient all-reduce.
Kernels: dqrm_dense_grad_scale, dqrm_dense_grad_quant, dqrm_dense_grad_decode,
dqrm_dense_update (csrc/dqrm_dense.hip).

SimulatedDenseBuffers is the MLP half of the simulated-DP buffer of sgd_quantized_gradients.py
(one device plays N ranks; error-compensated INT8 accumulate :96-139, update :381-404) over the
same channel table: dqrm_dense_ec_accumulate and dqrm_dense_sim_update, one launch each.
"""
from __future__ import annotations

import ctypes as C
from typing import Protocol, Sequence

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from . import _lib as L
from .linear import note_raw_write
from .tables import _ptr, _stream_handle

_WIRE_DTYPE = {L.DQRM_WIRE_F16: torch.float16, L.DQRM_WIRE_I32: torch.int32, L.DQRM_WIRE_F32: torch.float32}


class DenseChannels:
    """The channel table of a list of Linear layers: layer k contributes its weight rows
    (one channel each, per_channel=True) then its bias vector (one channel).
    weight_slices[k] / bias_index[k] locate layer k's scales in the [C] scale vectors."""

    def __init__(self, layers: Sequence[nn.Module]):
        self.layers = list(layers)
        self.weight_slices: list[slice] = []
        self.bias_index: list[int] = []
        lens, c = [], 0
        for l in self.layers:
            out, inp = l.weight.shape
            if l.bias is None:
                raise ValueError("quantize_bias_grad needs every Linear layer to have a bias (s_q_g_p_c.py:931)")
            self.weight_slices.append(slice(c, c + out))
            lens += [inp] * out
            c += out
            self.bias_index.append(c)
            lens.append(out)
            c += 1
        self.num_channels = c
        self.len = np.asarray(lens, dtype=np.int32)
        self.wire_off = np.zeros(c, dtype=np.int64)
        if c:
            self.wire_off[1:] = np.cumsum(self.len[:-1], dtype=np.int64)
        self.total_elems = int(self.len.sum()) if c else 0
        self.max_len = int(self.len.max()) if c else 0

    def tensors(self):
        """[(grad, param)] per layer tensor, in channel order (weight, bias, weight, ...)."""
        out = []
        for l in self.layers:
            out.append((l.weight.grad, l.weight.data))
            out.append((l.bias.grad, l.bias.data))
        return out


class DenseKernels(Protocol):
    """The four device steps (HIP by default; CPU tests inject an oracle-backed checker).
    prepare() runs once per exchange()/apply() before the steps."""

    def prepare(self) -> None: ...

    def scale(self, bits: int, s_loc: torch.Tensor) -> None: ...

    def quant(self, bits: int, s_all: torch.Tensor, num_ranks: int, s_avg: torch.Tensor, wire_type: int,
              wire: torch.Tensor) -> None: ...

    def decode(self, wire: torch.Tensor, wire_type: int, num_ranks: int) -> None: ...

    def update(self, s: torch.Tensor | None, lr: float) -> None: ...


class HipDenseKernels:
    """libdqrm's dense kernels over a DenseChannels table; the only implementation the
    product uses. The device channel table (grad/param pointers per channel) is rebuilt
    whenever a layer's .grad or .data storage changes."""

    def __init__(self, channels: DenseChannels, device):
        self.ch = channels
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.DQRMError(f"libdqrm's dense kernels need the layers on a GPU (got {self.device}); "
                              "there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = L.load()
        self._key = None
        self._c = L.DenseSet()
        self._bufs: list[torch.Tensor] = []

    def prepare(self) -> None:
        """Rebuild the device channel table if a layer's .grad / .data storage moved."""
        ts = self.ch.tensors()
        key = tuple((g.data_ptr(), p.data_ptr()) for g, p in ts)
        if key == self._key:
            return
        for g, p in ts:
            if g.device != self.device or p.device != self.device:
                raise ValueError(f"dense layers must live on {self.device} (got {g.device} / {p.device})")
            if g.dtype != torch.float32 or p.dtype != torch.float32 or not g.is_contiguous() or not p.is_contiguous():
                raise ValueError("dense layers need contiguous float32 weights and gradients")
        gp, pp = [], []
        for l in self.ch.layers:
            out, inp = l.weight.shape
            g0, p0 = l.weight.grad.data_ptr(), l.weight.data.data_ptr()
            gp += [g0 + 4 * inp * r for r in range(out)]
            pp += [p0 + 4 * inp * r for r in range(out)]
            gp.append(l.bias.grad.data_ptr())
            pp.append(l.bias.data.data_ptr())
        host = [np.asarray(gp, np.uint64).view(np.int64), np.asarray(pp, np.uint64).view(np.int64),
                self.ch.len, self.ch.wire_off]
        self._bufs = [torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in host]
        c = self._c
        c.num_channels = self.ch.num_channels
        c.max_len = self.ch.max_len
        c.total_elems = self.ch.total_elems
        c.grad, c.param, c.len, c.wire_off = (_ptr(b) for b in self._bufs)
        self._key = key

    def scale(self, bits, s_loc):
        L.check(self.lib.dqrm_dense_grad_scale(C.byref(self._c), bits, _ptr(s_loc), _stream_handle()),
                "dqrm_dense_grad_scale")

    def quant(self, bits, s_all, num_ranks, s_avg, wire_type, wire):
        L.check(self.lib.dqrm_dense_grad_quant(C.byref(self._c), bits, _ptr(s_all), num_ranks, _ptr(s_avg),
                                               wire_type, _ptr(wire), _stream_handle()),
                "dqrm_dense_grad_quant")

    def decode(self, wire, wire_type, num_ranks):
        L.check(self.lib.dqrm_dense_grad_decode(C.byref(self._c), _ptr(wire), wire_type, num_ranks,
                                                _stream_handle()),
                "dqrm_dense_grad_decode")

    def update(self, s, lr):
        note_raw_write()  # the parameters change behind torch's version counters
        L.check(self.lib.dqrm_dense_update(C.byref(self._c), _ptr(s), float(lr), _stream_handle()),
                "dqrm_dense_update")

    def ec_accumulate(self, bits, scale, err, buf):
        L.check(self.lib.dqrm_dense_ec_accumulate(C.byref(self._c), bits, _ptr(scale), _ptr(err), _ptr(buf),
                                                  _stream_handle()),
                "dqrm_dense_ec_accumulate")

    def sim_update(self, scale, buf, num_gpus, lr):
        L.check(self.lib.dqrm_dense_sim_update(C.byref(self._c), _ptr(scale), _ptr(buf), int(num_gpus), float(lr),
                                               _stream_handle()),
                "dqrm_dense_sim_update")


class DenseGradExchange:
    """The MLP half of grad_update_parallel_comm / weight_update_parallel_comm for all
    bot_l + top_l Linear layers. One instance per rank; buffers reused every step.

    grad_bits: 8 (the reference hard-codes num_bits=8 for the MLP, s_q_g_p_c.py:341,350),
    2..16, or 32 for mlp_layer_quantized=False (FP32 all-reduce / N, :358-369).
    """

    def __init__(self, layers: Sequence[nn.Module], grad_bits: int = 8, group=None,
                 kernels: DenseKernels | None = None, device=None, wire_type: int | None = None,
                 force_collectives: bool = False):
        """force_collectives: issue the scale all-gather and the wire all-reduce at world
        size 1 too, through the process group's backend (the N > 1 code path)."""
        if not (grad_bits == 32 or 2 <= grad_bits <= 16):
            raise ValueError("grad_bits must be 2..16 or 32")
        self.channels = DenseChannels(layers)
        self.grad_bits = grad_bits
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        self.coll = self.world > 1 or bool(force_collectives)
        if self.coll and not (dist.is_available() and dist.is_initialized()):
            raise ValueError("force_collectives needs an initialised process group")
        if device is None:
            device = self.channels.layers[0].weight.device if self.channels.layers else "cpu"
        self.device = torch.device(device)
        self.kernels = kernels if kernels is not None else HipDenseKernels(self.channels, self.device)
        if wire_type is None:
            wire_type = L.load().dqrm_dense_wire_type(grad_bits, self.world) if kernels is None else \
                _wire_type(grad_bits, self.world)
        if wire_type < 0:
            raise ValueError(f"no exact wire type for {grad_bits} bits over {self.world} ranks")
        self.wire_type = wire_type
        C_ = self.channels.num_channels
        self.s_loc = torch.zeros(C_, dtype=torch.float32, device=self.device)
        self.s_all = torch.zeros(self.world, C_, dtype=torch.float32, device=self.device)
        self.s_avg = torch.zeros(C_, dtype=torch.float32, device=self.device)
        self.wire = torch.zeros(self.channels.total_elems, dtype=_WIRE_DTYPE[wire_type], device=self.device)

    # -------------------------------------------------------------- collectives
    def _backend(self) -> str:
        return dist.get_backend(self.group)

    def _all_gather_scales(self) -> None:
        if self._backend() == "nccl":
            dist.all_gather_into_tensor(self.s_all.view(-1), self.s_loc, group=self.group)
        elif self.s_all.is_cuda:  # Gloo gathers host tensors (rehearsal only)
            host = self.s_all.cpu()
            dist.all_gather(list(host.unbind(0)), self.s_loc.cpu(), group=self.group)
            self.s_all.copy_(host)
        else:
            dist.all_gather(list(self.s_all.unbind(0)), self.s_loc, group=self.group)

    def _all_reduce_wire(self) -> None:
        if self._backend() == "nccl" or not self.wire.is_cuda:
            dist.all_reduce(self.wire, dist.ReduceOp.SUM, group=self.group)
        else:
            host = self.wire.cpu()
            dist.all_reduce(host, dist.ReduceOp.SUM, group=self.group)
            self.wire.copy_(host)

    # -------------------------------------------------------------- the step
    def exchange(self) -> None:
        """grad_update_parallel_comm's MLP branch: afterwards every layer's .grad holds the
        rank-averaged quantized gradient and weight_scaling_factor / bias_scaling_factor
        the averaged scales (views into this exchange's s_avg)."""
        k, gb = self.kernels, self.grad_bits
        k.prepare()
        if gb != 32:
            k.scale(gb, self.s_loc)
            if self.coll:
                self._all_gather_scales()
                s_all = self.s_all
            else:
                s_all = self.s_loc.view(1, -1)
        else:
            s_all = None
        k.quant(gb, s_all, self.world, self.s_avg if gb != 32 else None, self.wire_type, self.wire)
        if self.coll:
            self._all_reduce_wire()
        k.decode(self.wire, self.wire_type, self.world)
        if gb != 32:
            for l, ws, bi in zip(self.channels.layers, self.channels.weight_slices, self.channels.bias_index):
                l.weight_scaling_factor = self.s_avg[ws]
                l.bias_scaling_factor = self.s_avg[bi]

    def apply(self, lr: float) -> None:
        """weight_update_parallel_comm's MLP branch: W += (-lr * grad) * s."""
        self.kernels.prepare()
        self.kernels.update(self.s_avg if self.grad_bits != 32 else None, lr)


class SimulatedDenseKernels(Protocol):
    """The two device steps of SimulatedDenseBuffers (HipDenseKernels by default; CPU tests
    inject a numpy restatement). prepare() runs before each."""

    def prepare(self) -> None: ...

    def ec_accumulate(self, bits: int, scale: torch.Tensor, err: torch.Tensor, buf: torch.Tensor) -> None: ...

    def sim_update(self, scale: torch.Tensor, buf: torch.Tensor, num_gpus: int, lr: float) -> None: ...


class SimulatedDenseBuffers:
    """The MLP half of the simulated-DP buffer (sgd_quantized_gradients.py: one device plays N
    ranks) for all bot_l + top_l QuantLinear layers, with the reference's error compensation
    (quantize_linear_grad / quantize_bias_grad, err_compensation=True, per channel, :563-632):

      accumulate()           one micro-step (:96-139): v = grad + e; a channel whose scale is 0 takes
                             s = clamp(max|v|, 1e-8) / qmax; q = quantize(v, s); buf += q; e = v - q * s
      update(lr, num_gpus)   (:381-404) param += -lr * (buf * (s / num_gpus))
      zero()                 (:261-308) buf = 0, s = 0; e carries into the next window

    One libdqrm launch each for accumulate (dqrm_dense_ec_accumulate) and update
    (dqrm_dense_sim_update). The state is scale [C], err and buf [total_elems] over the
    DenseChannels table; every layer's weight_scaling_factor, bias_scaling_factor,
    error_compensation_weight and error_compensation_bias (its registered buffers, names
    unchanged) and weight_grad_buffer / bias_grad_buffer (plain attributes) are views of them, so
    they hold the live values after every call. A layer's error compensation at construction is
    taken over. grad_bits: 8 (the reference hard-codes num_bits=8, :104-136), 2..16."""

    def __init__(self, layers: Sequence[nn.Module], grad_bits: int = 8,
                 kernels: SimulatedDenseKernels | None = None, device=None):
        if isinstance(grad_bits, bool) or not 2 <= int(grad_bits) <= 16:
            raise ValueError("grad_bits must be 2..16")
        self.channels = ch = DenseChannels(layers)
        self.grad_bits = int(grad_bits)
        if device is None:
            device = ch.layers[0].weight.device if ch.layers else "cpu"
        self.device = torch.device(device)
        self.kernels = kernels if kernels is not None else HipDenseKernels(ch, self.device)
        self.scale = torch.zeros(ch.num_channels, dtype=torch.float32, device=self.device)
        self.err = torch.zeros(ch.total_elems, dtype=torch.float32, device=self.device)
        self.buf = torch.zeros(ch.total_elems, dtype=torch.float32, device=self.device)
        self.micro_steps = 0  # accumulate() calls since zero()
        self._views = []
        for l, ws, bi in zip(ch.layers, ch.weight_slices, ch.bias_index):
            w0, b0 = int(ch.wire_off[ws.start]), int(ch.wire_off[bi])
            nw, nb = l.weight.numel(), l.bias.numel()
            ew, eb = self.err[w0: w0 + nw].view(l.weight.shape), self.err[b0: b0 + nb]
            for view, name in ((ew, "error_compensation_weight"), (eb, "error_compensation_bias")):
                old = getattr(l, name, None)
                if isinstance(old, torch.Tensor) and old.shape == view.shape:
                    view.copy_(old)
            self._views.append((self.scale[ws], self.scale[bi], ew, eb,
                                self.buf[w0: w0 + nw].view(l.weight.shape), self.buf[b0: b0 + nb]))
        self._bind()

    _NAMES = ("weight_scaling_factor", "bias_scaling_factor", "error_compensation_weight",
              "error_compensation_bias", "weight_grad_buffer", "bias_grad_buffer")

    def _bind(self) -> None:
        """Point the layers' attributes at the state (again, if something replaced one)."""
        for l, views in zip(self.channels.layers, self._views):
            bufs, plain = l._buffers, l.__dict__  # dict reads: nn.Module.__getattr__ costs per call
            for name, v in zip(self._NAMES, views):
                if (bufs[name] if name in bufs else plain.get(name)) is not v:
                    setattr(l, name, v)

    def accumulate(self) -> None:
        for l in self.channels.layers:
            if l.weight.grad is None or l.bias.grad is None:
                raise ValueError("simulated DP: every QuantLinear of bot_l / top_l needs its weight and bias "
                                 "gradient at a micro-step (call it after backward())")
        self.kernels.prepare()
        self.kernels.ec_accumulate(self.grad_bits, self.scale, self.err, self.buf)
        self.micro_steps += 1
        self._bind()

    def update(self, lr: float, num_gpus: int) -> None:
        if int(num_gpus) < 1:
            raise ValueError("num_gpus must be >= 1")
        self.kernels.prepare()
        note_raw_write()  # the parameters change behind torch's version counters
        self.kernels.sim_update(self.scale, self.buf, int(num_gpus), float(lr))
        for l in self.channels.layers:  # what autograd saved of them is stale
            torch.autograd.graph.increment_version(l.weight)
            torch.autograd.graph.increment_version(l.bias)
        self._bind()

    def zero(self) -> None:
        self.buf.zero_()
        self.scale.zero_()
        self.micro_steps = 0
        self._bind()


def _wire_type(bits: int, num_ranks: int) -> int:
    """dqrm_dense_wire_type, for host-only (injected-kernel) runs."""
    if bits == 32:
        return L.DQRM_WIRE_F32
    if not 2 <= bits <= 16 or num_ranks < 1:
        return L.DQRM_E_INVALID
    return L.DQRM_WIRE_F16 if num_ranks << (bits - 1) <= 2048 else L.DQRM_WIRE_I32


__all__ = ["DenseChannels", "DenseKernels", "HipDenseKernels", "DenseGradExchange", "SimulatedDenseKernels",
           "SimulatedDenseBuffers"]
