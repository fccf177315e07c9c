"""DLRM's "dot" feature interaction (``DLRM_Net.interact_features``,
dlrm_s_pytorch_comm_grad.py:701-806) on libdqrm's fused kernels (csrc/dqrm_interact.hip; no CPU
fallback).

The reference composes it from ``torch.cat`` -> ``torch.bmm`` -> a fancy-index gather of the lower
triangle -> ``torch.cat`` and, with ``modify_feature_interaction``, runs the same product on 16-bit
fake-quantized features (``min``, ``max``, the symmetric scale, ``SymmetricQuantFunction``, a
multiply by ``scale ** 2``). Here the forward is one launch and the backward one launch (the
quantized forward is preceded by the scale's memset + launch); the embedding outputs are read in
place from a ``[B, T, D]`` tensor of any outer strides, which is what
``QuantEmbeddingBagCollection(..., layout="btd")`` returns (and what ``.transpose(0, 1)`` of its
``"tbd"`` output is).

Every sum is an f32 fmaf chain in ascending index (include/dqrm.h), so in plain mode a sample's
output and gradients do not depend on the batch it is part of. In quantized mode the scale is the
batch's, as in the reference.

    inter = DotInteraction(arch_interaction_itself=False)           # plain
    inter = DotInteraction(quantize_bits=16)                         # modify_feature_interaction
    R = inter(x, ly)                                                 # [B, D + P]
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from .tables import _stream_handle


def out_features(num_features: int, dim: int, arch_interaction_itself: bool = False) -> int:
    """D + P of ``num_features`` vectors of ``dim`` (ValueError outside libdqrm's limits)."""
    n = L.load().dqrm_interact_out_features(int(num_features), int(dim), int(bool(arch_interaction_itself)))
    if n < 0:
        raise ValueError(L.load().dqrm_last_error().decode(errors="replace"))
    return n


def _aligned(t: torch.Tensor) -> bool:
    return t.data_ptr() % 16 == 0


def _slab(ly) -> torch.Tensor:
    """``ly`` as one [B, T, D] tensor: a list / tuple of T [B, D] tensors is stacked (autograd
    routes the slab's gradient back to the pieces), a tensor is taken as it is."""
    if isinstance(ly, (list, tuple)):
        if len(ly) == 0:
            raise ValueError("DotInteraction needs at least one embedding output")
        return torch.stack(list(ly), dim=1)
    return ly


def _check(x: torch.Tensor, emb: torch.Tensor) -> None:
    if not isinstance(x, torch.Tensor) or not isinstance(emb, torch.Tensor):
        raise ValueError("DotInteraction takes x [B, D] and ly, a [B, T, D] tensor or a list of [B, D] tensors")
    if x.dtype != torch.float32 or emb.dtype != torch.float32:
        raise ValueError(f"DotInteraction needs float32 inputs (got {x.dtype} / {emb.dtype})")
    if x.dim() != 2 or emb.dim() != 3 or emb.shape[0] != x.shape[0] or emb.shape[2] != x.shape[1]:
        raise ValueError(f"DotInteraction needs x [B, D] and ly [B, T, D] (got {tuple(x.shape)} / {tuple(emb.shape)})")
    D, T = x.shape[1], emb.shape[1]
    if D % 4 != 0 or not 4 <= D <= 256:
        raise ValueError(f"DotInteraction needs D a multiple of 4 in 4..256 (got {D})")
    if not 1 <= T <= 63:
        raise ValueError(f"DotInteraction needs 1..63 embedding outputs (got {T})")
    if x.device.type != "cuda" or emb.device.type != "cuda":
        raise L.DQRMError(f"DotInteraction runs on libdqrm's HIP kernels: x and ly must be on a GPU "
                          f"(got {x.device} / {emb.device}); there is no CPU path")
    if x.device != emb.device:
        raise ValueError(f"x on {x.device} but ly on {emb.device}")


def _in_place(emb: torch.Tensor) -> torch.Tensor:
    """The slab as the kernels read it: inner stride 1, outer strides multiples of 4 elements and
    a 16-byte aligned start; anything else is copied once."""
    if emb.shape[0] == 0:
        return emb.contiguous()
    if emb.stride(2) == 1 and emb.stride(0) % 4 == 0 and emb.stride(1) % 4 == 0 and _aligned(emb):
        return emb
    return emb.contiguous()


def _config(x, emb, itself: bool, bits: int) -> L.Interact:
    c = L.Interact()
    c.num_features, c.dim = emb.shape[1] + 1, x.shape[1]
    c.self_interaction, c.quant_bits = int(itself), bits
    c.emb_stride_b, c.emb_stride_f = emb.stride(0), emb.stride(1)
    return c


class _InteractFn(torch.autograd.Function):
    """Autograd bridge over dqrm_interact_scale / _fwd / _bwd. The backward uses the scale its own
    forward computed."""

    @staticmethod
    def forward(ctx, x, emb, itself, bits, owner):
        lib, st = L.load(), _stream_handle()
        B, D = x.shape
        c = _config(x, emb, itself, bits)
        r = torch.empty((B, out_features(c.num_features, D, itself)), dtype=torch.float32, device=x.device)
        s = None
        if bits:
            s = torch.empty(1, dtype=torch.float32, device=x.device)
            if B == 0:
                s.fill_(1e-8 / (2 ** (bits - 1) - 1))
            L.check(lib.dqrm_interact_scale(C.byref(c), x.data_ptr(), emb.data_ptr(), B, s.data_ptr(), st),
                    "dqrm_interact_scale")
            if owner is not None:
                owner.feature_scaling_factor = s
        L.check(lib.dqrm_interact_fwd(C.byref(c), x.data_ptr(), emb.data_ptr(), B,
                                      None if s is None else s.data_ptr(), r.data_ptr(), st), "dqrm_interact_fwd")
        ctx.save_for_backward(x, emb, s)
        ctx.itself, ctx.bits = itself, bits
        return r

    @staticmethod
    @once_differentiable
    def backward(ctx, dr):
        x, emb, s = ctx.saved_tensors
        want_x, want_e = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_e):
            return None, None, None, None, None
        dr = dr.contiguous()
        if not _aligned(dr):
            dr = dr.clone()
        B, T = x.shape[0], emb.shape[1]
        dx = torch.empty_like(x) if want_x else None
        demb = torch.empty((B, T, x.shape[1]), dtype=torch.float32, device=x.device) if want_e else None
        c = _config(x, emb, ctx.itself, ctx.bits)
        L.check(L.load().dqrm_interact_bwd(C.byref(c), x.data_ptr(), emb.data_ptr(), dr.data_ptr(), B,
                                           None if s is None else s.data_ptr(),
                                           None if dx is None else dx.data_ptr(),
                                           None if demb is None else demb.data_ptr(), _stream_handle()),
                "dqrm_interact_bwd")
        return dx, demb, None, None, None


def _bits(quantize_bits) -> int:
    if quantize_bits is None:
        return 0
    bits = int(quantize_bits)
    if not 2 <= bits <= 16:
        raise ValueError(f"quantize_bits must be None or 2..16 (got {quantize_bits})")
    return bits


def _run(x, ly, itself: bool, bits: int, owner):
    emb = _slab(ly)
    _check(x, emb)
    x = x.contiguous()
    if not _aligned(x):
        x = x.clone()
    emb = _in_place(emb)
    if x.device.index != torch.cuda.current_device():
        with torch.cuda.device(x.device):
            return _InteractFn.apply(x, emb, itself, bits, owner)
    return _InteractFn.apply(x, emb, itself, bits, owner)


class DotInteraction(nn.Module):
    """``R = cat([x, Z[:, li, lj]])`` of ``Z = T @ T^T``, ``T = [x, ly_0, .., ly_{T-1}]`` per sample.

    arch_interaction_itself: keep the diagonal (the reference's flag of the same name).
    quantize_bits: None for the plain product; 2..16 for the reference's
    ``modify_feature_interaction`` form (which hard-codes 16). ``feature_scaling_factor`` then
    holds the last forward's scale, as the reference's attribute of that name does."""

    def __init__(self, arch_interaction_itself=False, quantize_bits=None):
        super().__init__()
        self.arch_interaction_itself = bool(arch_interaction_itself)
        self.quantize_bits = quantize_bits
        self._bits = _bits(quantize_bits)
        self.register_buffer("feature_scaling_factor", torch.zeros(1), persistent=False)

    def extra_repr(self):
        return f"arch_interaction_itself={self.arch_interaction_itself}, quantize_bits={self.quantize_bits}"

    def out_features(self, num_features: int, dim: int) -> int:
        return out_features(num_features, dim, self.arch_interaction_itself)

    def forward(self, x, ly):
        return _run(x, ly, self.arch_interaction_itself, self._bits, self)


def interact_features(x, ly, arch_interaction_itself=False, quantize_bits=None):
    """The reference's method as a function: ``R = interact_features(x, ly)``."""
    return _run(x, ly, bool(arch_interaction_itself), _bits(quantize_bits), None)


__all__ = ["DotInteraction", "interact_features"]
