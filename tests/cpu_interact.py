"""CPU restatement of the reference's dot feature interaction, for the DotInteraction tests.

What it restates (in this file's own words, torch ops on the CPU with autograd):
  dlrm_s_pytorch_comm_grad.py:701-806   DLRM_Net.interact_features, arch_interaction_op "dot",
                                        plain and with modify_feature_interaction
  quant_utils.py:196-220                the symmetric scale
  quant_utils.py:75-101, :316-363       round(1/s * x + 0), clamp, and the STE backward
The op sequence (cat, bmm, index, cat) runs in float64 with autograd; the quantization (min, max,
scale, round, clamp) runs as the reference's separately rounded f32 operations and its integers
enter the float64 sequence exactly. Plus the input builders the GPU tests share.
"""
from __future__ import annotations

import numpy as np
import torch

# (B, F, D, itself): one pair and one vector load; the diagonal and its doubling; the two real
# shapes (351 pairs: the last group of 64 lanes is not full); more samples than workgroups of one
# pass on a small device, ragged; the F limit (2016 pairs)
SHAPES = [(1, 2, 4, False), (3, 2, 4, True), (5, 27, 16, False), (7, 27, 64, False), (130, 9, 128, True),
          (67, 64, 8, False)]
# one more than the issue's six, for the kernels' other launch form (csrc/dqrm_interact.hip,
# launch_samples): the largest tile (F = 64, D = 256: 75 KB with the pair gradients) needs the
# kernel's dynamic LDS limit raised past 64 KiB
LDS_SHAPES = [(3, 64, 256, True)]


def pair_lists(F: int, itself: bool):
    """li, lj exactly as interact_features builds them (:720-722)."""
    offset = 1 if itself else 0
    li = [i for i in range(F) for j in range(i + offset)]
    lj = [j for i in range(F) for j in range(i + offset)]
    return li, lj


def num_pairs(F: int, itself: bool) -> int:
    return F * (F - 1) // 2 + (F if itself else 0)


def qmax(bits: int) -> int:
    return 2 ** (bits - 1) - 1


def features(x: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    """T [B, F, D] the way the reference forms it: cat([x] + ly, dim=1).view(B, -1, D)."""
    B, D = x.shape
    ly = [emb[:, t] for t in range(emb.shape[1])]
    return torch.cat([x] + ly, dim=1).view(B, -1, D)


# ---------------------------------------------------------------------------------- f32 quantization
def feature_scale(T32: torch.Tensor, bits: int) -> torch.Tensor:
    """symmetric_linear_quantization_params(bits, T.min(), T.max(), False), f32, shape [1]."""
    assert T32.dtype == torch.float32
    n = qmax(bits)
    with torch.no_grad():
        lo, hi = T32.min(), T32.max()
        s = torch.maximum(lo.abs(), hi.abs())
        return (torch.clamp(s, min=1e-8) / n).view(1)


def feature_integers(T32: torch.Tensor, s32: torch.Tensor, bits: int) -> torch.Tensor:
    """SymmetricQuantFunction's forward in f32: clamp(round(1/s * T + 0), -n-1, n)."""
    assert T32.dtype == torch.float32 and s32.dtype == torch.float32
    n = qmax(bits)
    q = torch.round(1.0 / s32.view(()) * T32 + torch.tensor(0.0))
    return torch.clamp(q, -n - 1, n)


class _SymQuant64(torch.autograd.Function):
    """The f32 integers of T inside a float64 graph; the incoming gradient divided by s backward."""

    @staticmethod
    def forward(ctx, T64, T32, bits, s32):
        ctx.s = s32.double().view(())
        return feature_integers(T32, s32, bits).double()

    @staticmethod
    def backward(ctx, grad):
        return grad / ctx.s, None, None, None


# ---------------------------------------------------------------------------------- the op sequence
def forward_backward(x, emb, dr, itself: bool, bits: int | None):
    """(R, dx, demb, s) of the reference's op sequence evaluated in float64 with autograd, for f32
    inputs x [B, D], emb [B, T, D] and the output gradient dr [B, D + P]. s: the f32 scale
    ([1]; None in plain mode)."""
    x64 = x.double().requires_grad_(True)
    e64 = emb.double().requires_grad_(True)
    T = features(x64, e64)
    F = T.shape[1]
    s = None
    if bits:
        T32 = features(x, emb)
        s = feature_scale(T32, bits)
        Ti = _SymQuant64.apply(T, T32, bits, s)
        Z = torch.bmm(Ti, torch.transpose(Ti, 1, 2)) * (s.double().view(()) ** 2)
    else:
        Z = torch.bmm(T, torch.transpose(T, 1, 2))
    li, lj = pair_lists(F, itself)
    Zflat = Z[:, torch.tensor(li), torch.tensor(lj)]
    R = torch.cat([x64] + [Zflat], dim=1)
    R.backward(dr.double())
    return R.detach(), x64.grad, e64.grad, s


def coefficient_matrix(dr, F: int, D: int, itself: bool) -> torch.Tensor:
    """|c(i, j)| of the backward as a [B, F, F] float64 matrix (for the error bounds): |g| placed
    at (i, j) and (j, i), twice |g| on the diagonal."""
    li, lj = pair_lists(F, itself)
    g = dr[:, D:].double().abs()
    C = torch.zeros(dr.shape[0], F, F, dtype=torch.float64)
    C[:, torch.tensor(li), torch.tensor(lj)] = g
    return C + C.transpose(1, 2)


# ---------------------------------------------------------------------------------- inputs
def random_case(B, F, D, itself, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, D)).astype(np.float32)
    emb = rs.standard_normal((B, F - 1, D)).astype(np.float32)
    dr = rs.standard_normal((B, D + num_pairs(F, itself))).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, emb, dr))


def exact_case(B, F, D, itself, bits, seed):
    """Inputs on which every product and partial sum of the forward and the backward is exact in
    f32, in any order. dr: eighths in [-1, 1].
      plain: x, emb quarter-integers in [-4, 4] (D <= 128, F <= 64: numerators below 2^24);
      bits 8: T = m / 64, integer m in [-127, 127] with a +-127 present: s = 1/64 and 1/s = 64
              exactly, so the integers are m;
      bits 16: one +-32767 entry, every other |m| <= 8 (D <= 16, no self-interaction: 32767^2 is
              not representable), s = 1/64 again.
    Random integers: no value pattern survives a transpose of the pair order or a swap of features."""
    rs = np.random.RandomState(seed)
    P = num_pairs(F, itself)
    dr = (rs.randint(-8, 9, (B, D + P)) / 8.0).astype(np.float32)
    if not bits:
        T = rs.randint(-16, 17, (B, F, D)) / 4.0
    else:
        assert bits in (8, 16)
        if bits == 16:
            assert D <= 16 and not itself
        small = 127 if bits == 8 else 8
        m = rs.randint(-small, small + 1, (B, F, D))
        b, f, k = rs.randint(0, B), rs.randint(0, F), rs.randint(0, D)
        m[b, f, k] = qmax(bits) if rs.randint(0, 2) else -qmax(bits)
        T = m / 64.0
    T = T.astype(np.float32)
    x, emb = np.ascontiguousarray(T[:, 0]), np.ascontiguousarray(T[:, 1:])
    return tuple(torch.from_numpy(a) for a in (x, emb, dr))


def gamma(m: int) -> float:
    """The standard bound factor of an m-operation f32 chain, u = 2^-24."""
    u = 2.0 ** -24
    return m * u / (1.0 - m * u)
