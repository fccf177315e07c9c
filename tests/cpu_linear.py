"""CPU restatement of the reference's QuantLinear arithmetic, for the QuantLinear tests.

What it restates (in this file's own words, torch ops on the CPU with autograd):
  quant_modules_not_quantize_grad.py:105-211   QuantLinear.forward (weight-only branch)
  quant_utils.py:196-220                       the symmetric scale
  quant_utils.py:75-101, :316-363              round(1/s * x + 0), clamp, and the STE backward
plus the input builders the GPU tests share.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import gen_inputs as G

SHAPES = [(7, 13, 5), (64, 415, 1), (33, 512, 256), (130, 70, 66)]  # (B, in, out)
# one more than the issue's four: large enough that all three products take the 64 x 64 tile
# (>= 1024 tiles of 32 x 32), ragged in every dimension
BIG_SHAPE = (1040, 1030, 1050)


def qmax(bits: int) -> int:
    return 2 ** (bits - 1) - 1


def _per_row(scale: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """The scale laid out against `like`: one per row of a matrix (a one-element scale
    broadcasts), elementwise against a vector."""
    if like.dim() == 2 and scale.numel() != 1:
        return scale.view(-1, 1)
    return scale.view(-1)


class SymQuant(torch.autograd.Function):
    """clamp(round(1/s * v + 0), -n-1, n) forward; the incoming gradient divided by s backward."""

    @staticmethod
    def forward(ctx, v, bits, scale):
        n = qmax(bits)
        ctx.scale = scale
        q = torch.round(1.0 / _per_row(scale, v) * v + torch.tensor(0.0))
        return torch.clamp(q, -n - 1, n)

    @staticmethod
    def backward(ctx, grad):
        s = ctx.scale
        s = s.view(-1, 1) if grad.dim() == 2 else s.view(-1)
        return grad / s, None, None


def weight_scale(W: torch.Tensor, bits: int, per_channel: bool) -> torch.Tensor:
    n = qmax(bits)
    with torch.no_grad():
        if per_channel:
            lo, hi = W.min(dim=1).values, W.max(dim=1).values
            s = torch.maximum(lo.abs(), hi.abs())
        else:
            s = torch.maximum(W.min().abs(), W.max().abs()).expand(1)
        return torch.clamp(s, min=1e-8) / n


def quantize(W, b, bits, per_channel):
    """(scale, weight_integer, bias_integer) as QuantLinear.forward leaves them."""
    s = weight_scale(W, bits, per_channel)
    return s, SymQuant.apply(W, bits, s), SymQuant.apply(b, bits, s)


def forward(x, W, b, bits, per_channel, full_precision=False):
    if full_precision:
        return F.linear(x, W, b)
    s, wi, bi = quantize(W, b, bits, per_channel)
    return F.linear(x, wi, bi) * s.view(1, -1)


def forward_backward(x, W, b, dy, bits, per_channel, full_precision=False):
    """y and the autograd gradients (x.grad, W.grad, b.grad) of sum(y * dy)."""
    x = x.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    y = forward(x, W, b, bits, per_channel, full_precision)
    y.backward(dy)
    return y.detach(), x.grad, W.grad, b.grad


# ---------------------------------------------------------------------------------- inputs
def random_case(B, K, O, seed):
    """gen_inputs.mlp_params weights with one all-zero row (the 1e-8 clamp) and biases that
    saturate the clamp; normal x and dy."""
    W, b = G.mlp_params([(O, K)], seed)[0]
    W, b = W.copy(), b.copy()
    W[O // 2] = 0.0
    b[::3] *= 3.0
    rs = np.random.RandomState(seed + 1)
    x = rs.standard_normal((B, K)).astype(np.float32)
    dy = rs.standard_normal((B, O)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (W, b, x, dy))


def exact_case(B, K, O, bits, per_channel, seed):
    """Inputs on which every product and partial sum of the forward and the backward is exact in
    f32, in any summation order: W = Wi * 2^-k_row with integer Wi in [-n, n] reaching +-n in
    every row (so s = 2^-k_row exactly), biases integer multiples of 2^-k_row reaching a little
    past +-n, x quarter-integers in [-4, 4], dy eighths in [-1, 1]. The generator is asymmetric
    (no value pattern survives a transpose or a row / column swap)."""
    rs = np.random.RandomState(seed)
    n = qmax(bits)
    Wi = rs.randint(-n, n + 1, (O, K)).astype(np.float64)
    Wi[np.arange(O), rs.randint(0, K, O)] = np.where(rs.randint(0, 2, O) == 1, n, -n)
    k = rs.randint(1, 5, (O, 1)) if per_channel else np.full((O, 1), 3)
    W = (Wi * 2.0 ** -k).astype(np.float32)
    b = (rs.randint(-n - 3, n + 4, O) * 2.0 ** -k[:, 0]).astype(np.float32)
    x = (rs.randint(-16, 17, (B, K)) / 4.0).astype(np.float32)
    dy = (rs.randint(-8, 9, (B, O)) / 8.0).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (W, b, x, dy))


def gamma(m: int) -> float:
    """The standard bound factor of an m-operation f32 chain, u = 2^-24."""
    u = 2.0 ** -24
    return m * u / (1.0 - m * u)
