"""CPU restatement of a QuantLinear layer followed by the MLP's activation (create_mlp,
dlrm_s_pytorch_comm_grad.py:279-343: nn.ReLU after every layer, nn.Sigmoid after the last), for
the fused-activation tests: tests/cpu_linear.py's layer with torch.relu / torch.sigmoid behind it
and autograd's backward, plus the bounds and the exact-data builder of the sigmoid backward.
"""
from __future__ import annotations

import numpy as np
import torch

import cpu_linear as R

NONE, RELU, SIGMOID = 0, 1, 2
_TORCH = {NONE: lambda z: z, RELU: torch.relu, SIGMOID: torch.sigmoid}


def forward_backward(x, W, b, dy, bits, per_channel, act, full_precision=False):
    """z (the layer's output), y = act(z) and the autograd gradients of sum(y * dy)."""
    x = x.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    z = R.forward(x, W, b, bits, per_channel, full_precision)
    y = _TORCH[act](z)
    y.backward(dy)
    return z.detach(), y.detach(), x.grad, W.grad, b.grad


def sigmoid_bound(sig64: torch.Tensor) -> torch.Tensor:
    """|y - sigma(z)| for y = 1.0f / (1.0f + expf(-z)): expf within 1 ulp enters y with weight
    e / (1 + e) <= 1, the add and the correctly rounded divide half an ulp each (2 ulp = 2^-22
    relative), 1.01 for the second-order terms, 2^-126 for a flushed denormal."""
    return 1.01 * 2.0 ** -22 * sig64 + 2.0 ** -126


def sigmoid_d(dy, y):
    """torch's sigmoid_backward order: (dy * (1 - y)) * y, every operation rounded in dy's dtype."""
    return (dy * (1.0 - y)) * y


def relu_d(dy, y):
    return torch.where(y <= 0, torch.zeros_like(dy), dy)


def backward_from_d(d, x, wi, s):
    """dx, dw, db of dqrm_linear_bwd's formulas over g = d * s, in d's dtype. s: [O] or [1]."""
    s = s.to(d.dtype).expand(d.shape[1])
    g = d * s
    return g @ wi.to(d.dtype), (g.T @ x.to(d.dtype)) / s.view(-1, 1), g.sum(0) / s


def sigmoid_exact_case(B, K, O, bits, per_channel, seed):
    """cpu_linear.exact_case with a caller-chosen y from {0, 1/4, 1/2, 3/4, 1}: (1 - y) * y is 0,
    3/16 or 1/4, dy is eighths in [-1, 1], so d = (dy * (1 - y)) * y is an integer multiple of
    2^-7 of magnitude <= 1/4 (32 units), exact in f32. With s = 2^-k (k <= 4), |wi| <= 127 and
    O <= 256 at 8 bits (7 and 1050 at 4 bits), x quarter-integers in [-4, 4] and B <= 1040:
      dx: 32 * 2^3 units of 2^-11 per g, times 127 * 256 terms  = 8.4e6  < 2^24
      dw: 32 units * 16 quarter-units * 1040                       = 5.4e5  < 2^24   (per row: one s)
      db: 32 units * 1040                                          = 3.4e4  < 2^24
    so every product and partial sum is exact in any order."""
    W, b, x, dy = R.exact_case(B, K, O, bits, per_channel, seed)
    rs = np.random.RandomState(seed + 1000)
    y = torch.from_numpy((rs.randint(0, 5, (B, O)) / 4.0).astype(np.float32))
    return W, b, x, dy, y
