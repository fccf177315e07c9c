"""CPU restatement of the reference's activation-quantized path, for the QuantAct tests.

What it restates (in this file's own words, torch ops on the CPU with autograd; the reference
itself cannot run here, its SymmetricQuantFunction calls .cuda()):
  quant_modules_not_quantize_grad.py:625-725   QuantAct.forward: the running range (:653-678),
                                               the scale (:683), the quantization (:694, :722-723)
  quant_modules_not_quantize_grad.py:105-211   QuantLinear.forward, the integer-activation branch
                                               (:150-161 bias scale and x / prev, :193-196 ste_round)
  quant_utils.py:196-220                       the symmetric scale
  quant_utils.py:75-101, :316-363              round(1/s * x + 0), clamp, and the STE backward
  dlrm_s_pytorch_tb_dp_one_parallel_comm.py:550-612, :857-876   apply_mlp with a scale, the stacks
plus the input builders the GPU tests share.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import cpu_linear as R

NONE, RELU, SIGMOID = 0, 1, 2
_TORCH = {NONE: lambda z: z, RELU: torch.relu, SIGMOID: torch.sigmoid}
P_EXACT = 2.0 ** -3  # the previous activation scale of the exact-data cases


# ---------------------------------------------------------------------------------- QuantAct
class ActRef:
    """QuantAct's state and forward. x_min / x_max / scale are [1] tensors, as its buffers."""

    def __init__(self, bits=4, momentum=0.95, running_stat=True):
        self.bits, self.momentum, self.running_stat = bits, momentum, running_stat
        self.x_min, self.x_max, self.scale = torch.zeros(1), torch.zeros(1), torch.zeros(1)

    def fix(self):
        self.running_stat = False

    def unfix(self):
        self.running_stat = True

    def update_range(self, x):
        """:653-678. The first branch ADDS the batch's range to the (equal) bounds: with the zero
        initial state that sets them, and it is taken again whenever the bounds are equal."""
        bmin, bmax = x.detach().min(), x.detach().max()
        m = self.momentum
        if bool(self.x_min == self.x_max):
            self.x_min = self.x_min + bmin
            self.x_max = self.x_max + bmax
        elif m == -1:
            self.x_min = torch.minimum(self.x_min, bmin)
            self.x_max = torch.maximum(self.x_max, bmax)
        else:
            self.x_min = self.x_min * m + bmin * (1 - m)
            self.x_max = self.x_max * m + bmax * (1 - m)

    def forward(self, x):
        """(y, scale); y carries autograd's graph when x requires a gradient."""
        if self.running_stat:
            self.update_range(x)
        n = R.qmax(self.bits)
        with torch.no_grad():
            self.scale = torch.clamp(torch.maximum(self.x_min.abs(), self.x_max.abs()), min=1e-8) / n
        q = R.SymQuant.apply(x, self.bits, self.scale)
        return q * self.scale.view(-1), self.scale


# ---------------------------------------------------------------------------------- the layer
class SteRound(torch.autograd.Function):
    """torch.round forward, the gradient passed through."""

    @staticmethod
    def forward(ctx, v):
        return torch.round(v)

    @staticmethod
    def backward(ctx, grad):
        return grad


def layer_forward(x, W, b, prev, bits, per_channel, act=NONE):
    """The integer-activation QuantLinear.forward followed by the MLP's activation. Returns
    (y, correct_output_scale [1, O] or [1, 1], parts) with parts = (scale, weight_integer,
    bias_integer, pre: the value ste_round rounds, z: the layer's output before the activation)."""
    s = R.weight_scale(W, bits, per_channel)
    wi = R.SymQuant.apply(W, bits, s)
    bias_scale = s.view(1, -1) * prev.view(1, -1)
    bi = R.SymQuant.apply(b, bits, bias_scale)
    x_int = x / prev.view(1, -1)
    cos = bias_scale[0].view(1, -1)
    pre = F.linear(x_int, wi, bi)
    z = SteRound.apply(pre) * cos
    return _TORCH[act](z), cos, (s, wi.detach(), bi.detach(), pre.detach(), z.detach())


def layer_forward_backward(x, W, b, dy, prev, bits, per_channel, act=NONE):
    """y, cos, parts and the autograd gradients (x.grad, W.grad, b.grad) of sum(y * dy)."""
    x = x.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    y, cos, parts = layer_forward(x, W, b, prev, bits, per_channel, act)
    y.backward(dy)
    return y.detach(), cos, parts, (x.grad, W.grad, b.grad)


def backward_from_d(d, x, wi, s, prev):
    """dx, dw, db of dqrm_linear_bwd_qact's formulas over g = d * cos, in d's dtype. s: [O] or [1]."""
    O = d.shape[1]
    s = s.to(d.dtype).expand(O)
    p = prev.to(d.dtype).view(())
    cos = s * p
    g = d * cos
    x_int = x.to(d.dtype) / p
    return (g @ wi.to(d.dtype)) / p, (g.T @ x_int) / s.view(-1, 1), g.sum(0) / cos


def stack_forward(x, params, prev, bits, sigmoid_layer=-1):
    """apply_mlp over per-tensor layers [(W, b), ...]: a Sigmoid after layer sigmoid_layer, a ReLU
    after every other. Returns (y, per layer the x / prev it saw, per layer its output before the
    activation)."""
    seen, zs = [], []
    for i, (W, b) in enumerate(params):
        seen.append((x / prev.view(1, -1)).detach())
        x, prev, parts = layer_forward(x, W, b, prev, bits, False, SIGMOID if i == sigmoid_layer else RELU)
        zs.append(parts[4])
    return x, seen, zs


# ---------------------------------------------------------------------------------- inputs
def act_batches(shape, seed):
    """Four batches for one QuantAct: an all-equal one (zero for an even seed: x_min == x_max stays
    true and the scale takes the 1e-8 clamp; else 0.375), two normal ones of different spread, and
    a wider one for after fix()."""
    rs = np.random.RandomState(seed)
    first = np.full(shape, 0.0 if seed % 2 == 0 else 0.375, dtype=np.float32)
    second = rs.standard_normal(shape).astype(np.float32)
    third = (1.5 * rs.standard_normal(shape) + 0.25).astype(np.float32)
    fourth = (4.0 * rs.standard_normal(shape)).astype(np.float32)
    return [torch.from_numpy(a) for a in (first, second, third, fourth)]


def exact_case(B, K, O, bits, per_channel, seed):
    """cpu_linear.exact_case moved onto a previous activation scale p = 2^-3: x an integer
    multiple of p / 4 (x / p a quarter-integer in [-4, 4], so acc + bias_integer has .25 / .5 /
    .75 fractions), the biases integer multiples of cos = 2^-k_row * p reaching a little past the
    clamp, W = Wi * 2^-k_row reaching +-n in every row, dy eighths in [-1, 1]. Every scale is a
    power of two, so with g = dy * cos (at most 2^6 units of 2^-10 per-channel), |Wi| <= 127 and
    O <= 256 at 8 bits (7 and 1050 at 4 bits), B <= 1040:
      fwd: 16 quarter-units * 127 * 1030 terms                  = 2.1e6  < 2^24
      dx:  2^6 units * 127 * 256                                = 2.1e6  < 2^24
      dw:  8 units of dy * 16 quarter-units * 1040 (one cos per row)    = 1.3e5  < 2^24
    every product and partial sum is exact in f32 in any order, and the divisions by p, s and cos
    are exact. Returns (W, b, x, dy, prev)."""
    W, b, x, dy = R.exact_case(B, K, O, bits, per_channel, seed)
    return W, b * P_EXACT, x * P_EXACT, dy, torch.tensor([P_EXACT])


def random_case(B, K, O, seed):
    """cpu_linear.random_case with a previous activation scale that is no power of two; x is off
    its grid, so the value the layer rounds has any fraction."""
    W, b, x, dy = R.random_case(B, K, O, seed)
    return W, b, x, dy, torch.tensor([0.0123], dtype=torch.float32)


def exact_stack(ln, bits, seed):
    """Per-tensor exact weights for a stack: W = Wi * 2^-3 with integer Wi in [-n, n] reaching +-n,
    biases integer multiples of 2^-6 (the first layer's cos for an input scale 2^-3)."""
    rs = np.random.RandomState(seed)
    n = R.qmax(bits)
    params = []
    for k, o in zip(ln[:-1], ln[1:]):
        Wi = rs.randint(-n, n + 1, (o, k)).astype(np.float64)
        Wi[0, 0], Wi[o - 1, k - 1] = n, -n
        W = (Wi * 2.0 ** -3).astype(np.float32)
        b = (rs.randint(-n - 3, n + 4, o) * 2.0 ** -6).astype(np.float32)
        params.append((torch.from_numpy(W), torch.from_numpy(b)))
    return params


def exact_act_input(B, K, seed):
    """Integer multiples of 2^-3 in [-127, 127] * 2^-3 reaching both ends: an 8-bit QuantAct
    returns them unchanged with the scale 2^-3."""
    rs = np.random.RandomState(seed)
    q = rs.randint(-127, 128, (B, K)).astype(np.float32)
    q[0, 0], q[B - 1, K - 1] = 127, -127
    return torch.from_numpy(q * np.float32(2.0 ** -3))
