"""Golden fixture of the MLP half of the simulated-DP buffer, made with PyTorch (CPU) ops that
restate the reference's call sequence (sgd_quantized_gradients.py @ 2024-10-24):

  grad_buffer_update_added_quantization, MLP branch                 :96-139
      not torch.is_nonzero(torch.sum(layer.weight_scaling_factor, dim=0)):
          buffer_changes, scale = quantize_linear_grad(layer, 8, parallel=False, err_compensation=True)
          layer.weight_scaling_factor = scale
      else: quantize_linear_grad(..., scale=layer.weight_scaling_factor, err_compensation=True)
      layer.weight_grad_buffer.add_(buffer_changes)                 (the bias likewise)
  quantize_linear_grad (per_channel=True by default) / quantize_bias_grad   :563-632
      weight = grad + error_compensation; scale = symmetric_linear_quantization_params(8, min, max)
      (quant_utils.py:196-220); grad_up = SymmetricQuantFunction.apply(weight, 8, scale)
      (quant_utils.py:75-101, 316-346); error_compensation = weight - grad_up * scale
  weights_update_added_quantization, MLP branch                     :381-404
      weight_update = buffer * (scale.view(-1, 1) / num_gpus); weight.data.add_(-lr * weight_update)
  grad_buffer_zeroing                                               :261-308
      buffer.zero_(); scaling_factor.zero_()    (the error compensation is not zeroed)

torch's CPU kernels divide in `scale / num_gpus` (its CUDA kernels multiply by the reciprocal of a
scalar divisor, which differs in the last bit for N = 3, 5, 6, 7): the fixture pins the division.

Inputs come from tests/cpu_simdp.py (seeded); the file holds expected outputs only: e, buf, s
after every micro-step and the parameters after every window, N = 3 and N = 4, two windows each.

Run:  python tests/golden/make_golden_simdp_mlp.py    (writes tests/golden/simdp_mlp.npz)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cpu_simdp as S  # noqa: E402
import gen_inputs as G  # noqa: E402
from make_golden import RefSymmetricQuant  # noqa: E402

torch.set_num_threads(1)
WINDOWS = 2


def sym_params(num_bits, smin, smax, per_channel=False):  # quant_utils.py:196-220
    n = 2 ** (num_bits - 1) - 1
    if per_channel:
        scale, _ = torch.max(torch.stack([smin.abs(), smax.abs()], dim=1), dim=1)
        return torch.clamp(scale, min=1e-8) / n
    scale = max(smin.abs(), smax.abs())
    return torch.clamp(scale, min=1e-8) / n


class Layer:
    """The attributes of a QuantLinear the three hooks touch."""

    def __init__(self, W, b):
        self.weight = torch.nn.Parameter(torch.from_numpy(W.copy()))
        self.bias = torch.nn.Parameter(torch.from_numpy(b.copy()))
        o = W.shape[0]
        self.weight_scaling_factor = torch.zeros(o)
        self.bias_scaling_factor = torch.zeros(o)
        self.error_compensation_weight = torch.zeros_like(self.weight)
        self.error_compensation_bias = torch.zeros_like(self.bias)
        self.weight_grad_buffer = torch.zeros_like(self.weight)
        self.bias_grad_buffer = torch.zeros_like(self.bias)


def quantize_linear_grad(layer, num_bits, scale=None):  # :563-600, parallel=False, err_compensation=True
    with torch.no_grad():
        weight = layer.weight.grad + layer.error_compensation_weight
        if scale is None:
            w_min, _ = torch.min(weight, dim=1, out=None)
            w_max, _ = torch.max(weight, dim=1, out=None)
            fc_scaling_factor = sym_params(num_bits, w_min, w_max, True)
        else:
            fc_scaling_factor = scale
        grad_up = RefSymmetricQuant.apply(weight, num_bits, fc_scaling_factor)
        layer.error_compensation_weight = weight - (grad_up * fc_scaling_factor.view(-1, 1))
        return grad_up, fc_scaling_factor


def quantize_bias_grad(layer, num_bits, scale=None):  # :602-632
    with torch.no_grad():
        bias = layer.bias.grad + layer.error_compensation_bias
        if scale is None:
            bias_min, _ = torch.min(bias, dim=0, out=None)
            bias_max, _ = torch.max(bias, dim=0, out=None)
            scale = sym_params(num_bits, bias_min, bias_max)
        grad_update = RefSymmetricQuant.apply(bias, num_bits, scale)
        layer.error_compensation_bias = bias - (grad_update * scale)
        return grad_update, scale


def grad_buffer_update(layers):  # :96-139
    with torch.no_grad():
        for l in layers:
            if not torch.is_nonzero(torch.sum(l.weight_scaling_factor, dim=0)):
                buffer_changes, scale = quantize_linear_grad(l, 8)
                l.weight_scaling_factor = scale
            else:
                buffer_changes, _ = quantize_linear_grad(l, 8, scale=l.weight_scaling_factor)
            l.weight_grad_buffer.add_(buffer_changes)
            if not torch.is_nonzero(torch.sum(l.bias_scaling_factor, dim=0)):
                buffer_changes, scale = quantize_bias_grad(l, 8)
                l.bias_scaling_factor = scale
            else:
                buffer_changes, _ = quantize_bias_grad(l, 8, scale=l.bias_scaling_factor)
            l.bias_grad_buffer.add_(buffer_changes)


def weights_update(layers, lr, num_gpus):  # :381-404
    with torch.no_grad():
        for l in layers:
            weight_update = l.weight_grad_buffer * (l.weight_scaling_factor.view(-1, 1) / num_gpus)
            l.weight.data.add_(-lr * weight_update)
            bias_update = l.bias_grad_buffer * (l.bias_scaling_factor / num_gpus)
            l.bias.data.add_(-lr * bias_update)


def zeroing(layers):  # :261-308
    for l in layers:
        l.weight_grad_buffer.zero_()
        l.weight_scaling_factor.zero_()
        l.bias_grad_buffer.zero_()
        l.bias_scaling_factor.zero_()


def flat(layers, w, b):
    return np.concatenate([np.concatenate([getattr(l, w).detach().numpy().reshape(-1),
                                           getattr(l, b).detach().numpy().reshape(-1)]) for l in layers])


def main():
    recs, inputs = {}, []
    for N in (3, 4):
        layers = [Layer(W, b) for W, b in S.layer_params()]
        zeroing(layers)
        for w in range(WINDOWS):
            for k in range(N):
                gs = S.grads(w, k)
                inputs.append(gs)
                for l, (gW, gb) in zip(layers, gs):
                    l.weight.grad = torch.from_numpy(gW.copy())
                    l.bias.grad = torch.from_numpy(gb.copy())
                grad_buffer_update(layers)
                tag = f"n{N}_w{w}_k{k}"
                recs[tag + "_e"] = flat(layers, "error_compensation_weight", "error_compensation_bias")
                recs[tag + "_buf"] = flat(layers, "weight_grad_buffer", "bias_grad_buffer")
                recs[tag + "_s"] = flat(layers, "weight_scaling_factor", "bias_scaling_factor")
            weights_update(layers, S.LR, N)
            recs[f"n{N}_w{w}_p"] = flat(layers, "weight", "bias")
            zeroing(layers)
    for v in recs.values():
        assert v.dtype == np.float32
    recs.update(shapes=np.asarray(S.SHAPES, np.int64), seed=np.int64(S.SEED), lr=np.float32(S.LR),
                windows=np.int64(WINDOWS), inputs_checksum=np.asarray(G.checksum(inputs, S.layer_params())))
    np.savez_compressed(os.path.join(HERE, "simdp_mlp.npz"), **recs)
    print("wrote simdp_mlp.npz", os.path.getsize(os.path.join(HERE, "simdp_mlp.npz")), "bytes")


if __name__ == "__main__":
    main()
