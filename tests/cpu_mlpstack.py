"""CPU restatement of MLPStack.sgd_step's arithmetic (dqrm_mlp_sgd) and the inputs the MLPStack
tests share.

What it restates, in numpy float32 with every product and sum rounded on its own:
  sgd_quantized_gradients_parallel_comm.py:645-646   W += -lr * grad
  sgd_quantized_gradients_parallel_comm.py:642-643   W += (-lr * grad) * s
The quantization that follows the update is tests/cpu_linear.py's ``quantize``.
"""
from __future__ import annotations

import numpy as np
import torch

import cpu_linear as R

# name -> (ln, sigmoid_layer) of create_mlp
STACKS = {
    "A": ([13, 32, 16], -1),   # ReLU throughout
    "B": ([20, 32, 1], 1),     # sigmoid last, a one-column output
    "C": ([130, 37, 5], -1),   # rows longer than a wave's stride, row counts that are no multiple of 4
}
BATCH = 33


def sgd(p: np.ndarray, g: np.ndarray, lr: float, s=None) -> np.ndarray:
    """p + (nlr * g) [* s] with nlr = -(float)lr: float32 operands, so numpy rounds each
    operation to float32 (s: a float32 scalar or a column of per-row scales)."""
    assert p.dtype == np.float32 and g.dtype == np.float32
    t = np.float32(-np.float32(lr)) * g
    if s is not None:
        t = t * np.asarray(s, dtype=np.float32)
    assert t.dtype == np.float32
    return p + t


def sgd_single_rounding(p: np.ndarray, g: np.ndarray, lr: float) -> np.ndarray:
    """What an FMA would give: p + nlr * g rounded once. The float64 product of two float32
    values is exact; the float64 sum is within half a float64 ulp of the exact one, far below the
    float32 rounding that follows."""
    nlr = np.float64(np.float32(-np.float32(lr)))
    return (p.astype(np.float64) + nlr * g.astype(np.float64)).astype(np.float32)


def quantize(W: np.ndarray, b: np.ndarray, bits: int, per_channel: bool):
    """(scale, weight_integer, bias_integer) of cpu_linear.quantize, as numpy arrays."""
    s, wi, bi = R.quantize(torch.from_numpy(W), torch.from_numpy(b), bits, per_channel)
    return s.numpy(), wi.numpy(), bi.numpy()


def random_grads(shapes, seed):
    """[(dw, db)] standard-normal float32 gradients for layers of the given (out, in) shapes."""
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal((o, k)).astype(np.float32), rs.standard_normal(o).astype(np.float32))
            for o, k in shapes]


def tie_case(O, K, bits, seed):
    """(W, b) on which round(1/s * v) meets exact ties: cpu_linear.exact_case's rows (integers
    times 2^-k reaching +-n, so s = 2^-k exactly) with about a quarter of the other elements, and
    every other bias element, moved to (j + 1/2) * 2^-k for an integer j in [-n, n - 1]."""
    W, b, _, _ = R.exact_case(1, K, O, bits, True, seed)
    W, b = W.numpy().copy(), b.numpy().copy()
    n = R.qmax(bits)
    s = np.abs(W).max(axis=1, keepdims=True) / n
    rs = np.random.RandomState(seed + 1)
    half = ((rs.randint(-n, n, (O, K)) + 0.5) * s).astype(np.float32)
    pick = (rs.randint(0, 4, (O, K)) == 0) & (np.abs(W) < n * s)
    W = np.where(pick, half, W)
    b[::2] = ((rs.randint(-n, n, O) + 0.5) * s[:, 0]).astype(np.float32)[::2]
    assert np.array_equal(np.abs(W).max(axis=1, keepdims=True) / n, s)
    return W, b
