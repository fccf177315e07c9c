"""CPU restatement of DLRMLoss (csrc/dqrm_loss.hip, include/dqrm.h): the loss_threshold clamp of
DLRM_Net.forward (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:837-839) and loss_fn_wrap (:193-212),
in numpy, every operation rounded on its own in the chosen dtype. With dtype=np.float32 it is the
kernel's arithmetic step by step (logf / log1pf excepted: their bits belong to the device's math
library, see term_bound); with dtype=np.float64 it is the same sequence in double, the form the
host tests hold against torch and the GPU tests measure the f32 terms against.

THE SUM ORDER (ordered_sum), a function of the number of terms alone:
  slot s = i mod 256, s = 0..255, starts at +0.0 and adds its terms i = s, s + 256, ... in
  ascending i; the 256 slots are then folded with slot[s] += slot[s + stride] (s < stride) for
  stride = 128, 64, 32, 16, 8, 4, 2, 1; the sum is slot[0]. loss = sum / B.
"""
from __future__ import annotations

import numpy as np

BCE, MSE, WBCE = "bce", "mse", "wbce"
SLOTS = 256
U = 2.0 ** -24        # half an ulp, relative: one correctly rounded f32 operation
LOG_ULPS = 1.0        # logf and log1pf: 1 ulp each in HIP's table of device math functions


def clamp_bounds(loss_threshold, dtype=np.float32):
    """(active, lo, hi): active only for 0 < threshold < 1; lo = dtype(threshold) and
    hi = dtype(1.0 - threshold), the subtraction in double (torch.clamp with Python scalars)."""
    th = float(loss_threshold)
    return 0.0 < th < 1.0, dtype(th), dtype(1.0 - th)


def clamp(p, loss_threshold):
    """z = min(max(p, lo), hi) in p's dtype, a NaN kept; p itself when the clamp is inactive."""
    active, lo, hi = clamp_bounds(loss_threshold, p.dtype.type)
    if not active:
        return p.copy()
    z = np.where(p < lo, lo, p)
    return np.where(z > hi, hi, z)


def clamp_mask(p, loss_threshold):
    """True where the clamp passes the gradient: lo <= p <= hi (inclusive, as torch's), and for a
    NaN p (the gradient is NaN there anyway)."""
    active, lo, hi = clamp_bounds(loss_threshold, p.dtype.type)
    if not active:
        return np.ones(p.shape, dtype=bool)
    return ~((p < lo) | (p > hi))


def class_weights(t, weights):
    """weights[(int64) t] in t's dtype, the truncation of .long(); NaN for a class outside
    [0, len(weights)) or a NaN t."""
    w = np.asarray(weights, dtype=np.float32).astype(t.dtype)  # cast to f32 once, as the module does
    ok = (t > -1) & (t < len(w))
    c = np.where(ok, t, 0).astype(np.int64)
    ok &= c < len(w)
    return np.where(ok, w[np.where(ok, c, 0)], t.dtype.type(np.nan))


def _floor_at(v, floor):
    return np.where(v < floor, floor, v)  # a NaN stays


def bce_terms(z, t):
    """(t - 1) * max(log1p(-z), -100) - t * max(log(z), -100), each step in z's dtype."""
    T = z.dtype.type
    with np.errstate(divide="ignore", invalid="ignore"):
        a = _floor_at(np.log1p(-z), T(-100.0))
        b = _floor_at(np.log(z), T(-100.0))
    return (t - T(1.0)) * a - t * b


def bce_d(z, t):
    """(z - t) / max((1 - z) * z, 1e-12f): no transcendental, so the f32 form is the kernel's bits.
    The floor is the FLOAT 1e-12f in every dtype, as torch's `constexpr float EPSILON = 1e-12`."""
    T = z.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        return (z - t) / _floor_at((T(1.0) - z) * z, T(np.float32(1e-12)))


def ordered_sum(terms):
    """The sum of a 1-D array in THE SUM ORDER above, in the array's dtype."""
    x = np.asarray(terms).reshape(-1)
    T = x.dtype.type
    rows = -(-x.size // SLOTS)
    m = np.zeros(rows * SLOTS, dtype=x.dtype)  # a slot that ends early adds nothing more:
    m[:x.size] = x                             # the padding's x + 0.0 == x keeps its bits
    m = m.reshape(rows, SLOTS)
    slot = np.zeros(SLOTS, dtype=x.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(rows):
            slot = slot + m[r]
        stride = SLOTS // 2
        while stride >= 1:
            slot = slot[:stride] + slot[stride:2 * stride]
            stride //= 2
    return T(slot[0])


def forward(p, t, kind, loss_threshold=0.0, weights=None, dtype=np.float32):
    """dict(z, w, terms, loss, g) of DLRMLoss over flat p and t, every step in `dtype`:
    terms = w * l, loss = ordered_sum(terms) / B, g = (w * d) / B and 0 where the clamp cut."""
    p = np.asarray(p, dtype=dtype).reshape(-1)
    t = np.asarray(t, dtype=dtype).reshape(-1)
    B = dtype(p.size)
    z = clamp(p, loss_threshold)
    if kind == MSE:
        e = z - t
        w, terms, d = None, e * e, dtype(2.0) * e
    elif kind in (BCE, WBCE):
        terms, d = bce_terms(z, t), bce_d(z, t)
        w = None
        if kind == WBCE:
            w = class_weights(t, weights)
            with np.errstate(invalid="ignore", over="ignore"):
                terms, d = w * terms, w * d
    else:
        raise ValueError(kind)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(clamp_mask(p, loss_threshold), d / B, dtype(0.0))
        loss = ordered_sum(terms) / B
    return dict(z=z, w=w, terms=terms, loss=dtype(loss), g=g)


def backward(g, go):
    """dp = go * g in g's dtype."""
    with np.errstate(invalid="ignore", over="ignore"):
        return g.dtype.type(go) * g


def term_bound(z64, t64, w64):
    """|terms_f32 - terms_f64| for the bce / wbce term, from the kernel's operation sequence

        a = max(log1pf(-z), -100)      b = max(logf(z), -100)
        l = (t - 1) * a - t * b        term = w * l

    over the SAME f32 z, t and w (passed here as float64). With u = 2^-24 (half an ulp, relative)
    and A, Bv the exact log1p(-z), log(z) after the floor:
      * -z is exact; log1pf and logf are within LOG_ULPS = 1 ulp (HIP's documented bound for both
        on the device), i.e. 2u relative each; the floor at -100 is exact and 1-Lipschitz;
      * t - 1 is one rounding (u; exact for t in {0, 1}); (t - 1) * a another: the first product
        carries (2 + 1 + 1) u |(t - 1) A|;
      * t * b is one rounding: (2 + 1) u |t Bv|;
      * the subtraction adds u |l|, the multiply by w scales all of it by |w| and adds u |w l|
        (absent for bce, where w = 1, which only makes the bound looser there).
    1.01 covers the second-order terms, 4 * 2^-149 the four operations when a result is subnormal.
    Where a term is exactly 0 or exactly 100 * w the bound is met with room: those cases are
    asserted exactly by the tests instead."""
    z, t, w = (np.asarray(x, dtype=np.float64) for x in (z64, t64, w64))
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.maximum(np.log1p(-z), -100.0)
        Bv = np.maximum(np.log(z), -100.0)
    first, second = np.abs((t - 1.0) * A), np.abs(t * Bv)
    l = np.abs((t - 1.0) * A - t * Bv)
    log_u = 2.0 * LOG_ULPS
    inner = (log_u + 2.0) * U * first + (log_u + 1.0) * U * second + U * l
    return 1.01 * (np.abs(w) * inner + U * np.abs(w) * l) + 4.0 * 2.0 ** -149


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for f32: any summation order of n terms is within
    gamma_n * sum|x| of the exact sum (THE SUM ORDER's depth is far below n)."""
    return n * U / (1.0 - n * U)
