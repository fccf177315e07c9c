"""CPU restatement (numpy / torch-CPU) of the LSQ and PACT embedding quantizers' arithmetic
contracts (include/dqrm.h, "The LSQ and PACT embedding quantizers"): every named
step one IEEE f32 operation, bag sums sequential f32 adds in bag order from 0, and the LSQ step
gradient reduced in the documented shape -- 4096 strided fmaf chains per table over the elements
e = b*D + d, then a pairwise tree over the chain index."""
import math

import numpy as np
import torch

F32 = np.float32
F64 = np.float64
LSQ_CHAINS = 4096


# ------------------------------------------------------------------ shared
def bag_sums(rows, idx, off):
    """x[b] = sum of rows[i] for the lookups i of bag b, f32 adds in bag order from 0. rows f32
    [L, D]: lookup i's addend (the gathered row itself, or its mapped values)."""
    B, L = len(off), len(idx)
    out = np.zeros((B, rows.shape[1]), F32)
    for b in range(B):
        s0, s1 = int(off[b]), int(off[b + 1]) if b + 1 < B else L
        acc = np.zeros(rows.shape[1], F32)
        for i in range(s0, s1):
            acc = acc + rows[i]
        out[b] = acc
    return out


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays, exactly: the product is exact in f64, the f64 sum is rounded
    to odd with its exact error (TwoSum), and the rounding of that to f32 is then the single
    rounding of a*b + c."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def chain_tree_sum(a, b, chains=LSQ_CHAINS):
    """sum_e a_e * b_e in the kernels' shape: chain c = fmaf over e = c, c + chains, ... in
    ascending order from 0, then neighbours added pairwise, level by level."""
    a, b = np.ravel(a).astype(F32), np.ravel(b).astype(F32)
    n = a.size
    acc = np.zeros(chains, F32)
    for k in range(0, n, chains):
        m = min(chains, n - k)
        acc[:m] = fma32(a[k:k + m], b[k:k + m], acc[:m])
    while acc.size > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


# ------------------------------------------------------------------ LSQ
def lsq_consts(bit, n):
    lo, hi = -(2 ** (bit - 1)), 2 ** (bit - 1) - 1
    return F32(lo), F32(hi), F32(1.0 / math.sqrt(float(hi) * n))


def lsq_s_eff(s, g):
    s, g = F32(s), F32(g)
    sg = s * g
    return F32(F32(s - sg) + sg)


def lsq_init_step(W, bit=4):
    """mean|W| * 2 / sqrt(hi) with torch's CPU ops, as the reference's init_from does."""
    hi = 2 ** (bit - 1) - 1
    return (torch.from_numpy(np.ascontiguousarray(W)).abs().mean() * 2 / (hi ** 0.5)).numpy().astype(F32)


def lsq_forward(x, s, bit=4):
    """y for the bag sums x f32 [B, D] and the step s."""
    lo, hi, g = lsq_consts(bit, x.size)
    se = lsq_s_eff(s, g)
    q = x / se
    return np.rint(np.minimum(np.maximum(q, lo), hi)) * se


def lsq_terms(x, dy, s, bit=4):
    """(dx, r, gq, qs, g): the backward's elementwise values, all f32."""
    lo, hi, g = lsq_consts(bit, x.size)
    se = lsq_s_eff(s, g)
    q = x / se
    r = np.rint(np.minimum(np.maximum(q, lo), hi))
    m = (q >= lo) & (q <= hi)
    gq = np.where(m, dy * se, F32(0))
    return gq / se, r, gq, q / se, g


def lsq_backward(x, dy, s, bit=4):
    """(dx, ds): the gradient of the bag sums and of the step."""
    dx, r, gq, qs, g = lsq_terms(x, dy, s, bit)
    s1 = chain_tree_sum(dy, r)
    s2 = chain_tree_sum(-gq, qs)
    return dx, F32(F32(s1 + s2) * g)


def find_s_eff_pair(seed=0, tries=200000):
    """A (s, n) with (s - s*g) + s*g != s, by a seeded search (about 1 in 2000 random pairs)."""
    rs = np.random.RandomState(seed)
    for _ in range(tries):
        s = F32(rs.uniform(0.005, 0.05))
        B, D = int(rs.randint(1, 131)), int(rs.choice([4, 16, 64]))
        g = lsq_consts(4, B * D)[2]
        if lsq_s_eff(s, g) != s:
            return s, B, D
    raise AssertionError("no (s, n) pair with s_eff != s found")


# ------------------------------------------------------------------ PACT / DoReFa
def pact_values(w, tmax, k):
    """v f32 for the weights w f32, every step in f32 (torch's CPU tanh)."""
    sc = F32(2 ** k - 1)
    t = torch.tanh(torch.from_numpy(np.ascontiguousarray(w, dtype=F32))).numpy()
    mt = torch.tanh(torch.tensor(F32(tmax))).numpy().astype(F32)
    u = t / (F32(2) * mt)
    a = u + F32(0.5)
    j = np.rint(sc * a)
    return F32(2) * (j / sc) - F32(1)


def pact_truth(w, tmax, k):
    """(v, near): the level of every weight decided in float64, m = tanh(max|W|), mapped to v by
    the f32 formula; near marks |frac(sc * (t / (2m) + 0.5)) - 0.5| < sc * 2^-20, where the f32
    kernel may land on the neighbouring level."""
    sc = float(2 ** k - 1)
    arg = sc * (np.tanh(w.astype(F64)) / (2.0 * np.tanh(F64(tmax))) + 0.5)
    near = np.abs((arg - np.floor(arg)) - 0.5) < sc * 2.0 ** -20
    j = np.rint(arg).astype(F32)
    return F32(2) * (j / F32(sc)) - F32(1), near

