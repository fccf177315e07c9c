"""CPU restatement of DLRMMetrics (include/dqrm.h, csrc/dqrm_metrics.hip): the contract in numpy,
with ``np.sort``, ``np.searchsorted`` and Python ints. It is the checker of the GPU tests; sklearn
enters only through the recorded fixture (tests/golden/metrics.npz).

For (z, t) pairs, both float32:
  n_correct  #{ rint(z) == t }                       (np.round(S, 0) == T in f32, ties to even)
  key        s = z + 0.0f; b = bits(s); key = b >> 31 ? ~b : b | 0x80000000   (uint32)
  class      t == 1 positive, t == 0 negative; anything else F_LABEL; a non-finite z F_NONFINITE
  twice_u    sum over positives i of 2 * #{neg j: key_j < key_i} + #{neg j: key_j == key_i}
  roc_auc    twice_u / (2 * P * N), one division of Python ints (correctly rounded)
"""
from fractions import Fraction

import numpy as np

F_LABEL = 1
F_NONFINITE = 2


def keys_of(z):
    """The order-preserving uint32 key of every float32 score (-0 keyed as +0)."""
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    s = z + np.float32(0.0)
    b = s.view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def classes(t):
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    return t == np.float32(1.0), t == np.float32(0.0)


def flags_of(z, t):
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    pos, neg = classes(t)
    f = 0
    if not np.all(pos | neg):
        f |= F_LABEL
    if not np.all(np.isfinite(z)):
        f |= F_NONFINITE
    return f


def n_correct(z, t):
    z = np.ascontiguousarray(z, dtype=np.float32).reshape(-1)
    t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
    return int(np.count_nonzero(np.rint(z) == t))


def twice_u_sorted_negatives(kp, kn):
    """Every positive adds lb + ub in the sorted negatives."""
    a = np.sort(kn)
    lb = np.searchsorted(a, kp, side="left")
    ub = np.searchsorted(a, kp, side="right")
    return sum(int(v) for v in lb) + sum(int(v) for v in ub)


def twice_u_sorted_positives(kp, kn):
    """Every negative adds 2 P - lb - ub in the sorted positives."""
    a = np.sort(kp)
    lb = np.searchsorted(a, kn, side="left")
    ub = np.searchsorted(a, kn, side="right")
    return 2 * int(kp.size) * int(kn.size) - sum(int(v) for v in lb) - sum(int(v) for v in ub)


def compute(z, t, branch=None):
    """The result struct as Python ints, the two classes' keys, and the derived numbers.
    branch: None (the kernels' choice: the smaller class is sorted, the positives on a tie),
    "neg" or "pos" (which class is sorted)."""
    k = keys_of(z)
    pos, neg = classes(t)
    kp, kn = k[pos], k[neg]
    P, N = int(kp.size), int(kn.size)
    if branch is None:
        branch = "pos" if P <= N else "neg"
    tu = twice_u_sorted_positives(kp, kn) if branch == "pos" else twice_u_sorted_negatives(kp, kn)
    n = int(k.size)
    nc = n_correct(z, t)
    return {"n": n, "n_pos": P, "n_neg": N, "n_correct": nc, "twice_u": tu, "flags": flags_of(z, t),
            "keys_pos": kp, "keys_neg": kn, "sorted": branch,
            "test_acc": nc / n if n else float("nan"),
            "roc_auc": tu / (2 * P * N) if P and N else float("nan"),
            "roc_auc_exact": Fraction(tu, 2 * P * N) if P and N else None}
