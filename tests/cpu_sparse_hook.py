"""Float64 references for the autograd / optimizer call patterns of the grad_mode="sparse" modules
(test_sparse_hook_host, test_gpu_autograd_patterns): torch's own semantics, W0 - lr * the sum over
every lookup of every call whose gradient reached .grad, of that lookup's row gradient."""
import numpy as np

F32 = np.float32
F64 = np.float64
RTOL, ATOL = 1e-5, 1e-6  # the suite's tolerance for the optimizer's add of the COO
VISIBLE = 1e-3           # what a dropped or doubled gradient must change, at the least


def sgd(W, calls, lr):
    """W (float64 [n, D]) after one SGD step on the summed gradient of `calls` = [(idx, g)], one
    row g[i] per lookup idx[i]."""
    W = np.array(W, F64)
    for idx, g in calls:
        np.add.at(W, np.asarray(idx), -lr * np.asarray(g, F64))
    return W


def adagrad_first(W, calls, lr, eps=1e-10):
    """W after torch.optim.Adagrad's FIRST step (state_sum 0, no lr decay) on the summed gradient:
    every touched element moves by lr * g / (|g| + eps)."""
    G = np.zeros(np.shape(W), F64)
    for idx, g in calls:
        np.add.at(G, np.asarray(idx), np.asarray(g, F64))
    return np.array(W, F64) - lr * G / (np.sqrt(G * G) + eps)


def touched(calls):
    return np.unique(np.concatenate([np.asarray(idx).ravel() for idx, _ in calls]))


def assert_visible(good, bad, rows, what):
    """The precondition of every case, on the references alone: the defect (one call dropped, one
    gradient applied once more or once less) moves a touched row by a thousand tolerances."""
    d = float(np.abs(np.asarray(good)[rows] - np.asarray(bad)[rows]).max())
    assert d >= VISIBLE, f"{what}: the defect would change W by {d:.3g} only"
    return d


def assert_weights(got, want, what):
    np.testing.assert_allclose(np.asarray(got, F64), want, rtol=RTOL, atol=ATOL, err_msg=what)


def normal(seed, shape, scale=0.5):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(F32)
