"""The two numbers of the reference's test loop, kept on the device (csrc/dqrm_metrics.hip; no CPU
fallback): ``inference()`` (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1304-1404) synchronises and
copies scores and targets to the host per test batch, counts ``np.round(S, 0) == T`` and ends with
``sklearn.metrics.roc_auc_score``. ``DLRMMetrics`` takes each batch's scores where the forward left
them:

  * ``update(Z, T)`` (1 launch, no sync): every sample's order-preserving integer key is appended to
    its class's side of one buffer; the correct count and the two validity flags accumulate as
    integers. The sample count is kept on the host.
  * ``compute()``: dqrm_metrics_finish (``finish_launches()`` launches: the smaller class radix-sorted
    in place, the other class searching it) and ONE 40-byte read-back.

``roc_auc`` is ``twice_u / (2 * n_pos * n_neg)``, one float64 division of exact integers: twice the
Mann-Whitney U with ties counted one half, the area sklearn's trapezoid over ``roc_curve`` computes.
Its bits depend on the multiset of samples alone, not on batch order, batch size or the grid.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib as L
from .mlp import _on_device
from .tables import _stream_handle

_FLAG_TEXT = (
    (L.DQRM_METRICS_F_LABEL, "DQRM_METRICS_F_LABEL: a target that is neither 0.0 nor 1.0"),
    (L.DQRM_METRICS_F_NONFINITE, "DQRM_METRICS_F_NONFINITE: a NaN or infinite score"),
    (L.DQRM_METRICS_F_COUNT, "DQRM_METRICS_F_COUNT: the device counters contradict the samples seen"),
)


class DLRMMetrics:
    """Test accuracy and exact ROC AUC over a stream of ``(Z, T)`` batches of at most ``capacity``
    samples in all. It grows nothing: one ``keys`` buffer of ``capacity`` uint32 and four counter
    words, allocated here; the finish's workspace is allocated at the first ``compute()`` of a size
    and reused."""

    def __init__(self, capacity, device="cuda"):
        capacity = int(capacity)
        if not 1 <= capacity <= L.DQRM_METRICS_MAX_SAMPLES:
            raise ValueError(f"DLRMMetrics capacity must be 1..{L.DQRM_METRICS_MAX_SAMPLES} (got {capacity})")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.DQRMError(f"DLRMMetrics runs on libdqrm's HIP kernels: it must be on a GPU (got {dev}); "
                              "there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.capacity = capacity
        self.device = dev
        self.lib = L.load()
        self.keys = torch.empty(capacity, dtype=torch.int32, device=dev)  # uint32 bits
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self._out = torch.zeros(5, dtype=torch.int64, device=dev)
        self._ws = None
        self.n = 0  # samples since the reset: the host's own count, nothing is read back for it
        self.raw = None  # the latest compute()'s dqrm_metrics_result as Python ints (twice_u among them)
        self.c = L.Metrics()
        self.c.capacity, self.c.keys, self.c.counters = capacity, self.keys.data_ptr(), self.counters.data_ptr()
        self.reset()

    def reset(self):
        """Forget every sample (a 32-byte memset on the current stream)."""
        _on_device(self.device, self._reset)
        self.n = 0

    def _reset(self):
        L.check(self.lib.dqrm_metrics_reset(C.byref(self.c), _stream_handle()), "dqrm_metrics_reset")

    def _check(self, Z, T):
        if not isinstance(Z, torch.Tensor) or not isinstance(T, torch.Tensor):
            raise TypeError("DLRMMetrics.update needs two tensors (the scores and the targets)")
        for name, x in (("scores", Z), ("targets", T)):
            if x.dtype != torch.float32 or not x.is_contiguous():
                raise ValueError(f"DLRMMetrics.update needs contiguous float32 {name} (got {x.dtype}, "
                                 f"contiguous={x.is_contiguous()})")
        if not (Z.dim() == 1 or (Z.dim() == 2 and Z.shape[1] == 1)):
            raise ValueError(f"DLRMMetrics.update needs [B, 1] or [B] scores (got {tuple(Z.shape)})")
        if T.numel() != Z.numel():
            raise ValueError(f"scores have {Z.numel()} elements, targets {T.numel()}")
        if Z.numel() < 1:
            raise ValueError("DLRMMetrics.update needs at least one sample")
        if self.n + Z.numel() > self.capacity:
            raise ValueError(f"DLRMMetrics capacity {self.capacity} exceeded: {self.n} samples seen, "
                             f"{Z.numel()} more given (it grows nothing: size it for the whole test set)")
        if Z.device.type != "cuda":
            raise L.DQRMError(f"DLRMMetrics runs on libdqrm's HIP kernels: the scores must be on a GPU "
                              f"(got {Z.device}); there is no CPU path")
        if Z.device != self.device or T.device != self.device:
            raise ValueError(f"DLRMMetrics on {self.device} but scores on {Z.device} and targets on {T.device}")

    def update(self, Z, T):
        """Add a batch: contiguous float32 scores and targets, ``[B]`` or ``[B, 1]``, on the device.
        One launch on the current stream; nothing is synchronised or read back."""
        self._check(Z, T)
        _on_device(self.device, self._update, Z, T)

    def _update(self, Z, T):
        B = Z.numel()
        L.check(self.lib.dqrm_metrics_update(C.byref(self.c), Z.data_ptr(), T.data_ptr(), B, self.n, _stream_handle()),
                "dqrm_metrics_update")
        self.n += B

    def finish_launches(self):
        """The kernel launches of ``compute()`` for the samples seen so far."""
        n = self.lib.dqrm_metrics_finish_launches(self.n)
        if n < 0:
            L.check(n, "dqrm_metrics_finish_launches")
        return n

    def _finish(self):
        need = self.lib.dqrm_metrics_workspace_bytes(self.n)
        if need == 0:
            L.check(L.DQRM_E_INVALID, "dqrm_metrics_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        L.check(self.lib.dqrm_metrics_finish(C.byref(self.c), self.n, self._out.data_ptr(), self._ws.data_ptr(),
                                             self._ws.numel(), _stream_handle()), "dqrm_metrics_finish")

    def compute(self):
        """``{"n", "n_pos", "n_correct", "test_acc", "roc_auc"}`` over everything seen since the
        reset: the finish and one 40-byte read-back. The state stays valid: more updates may follow.
        A flagged stream (a NaN / infinite score, a target other than 0 and 1) raises ValueError, as
        sklearn does; a stream with one class only gives ``roc_auc = nan`` with a RuntimeWarning."""
        if self.n < 1:
            raise ValueError("DLRMMetrics.compute: no sample seen since the reset")
        _on_device(self.device, self._finish)
        r = self._out.cpu().numpy().view(np.uint64)
        n_pos, n_neg, n_correct, twice_u, flags = (int(v) for v in r)
        self.raw = {"n_pos": n_pos, "n_neg": n_neg, "n_correct": n_correct, "twice_u": twice_u, "flags": flags}
        if flags:
            raise ValueError("DLRMMetrics.compute: " + "; ".join(text for bit, text in _FLAG_TEXT if flags & bit))
        if n_pos == 0 or n_neg == 0:
            warnings.warn("Only one class is present in the targets: ROC AUC is not defined", RuntimeWarning,
                          stacklevel=2)
            auc = float("nan")
        else:
            auc = twice_u / (2 * n_pos * n_neg)  # one float64 division: correctly rounded from exact integers
        return {"n": self.n, "n_pos": n_pos, "n_correct": n_correct, "test_acc": n_correct / self.n, "roc_auc": auc}


__all__ = ["DLRMMetrics"]
