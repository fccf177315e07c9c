"""All tables of a model in the reference's row-wise PTQ formats, gathered in one launch.

``DLRM_Net.quantize_embedding(bits)`` (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:683-700) prepacks
every table with ``embedding_bag_{4bit,byte}_prepack`` and ``apply_emb`` (:639-659) then gathers
table after table with ``embedding_bag_{4bit,byte}_rowwise_offsets``. ``RowwiseTableSet`` holds
the T packed tables as ONE ``uint8 [R, row_bytes]`` slab (``quantized_ops``' row layout, byte for
byte) and ``forward`` runs every table's bags as one launch (dqrm_rowwise_set_fwd), with the
per-table ops' bits. There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import _lib as L
from .tables import EmbeddingTableSet, LookupBatch, _ptr, _stream_handle

SUPPORTED_DIMS = (8, 16, 32, 64, 128, 256)


def _check_bits(bits, who):
    if isinstance(bits, bool) or bits not in (4, 8):
        raise ValueError(f"{who}: bits must be 4 or 8, got {bits!r}")
    return int(bits)


class RowwiseTableSet:
    """T row-wise quantized tables of dim D in one packed slab.

    ``packed``: ``uint8 [R, row_bytes]`` (4-bit: D/2 nibble bytes | fp16 scale | fp16 bias; byte: D
    bytes | f32 scale | f32 bias); ``T``, ``D``, ``bits``, ``num_rows``. Build one with
    ``from_tables`` (an ``EmbeddingTableSet``: one prepack launch over its whole FP32 slab),
    ``from_weights`` (a list of ``[n, D]`` tensors) or ``from_packed`` (a slab packed earlier).
    """

    def __init__(self, packed: torch.Tensor, num_rows: Sequence[int], dim: int, bits: int):
        self.lib = L.load()
        self.bits = _check_bits(bits, "RowwiseTableSet")
        self.D = int(dim)
        if self.D not in SUPPORTED_DIMS:
            raise ValueError(f"embedding dim {dim} unsupported (built for {SUPPORTED_DIMS})")
        self.num_rows = [int(n) for n in num_rows]
        self.T = len(self.num_rows)
        if not 1 <= self.T <= 256:
            raise ValueError("1..256 tables supported")
        self.R = sum(self.num_rows)
        self.row_bytes = int(self.lib.dqrm_rowwise_row_bytes(self.bits, self.D))
        if (not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or not packed.is_cuda
                or tuple(packed.shape) != (self.R, self.row_bytes) or not packed.is_contiguous()):
            raise ValueError(f"packed must be a contiguous uint8 CUDA tensor [{self.R}, {self.row_bytes}]")
        if min(self.num_rows) < 0 or self.R < 1:
            raise ValueError("RowwiseTableSet needs at least one row")
        self.packed = packed
        self.device = packed.device
        self.row_base = [0]
        for n in self.num_rows[:-1]:
            self.row_base.append(self.row_base[-1] + n)
        self.meta = torch.tensor([self.row_base, self.num_rows], dtype=torch.int64, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._err_host, self._err_evt, self._err_pending = None, None, False
        self._c = L.RowwiseSet(self.T, self.D, self.bits, 0, self.R, _ptr(self.packed), _ptr(self.meta),
                               _ptr(self.err))

    @property
    def c(self) -> L.RowwiseSet:
        return self._c

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_tables(cls, tables: EmbeddingTableSet, bits: int) -> "RowwiseTableSet":
        """Every table of ``tables`` prepacked by ONE dqrm_rowwise_prepack over its ``[R, D]`` slab
        (prepacking is per row, so the slab packs as one table); ``tables`` is not modified."""
        bits = _check_bits(bits, "RowwiseTableSet.from_tables")
        if tables.D not in SUPPORTED_DIMS:
            raise ValueError(f"embedding dim {tables.D} unsupported (built for {SUPPORTED_DIMS})")
        lib = L.load()
        rb = int(lib.dqrm_rowwise_row_bytes(bits, tables.D))
        W = tables.W
        packed = torch.empty((tables.R, rb), dtype=torch.uint8, device=W.device)
        with torch.cuda.device(W.device):
            L.check(lib.dqrm_rowwise_prepack(bits, W.data_ptr(), tables.R, tables.D, packed.data_ptr(),
                                             _stream_handle()), "dqrm_rowwise_prepack")
        return cls(packed, tables.num_rows, tables.D, bits)

    @classmethod
    def from_weights(cls, weights: Sequence[torch.Tensor], bits: int, device=None) -> "RowwiseTableSet":
        """From a list of ``[n, D]`` float tensors (one prepack launch over their concatenation)."""
        bits = _check_bits(bits, "RowwiseTableSet.from_weights")
        if len(weights) < 1 or any(w.dim() != 2 or w.shape[1] != weights[0].shape[1] for w in weights):
            raise ValueError("from_weights needs a list of [n, D] tensors of one D")
        if not torch.cuda.is_available():
            raise L.DQRMError("row-wise quantized tables live on the GPU only (no CPU path)")
        dev = torch.device(device) if device is not None else (
            weights[0].device if weights[0].is_cuda else torch.device("cuda", torch.cuda.current_device()))
        D = int(weights[0].shape[1])
        if D not in SUPPORTED_DIMS:
            raise ValueError(f"embedding dim {D} unsupported (built for {SUPPORTED_DIMS})")
        W = torch.cat([w.detach().to(device=dev, dtype=torch.float32) for w in weights]).contiguous()
        lib = L.load()
        rb = int(lib.dqrm_rowwise_row_bytes(bits, D))
        packed = torch.empty((W.shape[0], rb), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.dqrm_rowwise_prepack(bits, W.data_ptr(), W.shape[0], D, packed.data_ptr(),
                                             _stream_handle()), "dqrm_rowwise_prepack")
        return cls(packed, [int(w.shape[0]) for w in weights], D, bits)

    @classmethod
    def from_packed(cls, packed: torch.Tensor, num_rows: Sequence[int], dim: int, bits: int) -> "RowwiseTableSet":
        """Over a slab packed earlier (per-table prepack results concatenated, or a saved one)."""
        return cls(packed, num_rows, dim, bits)

    def table_packed(self, t: int) -> torch.Tensor:
        """Table t's packed rows, a view: byte-equal to the per-table prepack op's result."""
        b = self.row_base[t]
        return self.packed[b: b + self.num_rows[t]]

    @property
    def nbytes(self) -> int:
        return self.packed.numel()

    # ------------------------------------------------------------------ errors
    poll_errors = EmbeddingTableSet.poll_errors  # the non-blocking pinned snapshot of `err`

    def read_errors(self, clear: bool = True) -> int:
        """The device error flags (DQRM_ERRF_*), synchronising; clear: reset them."""
        flags = int(self.err.item()) & 0xFFFFFFFF
        if flags and clear:
            self.err.zero_()
        return flags

    # ------------------------------------------------------------------ forward
    def forward(self, batch: LookupBatch, per_sample_weights: torch.Tensor | None = None, layout: str = "btd",
                out: torch.Tensor | None = None, check: bool = False) -> torch.Tensor:
        """Every table's bags in one launch: ``[B, T, D]`` (layout "btd", the interaction's order) or
        ``[T, B, D]`` ("tbd"), float32, with ``embedding_bag_{4bit,byte}_rowwise_offsets``' bits per
        table. per_sample_weights: float32 ``[sum L_t]``, parallel to ``batch.idx``. out: a float32
        tensor of that shape whose last dim is contiguous (other strides multiples of 4, 16-byte
        aligned). check=True reads the error word (a host sync) and raises ``IndexError`` for an
        index outside its table, ``ValueError`` for bad offsets, as the per-table ops do."""
        if not isinstance(batch, LookupBatch):
            raise TypeError("RowwiseTableSet.forward takes a LookupBatch")
        if batch.num_tables != self.T:
            raise ValueError("batch has %d tables, set has %d" % (batch.num_tables, self.T))
        if layout not in ("btd", "tbd"):
            raise ValueError("layout must be 'btd' or 'tbd'")
        if batch.idx.device != self.device:
            raise ValueError(f"batch on {batch.idx.device} but the set on {self.device}")
        B, T, D = batch.num_bags, self.T, self.D
        shape = (B, T, D) if layout == "btd" else (T, B, D)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != shape
              or out.stride(2) != 1):
            raise ValueError(f"out must be a float32 {shape} tensor on {self.device} with a contiguous last dim")
        sb, st = (out.stride(0), out.stride(1)) if layout == "btd" else (out.stride(1), out.stride(0))
        psw = None
        if per_sample_weights is not None:
            psw = per_sample_weights
            if psw.dtype != torch.float32 or psw.device != self.device or not psw.is_contiguous():
                psw = psw.to(device=self.device, dtype=torch.float32).contiguous()
            if psw.numel() != batch.idx.numel():
                raise ValueError("per_sample_weights must have one weight per index")
        with torch.cuda.device(self.device):
            L.check(self.lib.dqrm_rowwise_set_fwd(C.byref(self._c), C.byref(batch.c), _ptr(psw), _ptr(out), st, sb,
                                                  _stream_handle()), "dqrm_rowwise_set_fwd")
        if check:
            flags = self.read_errors(clear=True)
            if flags & L.DQRM_ERRF_INDEX:
                raise IndexError("embedding_bag: an index is out of range of its table")
            if flags:
                raise ValueError("embedding_bag: offsets must be non-decreasing and within [0, len(indices)]")
        return out


__all__ = ["RowwiseTableSet"]
