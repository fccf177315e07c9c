"""Drop-in for the reference's simulated data-parallel quantized SGD
(``sgd_quantized_gradients.py``): one device plays N ranks by running N micro-steps whose
INT8-quantized gradients accumulate in buffers, then one dequantized update.

    grad_buffer_update_added_quantization(model, number_of_gpus, emb_grad_quantized=True)  :56-139
    weights_update_added_quantization(model, lr, num_gpus, emb_grad_quantized, update_embedding) :349-404
    grad_buffer_zeroing(model)                                                                :231-308

Embedding branch (reference): the FIRST micro-step's scale s = max|coalesced grad| / 127 is kept
(``emb_scaling_factor`` is non-zero afterwards) and quantizes every later micro-step; the
buffer holds the exact integer sum; the update is W += -lr * (buffer * fl32(s / N)).
Here each micro-step is coalesced and quantize-packed on the device into its own payload
(dqrm_emb_bwd_coalesce + dqrm_grad_quant_pack with the first micro-step's per-slot
max|grad| as a one-rank scale input), and the update is dqrm_apply_sparse_update over the
N payloads in DQRM_UPD_SIMULATED mode (the integer sum is order-free, hence identical to
the reference's coalesced buffer).

MLP branch (:96-139, :381-404, :261-308): every ``QuantLinear`` of ``bot_l`` then ``top_l`` (this
package's class, as the reference's isinstance test selects) goes through one
``dense.SimulatedDenseBuffers``, created at the first call and kept on the model: the
error-compensated INT8 accumulate is ONE launch per micro-step for all layers
(dqrm_dense_ec_accumulate), the update one more (dqrm_dense_sim_update). The branch runs
whatever ``emb_grad_quantized`` and ``update_embedding`` are, after the embedding branch. A model
without ``bot_l`` / ``top_l``, or with no ``QuantLinear`` in them, is left as it is (the reference
raises a Warning for a missing list).

Embedding modules must be built with ``grad_mode="dp"``.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .comm import HipExchangeKernels, payload_bytes
from .dense import DenseChannels, SimulatedDenseBuffers
from .linear import QuantLinear
from .quant_modules_not_quantize_grad import _QuantEmbeddingBase
from .tables import CoalescedGrad, LookupBatch, default_caps

GRAD_BITS = 8  # the reference hard-codes num_bits = 8 here (:77,:80 and :104-136)


class _MicroStepBuffer:
    """The simulated-DP buffer of one table set: N payloads + the first micro-step's
    per-slot max|grad| and scale."""

    def __init__(self, ts, max_lookups: int):
        self.max_lookups = max_lookups
        self.ws = CoalescedGrad.allocate(ts.num_rows, max_lookups, ts.D, ts.device)
        caps = default_caps(ts.num_rows, max_lookups)
        base = [0]
        for c in caps:
            base.append(base[-1] + c)
        self.cap_total = base[-1]
        self.cap_base = torch.tensor(base, dtype=torch.int64, device=ts.device)
        self.payload_bytes = payload_bytes(ts.T, self.cap_total, ts.D, GRAD_BITS)
        self.payloads: list[torch.Tensor] = []
        self.first_absmax: torch.Tensor | None = None
        self.s_first = torch.zeros(ts.T, dtype=torch.float32, device=ts.device)
        self.kernels = HipExchangeKernels(ts)

    @staticmethod
    def fitting(buf, ts, max_lookups: int):
        """buf if it holds a micro-step of max_lookups lookups per table, else a new buffer."""
        if buf is None or buf.max_lookups < max_lookups:
            if buf is not None and buf.payloads:
                raise ValueError("micro-step batch larger than the first one of this accumulation")
            buf = _MicroStepBuffer(ts, max(max_lookups, 1))
        return buf

    def accumulate(self, batch, dy, ste, layout) -> None:
        """One micro-step (:76-85): coalesce, quantize with the first micro-step's scale, keep."""
        self.kernels.coalesce(batch, dy, self.ws, ste, layout)
        if self.first_absmax is None:  # emb_scaling_factor == 0: this micro-step sets the scale
            self.first_absmax = self.ws.absmax.clone().view(1, -1)
        payload = torch.empty(self.payload_bytes, dtype=torch.uint8, device=self.ws.rows.device)
        self.kernels.quant_pack(self.ws, self.first_absmax, 1, GRAD_BITS, self.cap_base, self.cap_total,
                                self.s_first, payload)
        self.payloads.append(payload)

    def apply(self, lr, num_gpus, repack) -> None:
        """W += -lr * (buffer * (s / N)) (:366-371) over the accumulated payloads."""
        if len(self.payloads) != int(num_gpus):
            raise ValueError(f"{len(self.payloads)} micro-steps accumulated but num_gpus={num_gpus}")
        gathered = torch.stack(self.payloads)
        self.kernels.apply(self.cap_base, self.cap_total, gathered, self.payload_bytes, len(self.payloads),
                           GRAD_BITS, self.s_first, lr, L.DQRM_UPD_SIMULATED, repack)

    def zero(self) -> None:
        self.payloads.clear()
        self.first_absmax = None


def _emb_modules(model) -> list[_QuantEmbeddingBase]:
    emb = getattr(model, "emb_l", None)
    if emb is None:
        raise Warning("Cannot find the list of embedding tables")
    mods = [emb] if isinstance(emb, _QuantEmbeddingBase) else list(emb)
    for m in mods:
        if not isinstance(m, _QuantEmbeddingBase) or m.grad_mode != "dp":
            raise ValueError("simulated DP needs this package's embedding modules with grad_mode='dp'")
    return mods


def _mlp_buffers(model, create: bool) -> SimulatedDenseBuffers | None:
    """The model's SimulatedDenseBuffers over the QuantLinear layers of bot_l then top_l, made at
    the first micro-step and kept in ``model._dqrm_sim_dense``; None for a model without such
    layers. ``model._dqrm_sim_dense_kernels``, if set, is called with the DenseChannels to give
    the kernels (host-only runs); the product has the HIP ones."""
    layers = []
    for name in ("bot_l", "top_l"):
        seq = getattr(model, name, None)
        if seq is not None:
            layers += [l for l in seq if isinstance(l, QuantLinear)]
    if not layers:
        return None
    key = tuple(id(l) for l in layers)
    ent = model.__dict__.get("_dqrm_sim_dense")
    if ent is None or ent[0] != key:
        if not create:
            return None
        factory = model.__dict__.get("_dqrm_sim_dense_kernels")
        kernels = None if factory is None else factory(DenseChannels(layers))
        ent = (key, SimulatedDenseBuffers(layers, grad_bits=GRAD_BITS, kernels=kernels))
        model.__dict__["_dqrm_sim_dense"] = ent
    return ent[1]


def grad_buffer_update_added_quantization(model, number_of_gpus, emb_grad_quantized=True) -> None:
    """sgd_quantized_gradients.py:56-139, one micro-step. Unquantized embedding gradients
    (emb_grad_quantized=False, :88-91): the micro-step's lookups and upstream gradient are
    kept on the device; the update applies buffer = sum of grad / N in the reference's order.
    The MLP branch (:96-139) follows in either case."""
    with torch.no_grad():
        for m in _emb_modules(model):
            if m._pending is None:
                continue
            if not emb_grad_quantized:
                fb = getattr(m, "_sim_fp32", None)
                if fb is None:
                    fb = m._sim_fp32 = []
                fb.append((m._pending, int(number_of_gpus)))
                m._pending = None
                continue
            batch, dy, ste, layout = m._pending
            buf = m._sim_buffer = _MicroStepBuffer.fitting(getattr(m, "_sim_buffer", None), m._tset,
                                                           batch.max_lookups)
            buf.accumulate(batch, dy, ste, layout)
            m.emb_scaling_factor.copy_(buf.s_first.view_as(m.emb_scaling_factor))
            m._pending = None
        sb = _mlp_buffers(model, create=True)
        if sb is not None:
            sb.accumulate()


def _apply_fp32_buffer(m: _QuantEmbeddingBase, lr: float) -> None:
    """The unquantized buffer's update (:374-377): W.add_(-lr * buffer), where the buffer is
    sum over the micro-steps, in order, of grad / N (grad_buffer_update_added_quantization,
    :88-91: buffer.add_(grad / N); buffer.coalesce()). The micro-steps' batches are joined
    bag after bag; one coalesce divides every lookup's gradient by N before the ordered sum
    (dqrm_emb_bwd_coalesce_scaled), and the FP32 payload path applies W + (-lr * buffer)."""
    items = m._sim_fp32
    ts = m._tset
    (_, _, ste, _), N = items[0]
    if any(it[1] != N for it in items) or any(it[0][2] != ste for it in items):
        raise ValueError("micro-steps of one accumulation differ in number_of_gpus or full precision")
    batch = LookupBatch.concat_bags([it[0][0] for it in items])

    def tbd(it):  # a micro-step's upstream gradient as [T, B_i, D] (the modules hand tbd or btd)
        b, g, _, lay = it[0]
        return g.reshape(ts.T, b.num_bags, ts.D) if lay == "tbd" else g.reshape(b.num_bags, ts.T, ts.D).transpose(0, 1)

    dy = torch.cat([tbd(it) for it in items], dim=1).contiguous()
    ws = CoalescedGrad.allocate(ts.num_rows, max(batch.max_lookups, 1), ts.D, ts.device)
    ts.backward_coalesce_scaled(batch, dy, ws, N, ste=ste)
    caps = default_caps(ts.num_rows, max(batch.max_lookups, 1))
    base = [0]
    for c in caps:
        base.append(base[-1] + c)
    cap_base = torch.tensor(base, dtype=torch.int64, device=ts.device)
    pb = payload_bytes(ts.T, base[-1], ts.D, 32)
    payload = torch.zeros(pb, dtype=torch.uint8, device=ts.device)
    k = HipExchangeKernels(ts)
    k.quant_pack(ws, None, 1, 32, cap_base, base[-1], None, payload)
    k.apply(cap_base, base[-1], payload.view(1, -1), pb, 1, 32, None, lr, L.DQRM_UPD_FP32, m._use_packed(False))


def weights_update_added_quantization(model, lr, num_gpus, emb_grad_quantized=True, update_embedding=True) -> None:
    """sgd_quantized_gradients.py:349-404. Embedding branch: W += -lr * buffer * (s / N);
    unquantized (:374-377): W += -lr * buffer. MLP branch (:381-404), in either case and
    whatever update_embedding is: param += -lr * (buffer * (s / N)) per channel."""
    with torch.no_grad():
        for m in _emb_modules(model):
            if not update_embedding:
                break
            if not emb_grad_quantized:
                if getattr(m, "_sim_fp32", None):
                    _apply_fp32_buffer(m, lr)
                continue
            buf = getattr(m, "_sim_buffer", None)
            if buf is None or not buf.payloads:
                continue
            buf.apply(lr, num_gpus, m._use_packed(False))
        sb = _mlp_buffers(model, create=False)
        if sb is not None and sb.micro_steps:
            sb.update(lr, num_gpus)


def grad_buffer_zeroing(model) -> None:
    """sgd_quantized_gradients.py:231-308: empty the buffers and zero the scales (the MLP
    layers' error compensation stays, as in the reference)."""
    for m in _emb_modules(model):
        buf = getattr(m, "_sim_buffer", None)
        if buf is not None:
            buf.zero()
        m._sim_fp32 = []
        m.emb_scaling_factor.zero_()
    sb = _mlp_buffers(model, create=False)
    if sb is not None:
        sb.zero()


__all__ = ["grad_buffer_update_added_quantization", "weights_update_added_quantization", "grad_buffer_zeroing"]
