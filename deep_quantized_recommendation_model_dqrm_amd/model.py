"""The reference's ``DLRM_Net`` (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:214-880) assembled from
the package's stages, with a training step that is ONE host call.

``DQRMNet`` owns an ``EmbeddingTableSet`` (all tables in one slab), ``bot_l`` / ``top_l`` from
``create_mlp`` (the reference's state-dict keys) with an ``MLPStack`` each, a ``DotInteraction`` and
a ``DLRMLoss``.

  * ``forward(dense_x, batch)`` is the autograd composition of those modules: nothing in it is
    new. It serves training under ``torch.autograd`` and is what the step is tested against.
  * ``predict(dense_x, batch, labels=None)`` is dqrm_model_fwd: the same forward as one host call.
  * ``train_step(dense_x, batch, labels, lr)`` is dqrm_model_step: forward, loss, backward, the
    embedding SGD and the update of both MLP stacks (one launch, requantization included) behind
    one ABI crossing: no autograd graph, no per-stage tensors, no optimizer. The library calls the
    stages' own exports in the composition's order, so every buffer holds the composition's bits.

  * ``quantize_embedding(bits)`` is the reference's ``DLRM_Net.quantize_embedding`` (:683-700): the
    tables prepacked row-wise to INT4 / INT8 (``RowwiseTableSet``); ``predict`` and ``evaluate`` then
    run from the packed rows (dqrm_model_fwd_rowwise: still one host call and one embedding launch
    per batch) and the FP32 slab may be released.

A model is built on its GPU (``device=``) and stays there; there is no CPU path.

``micro_step`` / ``apply_micro_steps`` are the reference's simulated data parallelism (N micro-steps
into INT8 gradient buffers, one dequantized update) for the whole model on one device.

World size > 1 is out of scope of ``train_step``'s update: use ``train_step(..., update=False)``,
which stops after the backward and leaves the gradients in ``p.grad`` and ``model.emb_grad`` for
the package's DP hooks (``sgd_quantized_gradients_parallel_comm``) to exchange and apply.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .act import QuantAct
from .dense import SimulatedDenseBuffers
from .interaction import DotInteraction, out_features
from .loss import DLRMLoss
from .mlp import MLPStack, _on_device, create_mlp
from .quant_modules_not_quantize_grad import error_check_due, poll_device_errors, raise_device_errors
from .rowwise import RowwiseTableSet
from .sgd_quantized_gradients import GRAD_BITS, _MicroStepBuffer
from .tables import EmbeddingTableSet, LookupBatch, _stream_handle


def _no_cpu(what, dev):
    return L.DQRMError(f"DQRMNet.{what} runs on libdqrm's HIP kernels: the model must be on a GPU (got {dev}); "
                       "there is no CPU path")


class DQRMNet(nn.Module):
    """``DLRM_Net`` with the dot interaction, under the reference's argument names where they apply.

    ln_emb: rows per table; m_spa: the embedding dim; ln_bot / ln_top: the MLPs' widths
    (``ln_bot[-1] == m_spa``, ``ln_top[0] == m_spa + pairs``, ``ln_top[-1] == 1``); sigmoid_top /
    sigmoid_bot: the layer a Sigmoid follows (default: the top stack's last layer, none at the
    bottom); arch_interaction_itself; quantize_bits: None, or 2..16 for the fake-quantized
    interaction (the reference hard-codes 16); weight_bit, per_channel, full_precision_flag: the
    MLP layers'; embedding_bit, embedding_full_precision: the tables'; loss_function, loss_weights,
    loss_threshold: ``DLRMLoss``'s. Tables, then ``bot_l``, then ``top_l`` draw their initial
    values from numpy's global generator, in the reference's order (emb_weights: given tables).

    ``forward`` returns the top stack's output p ``[B, 1]``; the clamp of ``DLRM_Net.forward`` is
    ``DLRMLoss``'s (``model.loss(p, T, return_clamped=True)``). ``predict`` without labels returns
    p; with labels ``(E, Z)``, the loss and the clamped prediction.

    Freshness. ``train_step`` passes DQRM_MODEL_MLP_FRESH only while both ``MLPStack``s are fresh
    by their own records (mlp.MLPStack: storage, parameter versions, layer settings, the raw-write
    epoch), and after an updating step re-records them as ``MLPStack.sgd_step`` does (every written
    parameter's version is bumped). An optimizer step, ``load_state_dict``, ``p.add_()`` are
    caught; after a write through ``.data`` call ``invalidate()``.

    Prefetch. ``train_step(..., next_batch=nb)`` leaves nb's embedding forward in the workspace
    (inside the update's launch for small Criteo-form batches). The following ``train_step`` skips
    its own embedding forward only if its ``batch`` is that very object, the batch size is the
    same and no table write went through ``model.tables``'s methods or this
    model's other calls in between; otherwise it runs the forward itself.

    Quantized serving. After ``quantize_embedding(bits)`` (4 or 8) ``quantize_emb`` is True,
    ``quantize_bits`` is ``bits`` and ``emb_q`` the ``RowwiseTableSet``; ``predict`` / ``evaluate`` read
    it (no fake-quant on top, as the reference's ``apply_emb`` :639-659), ``forward`` and
    ``train_step`` raise ``RuntimeError`` (the reference's ``emb_l`` is ``None`` there).
    ``keep_fp32=True`` keeps the untouched FP32 tables, and ``dequantize_embedding()`` returns to
    them; ``keep_fp32=False`` releases them: ``tables`` is None and the ``emb_weight`` buffer gives
    way to ``emb_packed``, the packed slab, in ``state_dict()``.

    Simulated data parallelism. ``micro_step(dense_x, batch, labels, N)`` N times, then
    ``apply_micro_steps(lr, N)``: one device plays N ranks as the reference's pseudo-multigpu driver
    does with ``sgd_quantized_gradients``: INT8 gradient buffers for the tables and, with error
    compensation, for both stacks (one launch per micro-step and one per update for all MLP
    layers). Both raise ``RuntimeError`` after ``quantize_embedding``, as ``train_step`` does.

    ``quantize_activation=True`` (the drivers' ``--quantize_activation``) adds ``quant_input`` and
    ``quant_feature_outputs`` (``QuantAct``, under the reference's attribute names, activation_bit =
    max(weight_bit, 8), act_range_momentum=-1) in front of the two stacks, whose layers take their
    integer-activation branch; ``forward`` composes them and ``train_step`` / ``predict`` /
    ``evaluate`` run dqrm_model_step_qact / dqrm_model_fwd_qact. The QuantActs' ``x_min``, ``x_max``
    and ``act_scaling_factor`` are written in place by those calls, and ``running_stat`` is whatever
    the modules say (``fix()`` / ``unfix()``): like the reference's test loop, ``predict`` and
    ``evaluate`` keep updating a running range. Stacks of more than one layer must be per tensor
    (``ValueError`` for ``per_channel=True``: the reference cannot run that either). With
    ``full_precision_flag=True`` the QuantActs stand in front of full-precision stacks (the
    reference's act-only branch). ``micro_step`` / ``apply_micro_steps`` and ``quantize_embedding``
    raise ``NotImplementedError`` on such a model, and its CPU description is not built
    (``device="cpu"`` raises ``NotImplementedError``).

    Not built: momentum, weight
    decay, world size > 1 inside the step (one device can play N ranks: ``micro_step`` /
    ``apply_micro_steps``)."""

    def __init__(self, ln_emb, m_spa, ln_bot, ln_top, sigmoid_top=None, sigmoid_bot=-1,
                 arch_interaction_itself=False, quantize_bits=None, weight_bit=4, embedding_bit=4,
                 per_channel=False, full_precision_flag=False, embedding_full_precision=False,
                 quantize_activation=False, loss_function="bce", loss_weights=None, loss_threshold=0.0,
                 device="cuda", emb_weights=None):
        super().__init__()
        self.quantize_activation = bool(quantize_activation)
        if quantize_activation and torch.device(device).type != "cuda":
            raise NotImplementedError("DQRMNet: the CPU description of a quantize_activation=True model is not "
                                      "built; build it with device='cuda'")
        self.ln_emb = [int(n) for n in np.asarray(ln_emb).reshape(-1)]
        self.m_spa = int(m_spa)
        self.ln_bot = [int(n) for n in np.asarray(ln_bot).reshape(-1)]
        self.ln_top = [int(n) for n in np.asarray(ln_top).reshape(-1)]
        T, D = len(self.ln_emb), self.m_spa
        if T < 1 or len(self.ln_bot) < 2 or len(self.ln_top) < 2:
            raise ValueError("DQRMNet needs at least one table and one layer per MLP")
        if self.ln_bot[-1] != D:
            raise ValueError(f"ln_bot[-1] = {self.ln_bot[-1]} does not match m_spa = {D}: the bottom MLP's output "
                             "is a feature vector beside the embeddings")
        want = D + (T + 1) * T // 2 + (T + 1 if arch_interaction_itself else 0)
        if self.ln_top[0] != want:
            raise ValueError(f"ln_top[0] = {self.ln_top[0]} does not match the interaction's {want} features "
                             f"(m_spa + pairs of {T + 1} vectors, arch_interaction_itself={bool(arch_interaction_itself)})")
        if self.ln_top[-1] != 1:
            raise ValueError(f"ln_top[-1] must be 1 (got {self.ln_top[-1]})")
        if len(self.ln_bot) + len(self.ln_top) - 2 > L.DQRM_MLP_MAX_LAYERS:
            raise ValueError(f"DQRMNet takes at most {L.DQRM_MLP_MAX_LAYERS} MLP layers in all")
        self.embedding_bit = int(embedding_bit)
        self.embedding_full_precision = bool(embedding_full_precision)
        dev = torch.device(device)
        if emb_weights is None:  # q_m_n_q_g.py:273-275, table after table
            emb_weights = [torch.from_numpy(np.random.uniform(low=-np.sqrt(1 / n), high=np.sqrt(1 / n),
                                                              size=(n, D)).astype(np.float32)) for n in self.ln_emb]
        elif len(emb_weights) != T:
            raise ValueError("emb_weights needs one tensor per table")
        if sigmoid_top is None:
            sigmoid_top = len(self.ln_top) - 2
        if quantize_activation:
            if per_channel and not full_precision_flag and max(len(self.ln_bot), len(self.ln_top)) > 2:
                raise ValueError("DQRMNet(quantize_activation=True): stacks of more than one layer must quantize "
                                 "per tensor (per_channel=False): a per-channel correct_output_scale cannot feed the "
                                 "next layer, in the reference either")
            # dlrm_s_pytorch_tb_dp_one_parallel_comm.py:475-476, under the reference's attribute names
            abit = weight_bit if weight_bit >= 8 else 8
            self.quant_input = QuantAct(activation_bit=abit, act_range_momentum=-1)
            self.quant_feature_outputs = QuantAct(fixed_point_quantization=True, activation_bit=abit,
                                                  act_range_momentum=-1)
        self.bot_l = create_mlp(self.ln_bot, sigmoid_bot, weight_bit=weight_bit, full_precision_flag=full_precision_flag,
                                per_channel=per_channel, quantize_activation=self.quantize_activation)
        self.top_l = create_mlp(self.ln_top, sigmoid_top, weight_bit=weight_bit, full_precision_flag=full_precision_flag,
                                per_channel=per_channel, quantize_activation=self.quantize_activation)
        self.interact = DotInteraction(arch_interaction_itself, quantize_bits)
        self.loss = DLRMLoss(loss_function, loss_weights, loss_threshold)
        self.tables = None
        if dev.type == "cuda":
            self.tables = EmbeddingTableSet(self.ln_emb, D, device=dev, init=None, weights=emb_weights)
            self.register_buffer("emb_weight", self.tables.W, persistent=True)  # the slab itself
            self.bot_l.to(dev)
            self.top_l.to(dev)
            self.interact.to(dev)
            self.loss.to(dev)
            if quantize_activation:
                self.quant_input.to(dev)
                self.quant_feature_outputs.to(dev)
            assert want == out_features(T + 1, D, arch_interaction_itself)
        else:  # a description only: every compute path raises DQRMError
            self.register_buffer("emb_weight", torch.cat([w.float() for w in emb_weights]), persistent=True)
        self.bot_stack = MLPStack(self.bot_l)
        self.top_stack = MLPStack(self.top_l)
        self.emb_out = None    # forward(): the embedding slab [B, T, D], a leaf whose .grad is demb
        self.z = None          # train_step(): the clamped prediction [B, 1]
        self.emb_grad = None   # train_step(update=False): demb [B, T, D], a view of the workspace
        self.quantize_emb = False  # quantize_embedding(): predict / evaluate read emb_q
        self.quantize_bits = None  #   its bits, 4 or 8 (the interaction's are interact.quantize_bits)
        self.emb_q = None          #   the RowwiseTableSet
        self.emb_scaling_factor = None  # micro_step(): the tables' first-micro-step grad scales [T]
        d = self.__dict__      # plain attributes of the step (nn.Module.__setattr__ is slow per call)
        d["_ws_q"] = None      # (tensor, B): the row-wise forward's workspace, its own high-water mark
        d["_lay_q"] = None     # (L.Model, B, L.ModelLayout)
        d["_ws"] = None        # (tensor, B, max_lookups): the workspace's high-water mark
        d["_cm"] = None        # (key, L.Model, what it points into)
        d["_out"] = None       # (B, z, g)
        d["_grads"] = None     # (ptr key, dw array, db array)
        d["_lay"] = None       # (L.Model, B, max_lookups, L.ModelLayout)
        d["_last_flags"] = 0   # the DQRM_MODEL_* flags of the latest train_step
        d["_prefetched"] = None  # (batch object, tables.write_epoch, B)
        d["_sim_emb"] = None     # micro_step(): the tables' _MicroStepBuffer
        d["_sim_dense"] = None   #   and the stacks' SimulatedDenseBuffers
        d["_cq"] = None          # quantize_activation: (key, L.ModelQAct, what it points into)

    # ------------------------------------------------------------ bookkeeping
    def _device(self, what):
        if self.tables is None and self.emb_q is not None:  # quantize_embedding(keep_fp32=False)
            if self.emb_packed.data_ptr() != self.emb_q.packed.data_ptr():
                raise L.DQRMError("DQRMNet was moved or cast after quantize_embedding: its packed tables live "
                                  "in the RowwiseTableSet's slab")
            return self.emb_packed.device
        dev = self.emb_weight.device
        if self.tables is None or dev.type != "cuda":
            raise _no_cpu(what, dev)
        if self.emb_weight.data_ptr() != self.tables.W.data_ptr():
            raise L.DQRMError("DQRMNet was moved or cast after construction: its tables live in the "
                              "EmbeddingTableSet's slab; build the model with device=...")
        return dev

    def invalidate(self):
        """Forget what the model derived from its parameters: both stacks quantize again at the
        next forward, and a prefetched embedding forward is discarded. Needed only after a write
        torch cannot see (``p.data.add_()``, a kernel of your own on the tables)."""
        self.bot_stack.invalidate()
        self.top_stack.invalidate()
        self.__dict__["_prefetched"] = None

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        if self.tables is not None:
            self._device("load_state_dict")
            self.tables.refresh_absmax()  # W changed outside the kernels: rebuild the |W| hierarchy
            if self.emb_q is not None:    # ... and the packed rows derived from it
                self.emb_q = RowwiseTableSet.from_tables(self.tables, self.quantize_bits)
        elif self.emb_q is not None:
            self._device("load_state_dict")
        self.invalidate()
        return out

    def _fwd_flags(self):
        return L.DQRM_FWD_REFRESH_SCALE | (L.DQRM_FWD_FULL_PRECISION if self.embedding_full_precision else 0)

    def _check_inputs(self, dense_x, batch, labels, what):
        dev = self._device(what)
        if not isinstance(batch, LookupBatch):
            raise TypeError(f"DQRMNet.{what} takes a LookupBatch")
        if batch.num_tables != len(self.ln_emb):
            raise ValueError("batch has %d tables, set has %d" % (batch.num_tables, len(self.ln_emb)))
        B = batch.num_bags
        if (not isinstance(dense_x, torch.Tensor) or dense_x.dtype != torch.float32 or dense_x.device != dev
                or tuple(dense_x.shape) != (B, self.ln_bot[0]) or not dense_x.is_contiguous()):
            raise ValueError(f"DQRMNet.{what} needs a contiguous float32 [{B}, {self.ln_bot[0]}] dense_x on {dev}")
        if batch.idx.device != dev:
            raise ValueError(f"batch on {batch.idx.device} but the model on {dev}")
        if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != torch.float32
                                   or labels.device != dev or labels.numel() != B or not labels.is_contiguous()):
            raise ValueError(f"DQRMNet.{what} needs contiguous float32 labels of {B} elements on {dev}")
        if not 1 <= B <= L.DQRM_LOSS_MAX_BATCH:
            raise ValueError(f"DQRMNet.{what} takes 1..{L.DQRM_LOSS_MAX_BATCH} samples (got {B})")
        return dev, B

    def _c_model(self, kb, kt):
        """The dqrm_model over the stages' current C structs (rebuilt when any of them moved)."""
        cb, ct = self.bot_stack._c_struct(kb), self.top_stack._c_struct(kt)
        loss = self.loss
        w = loss.loss_ws
        tc = None if self.tables is None else self.tables.c  # released: dqrm_model_fwd_rowwise reads no tables
        key = (id(cb), id(ct), id(tc), loss.loss_function, loss.loss_threshold,
               None if w is None else w.data_ptr(), self.interact.arch_interaction_itself, self.interact._bits,
               self.embedding_bit, self.embedding_full_precision)
        ent = self.__dict__["_cm"]
        if ent is not None and ent[0] == key:
            return ent[1]
        lc = loss._config()
        m = L.Model()
        m.bottom, m.top, m.loss = C.pointer(cb), C.pointer(ct), C.pointer(lc)
        if tc is not None:
            m.tables = C.pointer(tc)
        m.interact.num_features, m.interact.dim = len(self.ln_emb) + 1, self.m_spa
        m.interact.self_interaction = int(self.interact.arch_interaction_itself)
        m.interact.quant_bits = self.interact._bits
        m.embedding_bit, m.emb_fwd_flags = self.embedding_bit, self._fwd_flags()
        m.ste, m.repack_bits = int(not self.embedding_full_precision), 0
        self.__dict__["_cm"] = (key, m, (cb, ct, lc, tc))
        return m

    def _c_qact(self, dev):
        """The dqrm_model_qact beside the model struct: the two QuantActs over their own buffers
        (x_min, x_max and act_scaling_factor are written in place) and one persistent
        correct_output_scale per layer, bound as the layers' buffer."""
        qs = (self.quant_input, self.quant_feature_outputs)
        layers = self.bot_stack.layers + self.top_stack.layers
        for q in qs:
            if q.full_precision_flag or q.quant_mode != "symmetric" or q.act_percentile != 0:
                raise NotImplementedError("DQRMNet: the one-call paths run symmetric QuantActs with "
                                          "full_precision_flag=False and act_percentile=0")
            for name in ("x_min", "x_max", "act_scaling_factor"):
                t = getattr(q, name)
                if t.device != dev or t.dtype != torch.float32 or t.numel() != 1:
                    raise ValueError(f"QuantAct.{name} must be one float32 on the model's device {dev}")
        integer = self.bot_stack._qact  # False: QuantActs in front of full-precision stacks
        if integer:
            for l in layers:  # [1, O] / [1, 1], as the layer's own forward leaves the buffer
                n = l.out_features if l.per_channel else 1
                t = l.correct_output_scale
                if tuple(t.shape) != (1, n) or t.device != dev or t.dtype != torch.float32:
                    l._buffers["correct_output_scale"] = torch.ones((1, n), dtype=torch.float32, device=dev)
        key = tuple((q.x_min.data_ptr(), q.x_max.data_ptr(), q.act_scaling_factor.data_ptr(), int(q.activation_bit),
                     bool(q.running_stat), float(q.act_range_momentum)) for q in qs) \
            + (tuple(l.correct_output_scale.data_ptr() for l in layers) if integer else ())
        ent = self.__dict__["_cq"]
        if ent is not None and ent[0] == key:
            return ent[1]
        cs = []
        for q in qs:
            c = L.ActQuant()
            c.activation_bit = int(q.activation_bit)
            c.running_stat = int(bool(q.running_stat))
            c.momentum = float(q.act_range_momentum)
            c.one_minus_momentum = 1.0 - float(q.act_range_momentum)  # as QuantAct._run rounds it
            c.x_min, c.x_max, c.scale = q.x_min.data_ptr(), q.x_max.data_ptr(), q.act_scaling_factor.data_ptr()
            cs.append(c)
        qa = L.ModelQAct()
        qa.quant_input, qa.quant_features = C.pointer(cs[0]), C.pointer(cs[1])
        arr = None
        if integer:
            arr = (C.c_void_p * len(layers))(*[l.correct_output_scale.data_ptr() for l in layers])
            qa.out_scale = arr
        self.__dict__["_cq"] = (key, qa, (cs, arr))
        return qa

    def _qa_only(self, what):
        if self.quantize_activation:
            raise NotImplementedError(f"DQRMNet.{what} is not built for a quantize_activation=True model")

    def _prepare(self, what):
        """The stacks' checks, their keys and the model struct."""
        if self.loss.loss_function == "wbce" and self.loss.loss_ws.device != self._device(what):
            raise ValueError("DLRMLoss.loss_ws is not on the model's device")
        self.bot_stack._prepare()
        self.top_stack._prepare()
        kb, kt = self.bot_stack._key(), self.top_stack._key()
        return kb, kt, self._c_model(kb, kt)

    def _workspace(self, m, B, max_lookups, dev, keep=0):
        """One device buffer per (B, max_lookups) high-water mark; a smaller batch is cut from the
        same buffer. A new buffer takes over the first `keep` bytes of the old one (a prefetched
        slab, which sits at offset 0 of every cut); without them it holds no prefetched forward."""
        ent = self.__dict__["_ws"]
        if ent is not None and ent[1] >= B and ent[2] >= max_lookups and ent[0].device == dev:
            return ent[0]
        hb = max(B, ent[1]) if ent is not None else B
        hl = max(max_lookups, ent[2]) if ent is not None else max_lookups
        if self.quantize_activation:
            need = self.tables.lib.dqrm_model_qact_workspace_bytes(C.byref(m), C.byref(self._c_qact(dev)), hb, hl)
        else:
            need = self.tables.lib.dqrm_model_workspace_bytes(C.byref(m), hb, hl)
        if need == 0:
            L.check(L.DQRM_E_INVALID, "dqrm_model_workspace_bytes")
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        if keep and ent is not None and ent[0].device == dev:
            ws[:keep].copy_(ent[0][:keep])
        else:
            self.__dict__["_prefetched"] = None
        self.__dict__["_ws"] = (ws, hb, hl)
        self.emb_grad = None
        return ws

    def _layout(self, m, B, max_lookups):
        ent = self.__dict__["_lay"]
        if ent is not None and ent[0] is m and ent[1] == B and ent[2] == max_lookups:
            return ent[3]
        lay = L.ModelLayout()
        # the quantize_activation cut starts with this one, at the same offsets
        L.check(self.tables.lib.dqrm_model_workspace_layout(C.byref(m), B, max_lookups, C.byref(lay)),
                "dqrm_model_workspace_layout")
        self.__dict__["_lay"] = (m, B, max_lookups, lay)
        return lay

    def _view(self, ws, m, B, max_lookups, name):
        """A part of the workspace as a float32 tensor: slab / demb [B, T, D], r / dr [B, R],
        dx [B, D], p [B, 1]."""
        T, D = self.tables.T, self.tables.D
        shape = {"slab": (B, T, D), "demb": (B, T, D), "r": (B, self.ln_top[0]), "dr": (B, self.ln_top[0]),
                 "dx": (B, D), "p": (B, 1)}[name]
        off = getattr(self._layout(m, B, max_lookups), name)
        n = 4 * int(np.prod(shape))
        return ws[off: off + n].view(torch.float32).view(shape)

    def _outputs(self, B, dev):
        ent = self.__dict__["_out"]
        if ent is None or ent[0] != B or ent[1].device != dev:
            ent = (B, torch.empty((B, 1), dtype=torch.float32, device=dev),
                   torch.empty(B, dtype=torch.float32, device=dev))
            self.__dict__["_out"] = ent
        return ent[1], ent[2]

    def _grad_arrays(self):
        """Persistent gradient tensors bound as the parameters' ``.grad``, and the two host arrays
        of their device pointers (bottom's layers, then top's)."""
        layers = self.bot_stack.layers + self.top_stack.layers
        ptrs = []
        for l in layers:
            for p in (l.weight, l.bias):
                g = p.grad
                if (g is None or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape
                        or not g.is_contiguous()):
                    g = p.grad = torch.zeros_like(p)
                ptrs.append(g.data_ptr())
        key = tuple(ptrs)
        ent = self.__dict__["_grads"]
        if ent is None or ent[0] != key:
            A = C.c_void_p * len(layers)
            ent = (key, A(*ptrs[0::2]), A(*ptrs[1::2]))
            self.__dict__["_grads"] = ent
        return ent[1], ent[2]

    def _poll(self):
        if error_check_due(self) and not torch.cuda.is_current_stream_capturing():
            poll_device_errors(self.tables if self.emb_q is None else self.emb_q)

    def _not_quantized(self, what):
        if self.emb_q is not None:
            raise RuntimeError(f"DQRMNet.{what}: the model serves row-wise quantized tables after "
                               "quantize_embedding() and cannot train (the reference's emb_l is None there); "
                               "call dequantize_embedding() first (quantize_embedding(keep_fp32=True) allows it)")

    # ------------------------------------------------------------ quantized serving
    def quantize_embedding(self, bits, keep_fp32=True):
        """The reference's ``DLRM_Net.quantize_embedding(bits)`` (:683-700): every table prepacked
        row-wise to 4- or 8-bit rows by one launch over the slab; ``predict`` / ``evaluate`` then
        gather from ``model.emb_q``. Any other ``bits`` raises ``ValueError`` (the reference prints
        nothing and returns). keep_fp32=False releases the FP32 tables (see the class docstring).
        Calling it again on a model that kept its FP32 tables repacks them with the new bits."""
        self._qa_only("quantize_embedding")
        if isinstance(bits, bool) or bits not in (4, 8):
            raise ValueError(f"DQRMNet.quantize_embedding: bits must be 4 or 8, got {bits!r}")
        if self.tables is None and self.emb_q is not None:
            raise L.DQRMError("DQRMNet.quantize_embedding: the FP32 tables were released "
                              "(quantize_embedding(keep_fp32=False)); there is nothing to pack again")
        self._device("quantize_embedding")
        q = RowwiseTableSet.from_tables(self.tables, int(bits))
        self.emb_q, self.quantize_emb, self.quantize_bits = q, True, int(bits)
        d = self.__dict__
        d["_ws_q"] = d["_lay_q"] = None
        if keep_fp32:  # the training workspace and its prefetch record stay as they are
            return
        del self.emb_weight
        self.register_buffer("emb_packed", q.packed, persistent=True)  # the packed slab itself
        self.tables = None
        self.emb_out = self.emb_grad = None
        d["_ws"] = d["_cm"] = d["_lay"] = d["_prefetched"] = None

    def dequantize_embedding(self):
        """Drop the packed tables of ``quantize_embedding(bits, keep_fp32=True)``: every path reads
        the FP32 tables again, which were never modified."""
        if self.emb_q is None:
            return
        if self.tables is None:
            raise L.DQRMError("DQRMNet.dequantize_embedding: the FP32 tables were released "
                              "(quantize_embedding(keep_fp32=False))")
        self.emb_q, self.quantize_emb, self.quantize_bits = None, False, None
        self.__dict__["_ws_q"] = self.__dict__["_lay_q"] = None

    def _workspace_q(self, m, B, dev):
        """The row-wise forward's own buffer (a forward-only cut), grown to the largest B seen."""
        ent = self.__dict__["_ws_q"]
        if ent is not None and ent[1] >= B and ent[0].device == dev:
            return ent[0]
        need = self.emb_q.lib.dqrm_model_fwd_rowwise_workspace_bytes(C.byref(m), C.byref(self.emb_q.c), B)
        if need == 0:
            L.check(L.DQRM_E_INVALID, "dqrm_model_fwd_rowwise_workspace_bytes")
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        self.__dict__["_ws_q"] = (ws, B)
        return ws

    def _predict_q(self, dense_x, batch, labels, dev, B):
        kb, kt, m = self._prepare("predict")
        fresh = self.bot_stack.is_fresh(kb) and self.top_stack.is_fresh(kt)
        q = self.emb_q
        ws = self._workspace_q(m, B, dev)
        self._poll()
        loss = z = None
        if labels is not None:
            loss = torch.empty((), dtype=torch.float32, device=dev)
            z = torch.empty((B, 1), dtype=torch.float32, device=dev)
        L.check(q.lib.dqrm_model_fwd_rowwise(
            C.byref(m), C.byref(q.c), C.byref(batch.c), L.DQRM_MODEL_MLP_FRESH if fresh else 0, dense_x.data_ptr(),
            None if labels is None else labels.data_ptr(), None if loss is None else loss.data_ptr(),
            None if z is None else z.data_ptr(), ws.data_ptr(), ws.numel(), _stream_handle()),
            "dqrm_model_fwd_rowwise")
        if labels is not None:
            return loss, z
        ent = self.__dict__["_lay_q"]
        if ent is None or ent[0] is not m or ent[1] != B:
            lay = L.ModelLayout()
            L.check(q.lib.dqrm_model_fwd_rowwise_workspace_layout(C.byref(m), C.byref(q.c), B, C.byref(lay)),
                    "dqrm_model_fwd_rowwise_workspace_layout")
            ent = self.__dict__["_lay_q"] = (m, B, lay)
        return ws[ent[2].p: ent[2].p + 4 * B].view(torch.float32).view(B, 1).clone()

    def fwd_rowwise_launches(self, batch, labels=False, fresh=None):
        """dqrm_model_fwd_rowwise_launches for a ``predict`` of the quantized model (fresh None: the
        stacks' current state)."""
        self._device("fwd_rowwise_launches")
        if self.emb_q is None:
            raise RuntimeError("DQRMNet.fwd_rowwise_launches: call quantize_embedding() first")
        kb, kt, m = self._prepare("fwd_rowwise_launches")
        if fresh is None:
            fresh = self.bot_stack.is_fresh(kb) and self.top_stack.is_fresh(kt)
        n = self.emb_q.lib.dqrm_model_fwd_rowwise_launches(C.byref(m), C.byref(self.emb_q.c), C.byref(batch.c),
                                                           L.DQRM_MODEL_MLP_FRESH if fresh else 0, int(bool(labels)))
        if n < 0:
            L.check(n, "dqrm_model_fwd_rowwise_launches")
        return n

    # ------------------------------------------------------------ the composition
    def forward(self, dense_x, batch):
        """p ``[B, 1]``: the bottom stack, the tables' fused forward, the interaction and the top
        stack as autograd nodes. ``model.emb_out`` is the embedding slab ``[B, T, D]``, a leaf: after
        ``backward()`` its ``.grad`` is what ``model.tables.backward_sgd(batch, grad, lr,
        layout="btd")`` takes; the stacks are updated with ``sgd_step``."""
        self._not_quantized("forward")
        self._device("forward")
        qa = self.quantize_activation
        integer = qa and self.bot_stack._qact  # False: QuantActs in front of full-precision stacks
        if qa:
            dense_x, s_in = self.quant_input(dense_x)
        x = self.bot_stack(dense_x, s_in)[0] if integer else self.bot_stack(dense_x)
        slab = self.tables.forward(batch, bits=self.embedding_bit, refresh_scale=True,
                                   full_precision=self.embedding_full_precision, layout="btd")
        if torch.is_grad_enabled():
            slab.requires_grad_(True)
        self.emb_out = slab
        r = self.interact(x, slab)
        if qa:
            r, s_feat = self.quant_feature_outputs(r)
        return self.top_stack(r, s_feat)[0] if integer else self.top_stack(r)

    # ------------------------------------------------------------ one host call
    def predict(self, dense_x, batch, labels=None):
        """The forward as ONE host call (dqrm_model_fwd): p ``[B, 1]`` without labels, ``(E, Z)``
        with them: the 0-dim loss and the clamped prediction. Quantizes the MLP weights only when
        the stacks are not fresh (``requantize()`` makes them so). After ``quantize_embedding`` the
        same, from the row-wise packed tables (dqrm_model_fwd_rowwise)."""
        dev, B = self._check_inputs(dense_x, batch, labels, "predict")
        return _on_device(dev, self._predict if self.emb_q is None else self._predict_q, dense_x, batch, labels,
                          dev, B)

    def _predict(self, dense_x, batch, labels, dev, B):
        kb, kt, m = self._prepare("predict")
        fresh = self.bot_stack.is_fresh(kb) and self.top_stack.is_fresh(kt)
        ws = self._workspace(m, B, batch.max_lookups, dev)
        self.__dict__["_prefetched"] = None  # the slab is overwritten
        self._poll()
        loss = z = None
        if labels is not None:
            loss = torch.empty((), dtype=torch.float32, device=dev)
            z = torch.empty((B, 1), dtype=torch.float32, device=dev)
        tail = (C.byref(batch.c), L.DQRM_MODEL_MLP_FRESH if fresh else 0, dense_x.data_ptr(),
                None if labels is None else labels.data_ptr(), None if loss is None else loss.data_ptr(),
                None if z is None else z.data_ptr(), ws.data_ptr(), ws.numel(), _stream_handle())
        if self.quantize_activation:
            L.check(self.tables.lib.dqrm_model_fwd_qact(C.byref(m), C.byref(self._c_qact(dev)), *tail),
                    "dqrm_model_fwd_qact")
        else:
            L.check(self.tables.lib.dqrm_model_fwd(C.byref(m), *tail), "dqrm_model_fwd")
        if labels is not None:
            return loss, z
        return self._view(ws, m, B, batch.max_lookups, "p").clone()

    def evaluate(self, batches, metrics=None, max_batches=-1):
        """The reference's test loop (``inference()``, :1304-1404) with every score left on the
        device: per batch dqrm_model_fwd with the labels, whose clamped prediction Z goes straight
        into ``DLRMMetrics.update`` (no clone, no sync), then ``compute()``'s dict: ``n``, ``n_pos``,
        ``n_correct``, ``test_acc`` and the exact ``roc_auc``.

        batches: an iterable of ``(dense_x, LookupBatch, labels)``; max_batches > 0 stops after that
        many (the reference's ``nbatches``, :1327). metrics: a ``DLRMMetrics`` to use (it is reset), or
        None: one is made for ``len(batches)`` times the first batch's size, so ``batches`` must then
        have a ``len`` and no later batch may be larger. Both stacks are requantized once
        beforehand if they are not fresh, which changes no bits and saves the per-batch weight
        quantization. A prefetched embedding forward is discarded, as by ``predict``. Every rank of a
        larger world evaluates what it is given."""
        from .metrics import DLRMMetrics

        if metrics is not None and not isinstance(metrics, DLRMMetrics):
            raise TypeError("DQRMNet.evaluate: metrics must be a DLRMMetrics (or None)")
        max_batches = int(max_batches)
        if metrics is None:
            try:
                nb = len(batches)
            except TypeError:
                raise ValueError("DQRMNet.evaluate: batches has no len(), so the metrics cannot be sized: pass "
                                 "metrics=DLRMMetrics(capacity)") from None
            if max_batches > 0:
                nb = min(nb, max_batches)
        dev = self._device("evaluate")
        if metrics is not None:
            if metrics.device != dev:
                raise ValueError(f"DQRMNet.evaluate: metrics on {metrics.device} but the model on {dev}")
            metrics.reset()
        kb, kt, _ = self._prepare("evaluate")
        if not (self.bot_stack.is_fresh(kb) and self.top_stack.is_fresh(kt)):
            self.requantize()
        seen = 0
        for k, item in enumerate(batches):
            if 0 < max_batches <= k:
                break
            dense_x, batch, labels = item
            if labels is None:
                raise ValueError("DQRMNet.evaluate: every batch needs its labels")
            dev, B = self._check_inputs(dense_x, batch, labels, "evaluate")
            if metrics is None:
                metrics = DLRMMetrics(max(nb, 1) * B, device=dev)
            _, Z = _on_device(dev, self._predict if self.emb_q is None else self._predict_q, dense_x, batch,
                              labels, dev, B)
            metrics.update(Z, labels)
            seen += 1
        if seen == 0:
            raise ValueError("DQRMNet.evaluate: no batch given")
        out = metrics.compute()
        if self.emb_q is not None:  # compute() has synchronised: one read of the packed set's flags
            raise_device_errors(self.emb_q.read_errors(clear=True))
        return out

    def requantize(self):
        """Quantize both stacks' weights now and mark them fresh (``MLPStack.requantize``)."""
        self._device("requantize")
        self.bot_stack.requantize()
        self.top_stack.requantize()

    def step_launches(self, batch, next_batch=None, update=True, prefetched=False, fresh=None):
        """dqrm_model_step_launches for a ``train_step`` with these arguments (fresh None: the
        stacks' current state)."""
        self._not_quantized("step_launches")
        self._device("step_launches")
        kb, kt, m = self._prepare("step_launches")
        if fresh is None:
            fresh = self.bot_stack.is_fresh() and self.top_stack.is_fresh()
        flags = (L.DQRM_MODEL_MLP_FRESH if fresh else 0) | (L.DQRM_MODEL_REQUANT if update else L.DQRM_MODEL_NO_UPDATE) \
            | (L.DQRM_MODEL_EMB_READY if prefetched else 0)
        nb = None if next_batch is None else C.byref(next_batch.c)
        if self.quantize_activation:
            qa = self._c_qact(self._device("step_launches"))
            n = self.tables.lib.dqrm_model_qact_step_launches(C.byref(m), C.byref(qa), C.byref(batch.c), nb, flags)
        else:
            n = self.tables.lib.dqrm_model_step_launches(C.byref(m), C.byref(batch.c), nb, flags)
        if n < 0:
            L.check(n, "dqrm_model_step_launches")
        return n

    def train_step(self, dense_x, batch, labels, lr, next_batch=None, update=True):
        """One training step as ONE host call (dqrm_model_step); returns the 0-dim loss tensor.
        ``model.z`` then holds the clamped prediction ``[B, 1]`` (overwritten by the next step).

        update=True: SGD with ``lr`` on the tables (dqrm_emb_bwd_sgd) and on both MLP stacks, which
        are requantized in the same launch and are fresh afterwards. next_batch: the batch of the
        following step; its embedding forward is left in the workspace (see the class docstring).
        update=False: the step stops after the backward; no parameter, table, scale or integer
        buffer is written, ``p.grad`` of every MLP parameter holds its gradient and
        ``model.emb_grad`` (set by every step) is the ``[B, T, D]`` gradient of the embedding slab (a
        view of the workspace, valid until the next call): the route for world size > 1, where the DP hooks
        take it from there. ``next_batch`` needs update=True.

        The MLP gradients are written into persistent tensors bound as ``p.grad`` (overwritten,
        not accumulated)."""
        self._not_quantized("train_step")
        dev, B = self._check_inputs(dense_x, batch, labels, "train_step")
        if next_batch is not None:
            if not update:
                raise ValueError("DQRMNet.train_step: next_batch needs update=True")
            if not isinstance(next_batch, LookupBatch) or next_batch.num_tables != self.tables.T:
                raise ValueError("DQRMNet.train_step: next_batch must be a LookupBatch of the model's tables")
            if next_batch.num_bags != B or next_batch.idx.device != dev:
                raise ValueError(f"DQRMNet.train_step: next_batch has {next_batch.num_bags} bags, batch {B} "
                                 "(the prefetched forward shares the slab)")
        return _on_device(dev, self._train_step, dense_x, batch, labels, float(lr), next_batch, bool(update), dev, B)

    def _train_step(self, dense_x, batch, labels, lr, next_batch, update, dev, B):
        bot, top, tables = self.bot_stack, self.top_stack, self.tables
        kb, kt, m = self._prepare("train_step")
        fresh = bot.is_fresh(kb) and top.is_fresh(kt)
        pf = self.__dict__["_prefetched"]
        ready = pf is not None and pf[0] is batch and pf[1] == tables.write_epoch and pf[2] == B
        # sized for the next batch too, so that its step finds its slab where this one leaves it
        ml = batch.max_lookups if next_batch is None else max(batch.max_lookups, next_batch.max_lookups)
        ws = self._workspace(m, B, ml, dev, keep=4 * B * tables.T * tables.D if ready else 0)
        self.__dict__["_prefetched"] = None
        flags = (L.DQRM_MODEL_MLP_FRESH if fresh else 0) | (L.DQRM_MODEL_EMB_READY if ready else 0) \
            | (L.DQRM_MODEL_REQUANT if update else L.DQRM_MODEL_NO_UPDATE)
        self.__dict__["_last_flags"] = flags
        z, g = self._outputs(B, dev)
        dw, db = self._grad_arrays()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        self._poll()
        if update:  # whatever happens from here on, the integers are no longer known to be current
            bot._fresh = top._fresh = None
        tail = (C.byref(batch.c), None if next_batch is None else C.byref(next_batch.c), flags,
                dense_x.data_ptr(), labels.data_ptr(), lr, loss.data_ptr(), z.data_ptr(), g.data_ptr(), dw, db,
                ws.data_ptr(), ws.numel(), _stream_handle())
        if self.quantize_activation:
            L.check(tables.lib.dqrm_model_step_qact(C.byref(m), C.byref(self._c_qact(dev)), *tail),
                    "dqrm_model_step_qact")
        else:
            L.check(tables.lib.dqrm_model_step(C.byref(m), *tail), "dqrm_model_step")
        self.__dict__["z"] = z
        self.__dict__["emb_grad"] = self._view(ws, m, B, batch.max_lookups, "demb")
        if not update:
            return loss
        tables.write_epoch += 1
        for l in bot.layers + top.layers:  # the kernel wrote them: what autograd saved of them is stale
            torch.autograd.graph.increment_version(l.weight)
            torch.autograd.graph.increment_version(l.bias)
        bot._fresh, top._fresh = bot._state(kb), top._state(kt)
        if next_batch is not None:
            self.__dict__["_prefetched"] = (next_batch, tables.write_epoch, B)
        return loss

    # ------------------------------------------------------------ simulated data parallelism
    def micro_step(self, dense_x, batch, labels, number_of_gpus):
        """One of the N micro-steps with which one device plays N ranks (the reference's
        pseudo-multigpu driver with ``sgd_quantized_gradients``); returns the 0-dim loss tensor.

        ``train_step(update=False)``, then this micro-step's gradients go into the INT8 buffers:
        the embedding gradient (``model.emb_grad``) is coalesced and quantize-packed with the
        first micro-step's max|grad| as the scale (``model.emb_scaling_factor`` ``[T]``), as
        ``grad_buffer_update_added_quantization`` does for the modules, and the gradients of both
        stacks' layers take ONE error-compensated accumulate (dqrm_dense_ec_accumulate; the layers'
        ``weight_scaling_factor``, ``error_compensation_weight``, ``weight_grad_buffer`` and the
        bias's hold the state). No parameter or table is written. ``apply_micro_steps`` applies
        and empties the buffers."""
        self._qa_only("micro_step")
        self._not_quantized("micro_step")
        n = int(number_of_gpus)
        if n < 1:
            raise ValueError(f"DQRMNet.micro_step: number_of_gpus must be >= 1 (got {number_of_gpus})")
        loss = self.train_step(dense_x, batch, labels, 0.0, update=False)
        _on_device(self._device("micro_step"), self._micro_step, batch)
        return loss

    def _sim_buffers(self):
        sb = self.__dict__.get("_sim_dense")
        if sb is None:
            sb = self.__dict__["_sim_dense"] = SimulatedDenseBuffers(self.bot_stack.layers + self.top_stack.layers,
                                                                     grad_bits=GRAD_BITS)
        return sb

    def _micro_step(self, batch):
        buf = _MicroStepBuffer.fitting(self.__dict__.get("_sim_emb"), self.tables, batch.max_lookups)
        self.__dict__["_sim_emb"] = buf
        buf.accumulate(batch, self.emb_grad, not self.embedding_full_precision, "btd")
        self.__dict__["emb_scaling_factor"] = buf.s_first
        self._sim_buffers().accumulate()

    def apply_micro_steps(self, lr, number_of_gpus, requantize=True):
        """The update after ``number_of_gpus`` micro-steps (``weights_update_added_quantization``
        then ``grad_buffer_zeroing``): the tables take W += -lr * (buffer * (s / N))
        (dqrm_apply_sparse_update, DQRM_UPD_SIMULATED), every MLP parameter
        p += -lr * (buffer * (s[c] / N)) in ONE launch (dqrm_dense_sim_update), and both buffers
        and their scales are zeroed (the MLP's error compensation carries into the next window).
        Raises ``ValueError`` unless exactly ``number_of_gpus`` micro-steps were accumulated. The
        stacks are stale afterwards; requantize=True (default) calls ``requantize()``, so that the
        next window's forwards skip the weight quantization."""
        self._qa_only("apply_micro_steps")
        self._not_quantized("apply_micro_steps")
        dev = self._device("apply_micro_steps")
        buf = self.__dict__.get("_sim_emb")
        if buf is None or len(buf.payloads) != int(number_of_gpus):
            raise ValueError(f"{0 if buf is None else len(buf.payloads)} micro-steps accumulated but "
                             f"num_gpus={number_of_gpus}")
        _on_device(dev, self._apply_micro_steps, buf, float(lr), int(number_of_gpus), bool(requantize))

    def _apply_micro_steps(self, buf, lr, n, requantize):
        sb = self._sim_buffers()
        self.bot_stack._fresh = self.top_stack._fresh = None
        self.__dict__["_prefetched"] = None
        self.tables.write_epoch += 1
        buf.apply(lr, n, False)
        sb.update(lr, n)
        buf.zero()
        buf.s_first.zero_()
        sb.zero()
        if requantize:
            self.requantize()


__all__ = ["DQRMNet"]
