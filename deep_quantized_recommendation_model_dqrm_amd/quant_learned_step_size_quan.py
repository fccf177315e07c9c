"""Drop-in for the reference's ``quantization_supp/quant_learned_step_size_quan.py`` embedding
module (``--quant-mode lsq``), backed by libdqrm's HIP kernels (no CPU fallback).

``QuantEmbeddingBagLSQ`` keeps the reference's constructor order and forward signature
(quant_learned_step_size_quan.py:65-100) and its state-dict keys (``embedding_bag.weight``,
``quan_w_fn.s``, ``quan_a_fn.s``). Its forward quantizes the POOLED EmbeddingBag output with one
learned step size (quantizer/lsq.py:47-58): with lo = -2^(bit-1), hi = 2^(bit-1)-1, n = B*D and
g = 1/sqrt(hi*n),

    s_eff = (s - s*g) + s*g;  q = x / s_eff;  y = round(clamp(q, lo, hi)) * s_eff

and its backward is autograd's of that composition: the clamp's mask on the row gradient, and
``quan_w_fn.s.grad`` (dense, for torch.optim.SGD) from a deterministic fixed-shape reduction
(include/dqrm.h, dqrm_emb_bwd_lsq). The row gradient then takes QuantEmbeddingBagTwo's
grad_mode "sparse" or "fused_sgd" path with the identity STE.

``LSQEmbeddingBagCollection`` is the T-table form: one launch per forward for all tables, the
steps one [T] parameter.

Not built: QuantLinearLSQ, QuantConv2dLSQ (they raise NotImplementedError), per-channel steps, and
the all_positive / symmetric thresholds beyond storing them.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from ._baselines import SCOPE, _BaselineEmbedding


class LsqQuan(nn.Module):
    """quantizer/lsq.py:18-45: the thresholds, the learned step ``s`` and its initialisation. The
    quantization itself runs inside the embedding kernels, so calling the module raises."""

    def __init__(self, bit, all_positive=False, symmetric=False, per_channel=True):
        super().__init__()
        self.bit = bit
        if all_positive:
            assert not symmetric, "Positive quantization cannot be symmetric"
            self.thd_neg, self.thd_pos = 0, 2 ** bit - 1
        elif symmetric:
            self.thd_neg, self.thd_pos = -2 ** (bit - 1) + 1, 2 ** (bit - 1) - 1
        else:
            self.thd_neg, self.thd_pos = -2 ** (bit - 1), 2 ** (bit - 1) - 1
        self.all_positive, self.symmetric, self.per_channel = all_positive, symmetric, per_channel
        self.s = nn.Parameter(torch.ones(1))

    def init_from(self, x, *args, **kwargs):
        """s = mean|x| * 2 / sqrt(thd_pos), over all of x or (per_channel) per first-dim slice,
        with torch's ops on x's device."""
        a = x.detach().abs()
        m = a.mean(dim=list(range(1, x.dim())), keepdim=True) if self.per_channel else a.mean()
        self.s = nn.Parameter(m * 2 / (self.thd_pos ** 0.5))

    def forward(self, x):
        raise NotImplementedError("LsqQuan as a stand-alone quantizer: " + SCOPE)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        s = state_dict.get(prefix + "s")  # the reference stores a per-tensor step as a 0-d tensor
        if s is not None and s.dim() == 0 and self.s.numel() == 1:
            state_dict[prefix + "s"] = s.reshape(self.s.shape)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


def _check_bit(bit: int) -> int:
    if not 2 <= int(bit) <= 8:
        raise ValueError("bit must be 2..8 (got %r)" % (bit,))
    return int(bit)


class _LsqFn(torch.autograd.Function):
    """forward = dqrm_emb_fwd_lsq; backward = dqrm_emb_bwd_lsq, then the module's grad_mode."""

    @staticmethod
    def forward(ctx, weight, step, owner, batch, bits, layout):
        one = layout == "bd"  # one table: its [B, D] output itself
        kl = "tbd" if one else layout
        train = any(ctx.needs_input_grad[:2])
        y, pooled = owner._tset.forward_lsq(batch, step, bits=bits, layout=kl, keep_pooled=train)
        if one:
            y = y.view(y.shape[1], y.shape[2])
        if train:
            ctx.save_for_backward(step, pooled)
        ctx.one, ctx.owner, ctx.batch, ctx.bits, ctx.layout = one, owner, batch, bits, kl
        return y

    @staticmethod
    def backward(ctx, dy):
        step, pooled = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.one:
            dy = dy.view(1, dy.shape[0], dy.shape[1])
        dx, dstep = ctx.owner._tset.backward_lsq(ctx.batch, dy, pooled, step, bits=ctx.bits, layout=ctx.layout)
        grad_w = ctx.owner._backward(ctx.batch, dx, False, "tbd")  # dx per lookup: the identity STE
        return grad_w, dstep, None, None, None, None


class QuantEmbeddingBagLSQ(_BaselineEmbedding):
    """quant_learned_step_size_quan.py:65-100, one table, on libdqrm. The driver passes its
    embedding_bit in the third slot (full_precision_flag), which the reference ignores: so does
    this module. bit: 2..8 (the reference's 4 by default)."""

    def __init__(self, num_embeddings, embedding_dim, full_precision_flag=False, embedding_id=None,
                 quan_w_fn=LsqQuan, quan_a_fn=LsqQuan, *, bit: int = 4, device="cuda",
                 weight: torch.Tensor | None = None, init: str = "numpy", grad_mode: str | None = None,
                 lr: float | None = None):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.embedding_id = embedding_id
        self.bit = _check_bit(bit)
        host = self._init_tables([num_embeddings], embedding_dim, device, [weight] if weight is not None else None,
                                 init, grad_mode, lr)
        dev = self._tset.device
        self.quan_w_fn = quan_w_fn(bit=self.bit, all_positive=False, symmetric=False, per_channel=False)
        self.quan_a_fn = quan_a_fn(bit=self.bit, all_positive=False, symmetric=False, per_channel=True)
        # init_from on the host tensor, as the reference does before .to(device)
        self.quan_w_fn.init_from(host[0].detach().to(torch.float32).cpu() if host is not None else self._tset.W.cpu())
        self.quan_w_fn.s = nn.Parameter(self.quan_w_fn.s.detach().reshape(1).to(dev))
        self.quan_a_fn.s = nn.Parameter(self.quan_a_fn.s.detach().to(dev))

    def forward(self, input, offsets=None, full_precision_flag=False, per_sample_weights=None, test_mode=False):
        self._begin_forward(test_mode)
        batch = self._module_batch(input, offsets)
        if full_precision_flag:
            return self._full_precision(batch, "bd")
        return _LsqFn.apply(self.embedding_bag.weight, self.quan_w_fn.s, self, batch, self.bit, "bd")


class LSQEmbeddingBagCollection(_BaselineEmbedding):
    """T LSQ tables in one set: forward(lS_o, lS_i) replaces apply_emb's per-table loop with ONE
    launch; ``quan_w_fn.s`` is one [T] parameter, table t's step initialised from table t."""

    def __init__(self, ln: Sequence[int], m: int, *, bit: int = 4, device="cuda", init: str = "numpy",
                 weights: Sequence[torch.Tensor] | None = None, grad_mode: str | None = None,
                 lr: float | None = None, seed: int = 123):
        super().__init__()
        self.ln = [int(n) for n in ln]
        self.embedding_dim = int(m)
        self.bit = _check_bit(bit)
        host = self._init_tables(self.ln, self.embedding_dim, device, weights, init, grad_mode, lr, seed=seed)
        self.quan_w_fn = LsqQuan(bit=self.bit, all_positive=False, symmetric=False, per_channel=False)
        steps = []
        for t in range(len(self.ln)):
            w = host[t].detach().to(torch.float32).cpu() if host is not None else self._tset.table_weight(t).cpu()
            steps.append(w.abs().mean() * 2 / (self.quan_w_fn.thd_pos ** 0.5))
        self.quan_w_fn.s = nn.Parameter(torch.stack(steps).to(self._tset.device))

    def table_weight(self, t: int) -> torch.Tensor:
        return self._tset.table_weight(t)

    def forward(self, lS_o, lS_i, full_precision_flag=False, test_mode=False, layout="list"):
        """lS_o / lS_i: per-table lists or stacked [T, B] tensors. layout "list" -> list of T
        [B, D] tensors (apply_emb's ly); "btd" -> [B, T, D]."""
        self._begin_forward(test_mode)
        batch = self._collection_batch(lS_o, lS_i)
        kl = "btd" if layout == "btd" else "tbd"
        if full_precision_flag:
            y = self._full_precision(batch, kl)
        else:
            y = _LsqFn.apply(self.embedding_bag.weight, self.quan_w_fn.s, self, batch, self.bit, kl)
        return list(y.unbind(0)) if layout == "list" else y


class QuantLinearLSQ(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("QuantLinearLSQ: " + SCOPE)


class QuantConv2dLSQ(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("QuantConv2dLSQ: " + SCOPE)


__all__ = ["LsqQuan", "QuantEmbeddingBagLSQ", "LSQEmbeddingBagCollection", "QuantLinearLSQ", "QuantConv2dLSQ"]
