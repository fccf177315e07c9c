"""Drop-in for the reference's ``quantization_supp/quant_pact_dorefa.py`` embedding module
(``--quant-mode pact``), backed by libdqrm's HIP kernels (no CPU fallback).

``QuantEmbeddingBagPACT`` keeps the reference's constructor and forward signature
(quant_pact_dorefa.py:57-112). The reference maps the WHOLE table on every forward
(DoReFaQuant, :10-28): tanh over the table, its maximum, a second dense table, then the gather.
tanh is odd and monotone, so max|tanh(W)| = tanh(max|W|), and max|W| per table is what the
table set's |W| hierarchy keeps current: the forward here touches only the gathered rows. With
k = bitwidth, sc = 2^k - 1 and mt = tanh(max|W|), per element of a gathered row

    v = 2 * (round(sc * (tanh(w) / (2*mt) + 0.5)) / sc) - 1

and the output is the bag sum of v. An all-zero table gives NaN, as the reference's 0/0 does.
The backward is the identity STE (:25-28): dy per lookup, through QuantEmbeddingBagTwo's
grad_mode "sparse" or "fused_sgd" path.

``PACTEmbeddingBagCollection`` is the T-table form: one launch per forward for all tables.

Not built: QuantLinearPACT and QuantConv2dPACT (they raise NotImplementedError).
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from ._baselines import SCOPE, _BaselineEmbedding


def _check_bitwidth(bitwidth: int) -> int:
    if not 2 <= int(bitwidth) <= 8:
        raise ValueError("bitwidth must be 2..8 (got %r)" % (bitwidth,))
    return int(bitwidth)


class _PactFn(torch.autograd.Function):
    """forward = dqrm_emb_fwd_pact; backward = the module's grad_mode on dy itself."""

    @staticmethod
    def forward(ctx, weight, owner, batch, bits, layout):
        one = layout == "bd"  # one table: its [B, D] output itself
        kl = "tbd" if one else layout
        y = owner._tset.forward_pact(batch, bits=bits, layout=kl)
        if one:
            y = y.view(y.shape[1], y.shape[2])
        ctx.one, ctx.owner, ctx.batch, ctx.layout = one, owner, batch, kl
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        if ctx.one:
            dy = dy.view(1, dy.shape[0], dy.shape[1])
        return ctx.owner._backward(ctx.batch, dy, False, ctx.layout), None, None, None, None


class QuantEmbeddingBagPACT(_BaselineEmbedding):
    """quant_pact_dorefa.py:57-112, one table, on libdqrm."""

    def __init__(self, num_embeddings, embedding_dim, bitwidth=8, full_precision_flag=False, embedding_id=None, *,
                 device="cuda", weight: torch.Tensor | None = None, init: str = "numpy",
                 grad_mode: str | None = None, lr: float | None = None):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.bitwidth = _check_bitwidth(bitwidth)
        self.full_precision_flag = full_precision_flag
        self.embedding_id = embedding_id
        self.fix_flag = False
        self._init_tables([num_embeddings], embedding_dim, device, [weight] if weight is not None else None, init,
                          grad_mode, lr)

    def __repr__(self):
        return "(" + super().__repr__() + " bitwidth = {}, full_precision_flag = {})".format(
            self.bitwidth, self.full_precision_flag)

    def fix(self):
        self.fix_flag = True

    def unfix(self):
        self.fix_flag = False

    def forward(self, input, offsets=None, per_sample_weights=None, full_precision_flag=False, test_mode=False):
        self._begin_forward(test_mode)
        batch = self._module_batch(input, offsets)
        if full_precision_flag:
            return self._full_precision(batch, "bd")
        return _PactFn.apply(self.embedding_bag.weight, self, batch, self.bitwidth, "bd")


class PACTEmbeddingBagCollection(_BaselineEmbedding):
    """T PACT tables in one set: forward(lS_o, lS_i) replaces apply_emb's per-table loop with ONE
    launch, each table scaled by its own tanh(max|W_t|)."""

    def __init__(self, ln: Sequence[int], m: int, bitwidth: int = 8, *, device="cuda", init: str = "numpy",
                 weights: Sequence[torch.Tensor] | None = None, grad_mode: str | None = None,
                 lr: float | None = None, seed: int = 123):
        super().__init__()
        self.ln = [int(n) for n in ln]
        self.embedding_dim = int(m)
        self.bitwidth = _check_bitwidth(bitwidth)
        self._init_tables(self.ln, self.embedding_dim, device, weights, init, grad_mode, lr, seed=seed)

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
            y = _PactFn.apply(self.embedding_bag.weight, self, batch, self.bitwidth, kl)
        return list(y.unbind(0)) if layout == "list" else y


class QuantLinearPACT(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("QuantLinearPACT: " + SCOPE)


class QuantConv2dPACT(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("QuantConv2dPACT: " + SCOPE)


__all__ = ["QuantEmbeddingBagPACT", "PACTEmbeddingBagCollection", "QuantLinearPACT", "QuantConv2dPACT"]
