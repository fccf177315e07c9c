"""What the LSQ and PACT embedding modules (quant_learned_step_size_quan.py,
quant_pact_dorefa.py) share: a table set built like QuantEmbeddingBagTwo's, the reference's
``embedding_bag.weight`` path, and QuantEmbeddingBagTwo's backward modes ("sparse" with the
presummed COO and the fused optimizer step, "fused_sgd") with the identity STE (ste=False)."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch
from torch import nn

from .quant_modules_not_quantize_grad import (_EmbeddingFn, _QuantEmbeddingBase, _WeightHolder, _batch_from_input,
                                              _pooling_one_arg, _register_sgd_owner)
from .tables import EmbeddingTableSet, LookupBatch

SCOPE = ("only the LSQ / PACT embedding tables run on libdqrm's kernels; the LSQ / PACT MLP and Conv2d "
         "layers are not built")


class _BaselineEmbedding(_QuantEmbeddingBase):
    """One table (a module) or T tables (a collection) in one EmbeddingTableSet."""

    def _init_tables(self, rows: Sequence[int], dim: int, device, weights, init: str, grad_mode, lr,
                     seed: int = 123) -> list[torch.Tensor] | None:
        """Builds self._tset and embedding_bag.weight; returns the host weights it was built from
        (None for init="uniform", whose rows exist on the device only)."""
        self._init_common(grad_mode, lr, 0, False)
        if self.grad_mode == "dp":
            raise NotImplementedError(
                "grad_mode='dp': the DP hooks are not built for %s (grad_mode 'sparse' or 'fused_sgd')"
                % type(self).__name__)
        rows = [int(n) for n in rows]
        if weights is None and init == "numpy":
            # the reference's draw: numpy global RNG, U(-sqrt(1/n), sqrt(1/n)), f32
            weights = [torch.from_numpy(np.random.uniform(low=-np.sqrt(1 / n), high=np.sqrt(1 / n),
                                                          size=(n, dim)).astype(np.float32)) for n in rows]
        self._tset = EmbeddingTableSet(rows, dim, device=device, init=None if weights is not None else "uniform",
                                       seed=seed, weights=weights)
        self.embedding_bag = _WeightHolder(nn.Parameter(self._tset.W, requires_grad=True))
        _register_sgd_owner(self, self.embedding_bag.weight)
        return weights

    def _begin_forward(self, test_mode: bool) -> None:
        """Before every forward: surface the device error flags, and bring the |W| hierarchy up to
        date on the rows an optimizer stepped (PACT's forward reads the table maximum from it)."""
        self._check_errors(test_mode)
        self._sync_external_update()

    def _module_batch(self, input, offsets) -> LookupBatch:
        return _batch_from_input(input, offsets, self._tset.device)

    def _collection_batch(self, lS_o, lS_i) -> LookupBatch:
        return LookupBatch(lS_i, lS_o, device=self._tset.device, pooling_one=_pooling_one_arg())

    def _full_precision(self, batch: LookupBatch, layout: str) -> torch.Tensor:
        """full_precision_flag: the plain FP32 EmbeddingBag sum (dqrm_emb_fwd), identity backward."""
        return _EmbeddingFn.apply(self.embedding_bag.weight, self, batch, 4, False, True, layout)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._tset.refresh_absmax()  # W changed outside the kernels: rebuild the |W| hierarchy
        return out
