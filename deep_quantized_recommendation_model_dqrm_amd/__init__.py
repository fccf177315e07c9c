"""MI355X-native (gfx950 / CDNA4) DQRM data-parallel QAT embedding path.

Drop-in for the reference's hot path (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM):
  * ``quant_modules_not_quantize_grad.QuantEmbeddingBagTwo``  (INT4 fake-quant EmbeddingBag)
  * ``quant_modules_not_quantize_grad.QuantLinear``            (INT4 fake-quant MLP layer, f32 MFMA)
  * ``quant_modules_not_quantize_grad.QuantAct``               (activation quantization with a running
                                                                range kept on the device)
  * ``DLRM_Net.create_mlp`` / ``apply_mlp``                      (``mlp``: the MLP stacks, ReLU / Sigmoid
                                                                fused into the layers' kernels)
  * ``DLRM_Net.interact_features``                               (``DotInteraction``: the dot interaction,
                                                                plain or 16-bit fake-quantized, fused)
  * ``DLRM_Net.forward``'s clamp and ``loss_fn_wrap``            (``DLRMLoss``: BCE / MSE / weighted BCE with
                                                                its gradient in one launch, a mean whose
                                                                bits depend on the batch size alone)
  * ``DLRM_Net`` itself and one iteration of its training loop  (``DQRMNet``: the stages above as one
                                                                model, ``train_step`` one host call)
  * ``inference()``'s accuracy count and ``roc_auc_score``     (``DLRMMetrics`` / ``DQRMNet.evaluate``: the
                                                                test loop's two numbers from integers kept
                                                                on the device, the AUC exact)
  * ``sgd_quantized_gradients_parallel_comm`` hooks            (INT8 sparse-grad all-reduce + SGD,
                                                                and the MLP's per-channel INT8 grads)
  * ``sgd_quantized_gradients`` simulated-DP buffer helpers     (embedding tables and the MLP's
                                                                error-compensated INT8 gradients)
  * ``quant_learned_step_size_quan.QuantEmbeddingBagLSQ`` and ``quant_pact_dorefa.QuantEmbeddingBagPACT``
                                                               (the --quant-mode lsq | pact embedding
                                                                baselines, fused; T-table collections)
  * ``quantized_ops.ops.quantized.embedding_bag_{4bit,byte}_*``  (row-wise PTQ inference formats)
  * ``DLRM_Net.quantize_embedding`` and the quantized ``apply_emb`` (``DQRMNet.quantize_embedding`` /
                                                                ``RowwiseTableSet``: all tables' row-wise
                                                                bags in one launch, the FP32 slab optional)
backed by hand-written HIP kernels behind the C ABI in ``include/dqrm.h`` (libdqrm.so).
"""
from . import _lib
from ._build import LIB_PATH, build
from .tables import CoalescedGrad, EmbeddingTableSet, LookupBatch, default_caps, reference_scale
from .comm import MultiSetExchange, SparseGradExchange, get_my_slice, payload_bytes
from .dense import DenseGradExchange, SimulatedDenseBuffers
from . import quant_modules_not_quantize_grad, sgd_quantized_gradients, sgd_quantized_gradients_parallel_comm
from .quant_modules_not_quantize_grad import QuantEmbeddingBagCollection, QuantEmbeddingBagTwo
from .linear import QuantLinear
from .act import QuantAct
from .mlp import FusedActivation, MLPStack, apply_mlp, create_mlp, fuse_activations, unfuse_activations
from .interaction import DotInteraction, interact_features
from .loss import DLRMLoss, loss_fn_wrap
from .rowwise import RowwiseTableSet
from .model import DQRMNet
from .metrics import DLRMMetrics
from . import quant_learned_step_size_quan, quant_pact_dorefa
from .quant_learned_step_size_quan import LSQEmbeddingBagCollection, LsqQuan, QuantEmbeddingBagLSQ
from .quant_pact_dorefa import PACTEmbeddingBagCollection, QuantEmbeddingBagPACT
from . import quantized_ops

__all__ = [
    "LIB_PATH",
    "build",
    "_lib",
    "EmbeddingTableSet",
    "LookupBatch",
    "CoalescedGrad",
    "default_caps",
    "reference_scale",
    "SparseGradExchange",
    "MultiSetExchange",
    "get_my_slice",
    "payload_bytes",
    "DenseGradExchange",
    "SimulatedDenseBuffers",
    "QuantEmbeddingBagTwo",
    "QuantEmbeddingBagCollection",
    "QuantLinear",
    "QuantAct",
    "create_mlp",
    "apply_mlp",
    "fuse_activations",
    "unfuse_activations",
    "FusedActivation",
    "MLPStack",
    "DotInteraction",
    "interact_features",
    "DLRMLoss",
    "loss_fn_wrap",
    "DQRMNet",
    "RowwiseTableSet",
    "DLRMMetrics",
    "LsqQuan",
    "QuantEmbeddingBagLSQ",
    "LSQEmbeddingBagCollection",
    "QuantEmbeddingBagPACT",
    "PACTEmbeddingBagCollection",
    "quant_learned_step_size_quan",
    "quant_pact_dorefa",
    "quant_modules_not_quantize_grad",
    "sgd_quantized_gradients",
    "sgd_quantized_gradients_parallel_comm",
    "quantized_ops",
]
