"""CPU checks of the fused MLP activations' host side: the two `_act` exports and DQRM_ACT_* in
the header, the library and the binding, their argument errors, fuse_activations /
unfuse_activations / create_mlp / apply_mlp on CPU-constructed modules, and QuantLinear.activation's
error behaviour."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ql(i, o, **kw):
    q = dq.QuantLinear(weight_bit=4, bias_bit=4, **kw)
    q.set_param(nn.Linear(i, o))
    return q


def _stack():
    return nn.ModuleList([_ql(6, 5), nn.ReLU(), _ql(5, 4), nn.ReLU(), _ql(4, 1), nn.Sigmoid()])


# ------------------------------------------------------------------ the C ABI
def test_header_library_and_binding_carry_the_act_exports():
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+dqrm_linear_fwd_act\s*\(", code) and re.search(r"\bint\s+dqrm_linear_bwd_act\s*\(", code)
    for name, value in (("DQRM_ACT_NONE", 0), ("DQRM_ACT_RELU", 1), ("DQRM_ACT_SIGMOID", 2)):
        assert int(re.search(name + r"\s*=\s*(\d+)", code).group(1)) == value
        assert getattr(L, name) == value
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    dq.build(verbose=False)
    lib = L.load()
    for name in ("dqrm_linear_fwd_act", "dqrm_linear_bwd_act"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.dqrm_linear_fwd_act.argtypes) == 7 and len(lib.dqrm_linear_bwd_act.argtypes) == 11


def _c_layer():
    c = L.Linear()
    c.in_features, c.out_features, c.weight_bit, c.bias_bit = 4, 2, 4, 4
    c.weight, c.bias, c.weight_integer, c.bias_integer, c.scale = 0x10, 0x20, 0x30, 0x40, 0x50
    return c


def test_act_calls_reject_bad_arguments_without_device():
    dq.build(verbose=False)
    lib = L.load()
    c = _c_layer()
    X, Y, DY, DW, DB = 0x60, 0x70, 0x80, 0x90, 0xA0  # never dereferenced: every call fails its checks
    for act in (-1, 3):
        assert lib.dqrm_linear_fwd_act(C.byref(c), 1, act, X, 3, Y, None) == L.DQRM_E_INVALID
        assert b"act" in lib.dqrm_last_error() and b"dqrm_linear_fwd_act" in lib.dqrm_last_error()
        assert lib.dqrm_linear_bwd_act(C.byref(c), 1, act, X, Y, DY, 3, None, DW, DB, None) == L.DQRM_E_INVALID
        assert b"act" in lib.dqrm_last_error() and b"dqrm_linear_bwd_act" in lib.dqrm_last_error()
    for act in (L.DQRM_ACT_RELU, L.DQRM_ACT_SIGMOID):
        assert lib.dqrm_linear_bwd_act(C.byref(c), 1, act, X, None, DY, 3, None, DW, DB, None) == L.DQRM_E_INVALID
        assert b"null y" in lib.dqrm_last_error()
    # the checks of dqrm_linear_fwd / _bwd
    assert lib.dqrm_linear_fwd_act(None, 1, L.DQRM_ACT_RELU, X, 3, Y, None) == L.DQRM_E_INVALID
    assert b"null layer" in lib.dqrm_last_error()
    assert lib.dqrm_linear_fwd_act(C.byref(c), 1, L.DQRM_ACT_RELU, None, 3, None, None) == L.DQRM_E_INVALID
    assert b"null x" in lib.dqrm_last_error()
    assert lib.dqrm_linear_fwd_act(C.byref(c), 1, L.DQRM_ACT_RELU, X, -1, Y, None) == L.DQRM_E_INVALID
    assert b"batch size" in lib.dqrm_last_error()
    assert lib.dqrm_linear_bwd_act(C.byref(c), 1, L.DQRM_ACT_NONE, None, None, None, 3, None, None, None,
                                   None) == L.DQRM_E_INVALID
    assert b"null x" in lib.dqrm_last_error()
    assert lib.dqrm_linear_bwd_act(C.byref(c), 1, L.DQRM_ACT_SIGMOID, X, Y, DY, 0, None, DW, DB, None) == L.DQRM_E_INVALID
    assert b"batch size" in lib.dqrm_last_error()
    c.weight_bit = 1
    assert lib.dqrm_linear_fwd_act(C.byref(c), 1, L.DQRM_ACT_SIGMOID, X, 3, Y, None) == L.DQRM_E_INVALID
    assert b"weight_bit" in lib.dqrm_last_error()
    c.weight_bit, c.out_features = 4, 0
    assert lib.dqrm_linear_bwd_act(C.byref(c), 1, L.DQRM_ACT_RELU, X, Y, DY, 3, None, DW, DB, None) == L.DQRM_E_INVALID
    assert b"out_features" in lib.dqrm_last_error()


# ------------------------------------------------------------------ fuse / unfuse
def test_fuse_keeps_positions_and_state_dict_keys():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.bot_l = _stack()

    m = M()
    keys = list(m.state_dict().keys())
    assert "bot_l.0.weight" in keys and "bot_l.2.weight" in keys and "bot_l.4.bias" in keys
    saved = io.BytesIO()
    torch.save(m.state_dict(), saved)
    assert dq.fuse_activations(m.bot_l) == 3
    assert list(m.state_dict().keys()) == keys
    assert [type(l).__name__ for l in m.bot_l] == ["QuantLinear", "FusedActivation"] * 3
    assert [l.activation for l in m.bot_l if isinstance(l, dq.QuantLinear)] == ["relu", "relu", "sigmoid"]
    assert [l.kind for l in m.bot_l if isinstance(l, dq.FusedActivation)] == ["relu", "relu", "sigmoid"]
    # a state dict saved unfused loads into the fused stack, and the fused one's back
    saved.seek(0)
    other = M()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(1.0)
    m.load_state_dict(torch.load(saved))
    fused_sd = m.state_dict()
    other.load_state_dict(fused_sd)
    for k in keys:
        assert torch.equal(other.state_dict()[k], fused_sd[k])
    # idempotent
    assert dq.fuse_activations(m.bot_l) == 0
    assert [type(l).__name__ for l in m.bot_l] == ["QuantLinear", "FusedActivation"] * 3
    # and back
    assert dq.unfuse_activations(m.bot_l) == 3
    assert [type(l) for l in m.bot_l][1::2] == [nn.ReLU, nn.ReLU, nn.Sigmoid]
    assert all(l.activation is None for l in m.bot_l if isinstance(l, dq.QuantLinear))
    assert list(m.state_dict().keys()) == keys
    assert dq.unfuse_activations(m.bot_l) == 0


def test_fused_activation_placeholder():
    f = dq.FusedActivation("relu")
    assert list(f.parameters()) == [] and list(f.buffers()) == [] and f.state_dict() == {}
    x = torch.tensor([-1.0, 2.0])
    assert f(x) is x
    assert "relu" in repr(f) and "fused into the preceding" in repr(f)
    assert "sigmoid" in repr(dq.FusedActivation("sigmoid"))
    with pytest.raises(ValueError):
        dq.FusedActivation("tanh")


def test_fuse_leaves_everything_else_alone():
    plain, relu_after_plain = nn.Linear(4, 4), nn.ReLU()
    tanh, inplace = nn.Tanh(), nn.ReLU(inplace=True)
    second = nn.ReLU()
    layers = [plain, relu_after_plain,   # a plain nn.Linear + ReLU pair
              _ql(4, 4), tanh,           # another activation module after ours
              nn.Identity(), inplace,    # an in-place ReLU after something that is not ours
              _ql(4, 4), nn.Sigmoid(), second]  # only the module directly after the layer
    assert dq.fuse_activations(layers) == 1
    assert layers[0] is plain and layers[1] is relu_after_plain
    assert layers[3] is tanh and layers[2].activation is None
    assert layers[5] is inplace
    assert isinstance(layers[7], dq.FusedActivation) and layers[6].activation == "sigmoid"
    assert layers[8] is second
    assert dq.fuse_activations(layers) == 0
    assert dq.unfuse_activations(layers) == 1 and type(layers[7]) is nn.Sigmoid


def test_apply_mlp_is_the_references_loop():
    """A QuantLinear gets the (x, scale) call and returns a pair; any other module maps x."""
    calls = []

    class Stub(dq.QuantLinear):
        def forward(self, x, prev_act_scaling_factor=None):
            calls.append(("quant", prev_act_scaling_factor))
            return x + 1.0, None

    class Plain(nn.Module):
        def forward(self, x):
            calls.append(("plain",))
            return x * 2.0

    layers = nn.ModuleList([Stub(), nn.ReLU(), Stub(), Plain()])
    assert dq.fuse_activations(layers) == 1
    out = dq.apply_mlp(torch.zeros(2, 3), layers)
    assert calls == [("quant", None), ("quant", None), ("plain",)]
    assert torch.equal(out, torch.full((2, 3), 4.0))


def test_create_mlp_draw_sequence_and_structure():
    ln = np.array([13, 32, 16])
    np.random.seed(11)
    layers = dq.create_mlp(ln, -1, weight_bit=8, per_channel=True)
    np.random.seed(11)
    for i in range(ln.size - 1):
        n, m = int(ln[i]), int(ln[i + 1])
        W = np.random.normal(0.0, np.sqrt(2 / (m + n)), size=(m, n)).astype(np.float32)
        b = np.random.normal(0.0, np.sqrt(1 / m), size=m).astype(np.float32)
        q = layers[2 * i]
        assert type(q) is dq.QuantLinear and q.weight.dtype == torch.float32
        np.testing.assert_array_equal(q.weight.detach().numpy(), W)
        np.testing.assert_array_equal(q.bias.detach().numpy(), b)
        assert (q.weight_bit, q.bias_bit, q.per_channel, q.full_precision_flag) == (8, 8, True, False)
        assert q.activation == "relu" and isinstance(layers[2 * i + 1], dq.FusedActivation)
    assert isinstance(layers, nn.ModuleList) and len(layers) == 4
    # a sigmoid after layer `sigmoid_layer`, torch modules when not fused, defaults of the signature
    np.random.seed(11)
    plain = dq.create_mlp([20, 32, 1], 1, fused=False)
    assert [type(l) for l in plain] == [dq.QuantLinear, nn.ReLU, dq.QuantLinear, nn.Sigmoid]
    assert all(l.activation is None and (l.weight_bit, l.bias_bit, l.per_channel, l.full_precision_flag) ==
               (4, 4, False, False) for l in plain[::2])
    assert dq.fuse_activations(plain) == 2 and plain[2].activation == "sigmoid"
    for name in ("create_mlp", "apply_mlp", "fuse_activations", "unfuse_activations", "FusedActivation"):
        assert name in dq.__all__


# ------------------------------------------------------------------ QuantLinear.activation
def test_activation_attribute_errors_and_default():
    q = _ql(6, 3)
    assert q.activation is None and "activation" not in q.__dict__  # older pickles read the default
    assert type(q).__name__ == "QuantLinear"
    for act in ("relu", "sigmoid"):
        q.activation = act
        with pytest.raises(L.DQRMError):  # no CPU path, fused or not
            q(torch.zeros(2, 6))
    for bad in ("tanh", "ReLU", 1, ["relu"]):
        q.activation = bad
        with pytest.raises(ValueError, match="activation"):
            q(torch.zeros(2, 6))
    # a layer whose instance dict lacks the attribute (pickled before it existed) still loads and reads None
    q.activation = "relu"
    state = q.__getstate__() if hasattr(q, "__getstate__") else dict(q.__dict__)
    state = {k: v for k, v in state.items() if k != "activation"}
    old = dq.QuantLinear.__new__(dq.QuantLinear)
    old.__setstate__(state)
    assert old.activation is None
