"""CPU checks of QuantLinear's host side: where it imports from, the reference's constructor
defaults, __repr__ and state-dict keys (quant_modules_not_quantize_grad.py:42-97), its error
behaviour, that the DP hooks select it, and ABI 12."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
from torch import nn

import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(**kw):
    q = dq.QuantLinear(**kw)
    q.set_param(nn.Linear(6, 3))
    return q


def test_imports_from_package_and_reference_module():
    from deep_quantized_recommendation_model_dqrm_amd import QuantLinear as A
    from deep_quantized_recommendation_model_dqrm_amd.quant_modules_not_quantize_grad import QuantLinear as B
    from deep_quantized_recommendation_model_dqrm_amd.linear import QuantLinear as D

    assert A is B is D
    assert "QuantLinear" in dq.__all__ and "QuantLinear" in dq.quant_modules_not_quantize_grad.__all__


def test_constructor_defaults_and_repr_are_the_references():
    sig = inspect.signature(dq.QuantLinear.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("weight_bit", 4), ("bias_bit", None), ("full_precision_flag", False), ("quant_mode", "symmetric"),
        ("per_channel", False), ("fix_flag", False), ("weight_percentile", 0), ("quantize_activation", False)]
    q = dq.QuantLinear()
    assert (q.weight_bit, q.bias_bit, q.full_precision_flag, q.quant_mode, q.per_channel, q.fix_flag,
            q.weight_percentile, q.quantize_activation, q.quantize_bias, q.counter) == \
        (4, None, False, "symmetric", False, False, 0, False, False, 0)
    assert repr(q) == "(QuantLinear() weight_bit=4, full_precision_flag=False, quantize_fn=symmetric)"
    # the drivers' positional call: weight_bit, bias_bit, full_precision_flag, per_channel=, quantize_activation=
    q = dq.QuantLinear(8, 16, True, per_channel=True, quantize_activation=False)
    assert (q.weight_bit, q.bias_bit, q.full_precision_flag, q.per_channel, q.quantize_bias) == (8, 16, True, True, True)
    assert repr(q) == "(QuantLinear() weight_bit=8, full_precision_flag=True, quantize_fn=symmetric)"
    q.fix()
    assert q.fix_flag is True
    q.unfix()
    assert q.fix_flag is False


def test_set_param_buffers_and_state_dict_keys():
    lin = nn.Linear(6, 3)
    q = dq.QuantLinear(weight_bit=4, bias_bit=8, per_channel=True)
    q.set_param(lin)
    assert (q.in_features, q.out_features) == (6, 3)
    assert list(q.state_dict().keys()) == ["weight", "bias", "fc_scaling_factor", "correct_output_scale",
                                           "weight_scaling_factor", "bias_scaling_factor"]
    assert sorted(n for n, _ in q.named_buffers()) == sorted([
        "fc_scaling_factor", "correct_output_scale", "weight_scaling_factor", "bias_scaling_factor",
        "weight_integer", "bias_integer", "error_compensation_weight", "error_compensation_bias"])
    assert torch.equal(q.weight.data, lin.weight.data) and q.weight.data_ptr() != lin.weight.data_ptr()
    assert torch.equal(q.bias.data, lin.bias.data)
    assert q.weight_integer.shape == (3, 6) and q.bias_integer.shape == (3,)
    assert torch.equal(q.correct_output_scale, torch.ones(3)) and torch.equal(q.fc_scaling_factor, torch.zeros(3))
    # a state dict round trip through a second layer
    q2 = _layer(weight_bit=4, bias_bit=8, per_channel=True)
    q2.load_state_dict(q.state_dict())
    assert torch.equal(q2.weight, q.weight)


def test_cpu_forward_raises_dqrm_error():
    for kw in (dict(bias_bit=4), dict(bias_bit=4, full_precision_flag=True)):
        with pytest.raises(L.DQRMError):
            _layer(**kw)(torch.zeros(2, 6))
    with pytest.raises(L.DQRMError):
        _layer(bias_bit=4)((torch.zeros(2, 6), None))  # the reference's (x, scale) tuple input


def test_unsupported_modes_raise_as_specified():
    x = torch.zeros(2, 6)
    with pytest.raises(Exception, match="only support symmetric") as e:
        _layer(bias_bit=4, quant_mode="asymmetric")(x)
    assert type(e.value) is Exception
    with pytest.raises(ValueError, match="unknown quant mode"):
        _layer(bias_bit=4, quant_mode="other")(x)
    with pytest.raises(NotImplementedError):
        _layer(bias_bit=4, quantize_activation=True)(x)
    with pytest.raises(NotImplementedError):
        _layer(bias_bit=4)(x, torch.ones(1))
    with pytest.raises(NotImplementedError):
        _layer(bias_bit=4)((x, torch.ones(1)))


def test_hooks_select_package_quantlinear_layers():
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients_parallel_comm as H

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.bot_l = nn.ModuleList([_layer(bias_bit=4), nn.ReLU(), _layer(bias_bit=4), nn.Linear(3, 3)])

    m = M()
    assert H._linear_layers(m, "bot_l") == [m.bot_l[0], m.bot_l[2]]


def test_abi_12_in_header_binding_and_library():
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12
    dq.build(verbose=False)
    lib = L.load()
    assert lib.dqrm_abi_version() == 12
    for name in ("dqrm_linear_wquant", "dqrm_linear_fwd", "dqrm_linear_bwd"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    # dqrm_linear: 6 x i32 + 5 pointers
    assert C.sizeof(L.Linear) == 24 + 5 * 8


def test_linear_calls_reject_bad_arguments_without_device():
    dq.build(verbose=False)
    lib = L.load()
    assert lib.dqrm_linear_wquant(None, None) == L.DQRM_E_INVALID
    assert b"null layer" in lib.dqrm_last_error()
    c = L.Linear()
    c.in_features, c.out_features, c.weight_bit, c.bias_bit = 4, 0, 4, 4
    assert lib.dqrm_linear_fwd(C.byref(c), 1, None, 1, None, None) == L.DQRM_E_INVALID
    assert b"out_features" in lib.dqrm_last_error()
    c.out_features = 2
    c.weight, c.bias, c.weight_integer, c.bias_integer, c.scale = 0x10, 0x20, 0x30, 0x40, 0x50
    c.weight_bit = 1
    assert lib.dqrm_linear_wquant(C.byref(c), None) == L.DQRM_E_INVALID
    assert b"weight_bit" in lib.dqrm_last_error()
    c.weight_bit = 4
    assert lib.dqrm_linear_fwd(C.byref(c), 1, None, 3, None, None) == L.DQRM_E_INVALID
    assert b"null x" in lib.dqrm_last_error()
    assert lib.dqrm_linear_bwd(C.byref(c), 1, None, None, 3, None, None, None, None) == L.DQRM_E_INVALID
    c.weight_integer = None
    assert lib.dqrm_linear_fwd(C.byref(c), 1, 0x60, 3, 0x70, None) == L.DQRM_E_INVALID
    assert b"weight_integer" in lib.dqrm_last_error()
