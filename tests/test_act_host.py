"""Host-side checks of QuantAct and the activation-quantized QuantLinear / MLP plumbing: exports,
constructor, buffers, errors, the C calls' argument validation (no device needed), and the
invariants of the CPU restatement the GPU tests compare against (tests/cpu_act.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import cpu_act as A
import cpu_linear as R
import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(**kw):
    q = dq.QuantLinear(**kw)
    q.set_param(nn.Linear(6, 3))
    return q


# ------------------------------------------------------------------ exports and constructor
def test_exports_where_the_reference_keeps_them():
    from deep_quantized_recommendation_model_dqrm_amd.quant_modules_not_quantize_grad import QuantAct, QuantLinear
    assert QuantAct is dq.QuantAct and QuantLinear is dq.QuantLinear
    assert "QuantAct" in dq.__all__ and "QuantAct" in dq.quant_modules_not_quantize_grad.__all__


def test_constructor_defaults_buffers_and_state_dict():
    sig = inspect.signature(dq.QuantAct.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("activation_bit", 4), ("act_range_momentum", 0.95), ("full_precision_flag", False),
        ("running_stat", True), ("quant_mode", "symmetric"), ("fix_flag", False), ("act_percentile", 0),
        ("fixed_point_quantization", False)]
    fsig = inspect.signature(dq.QuantAct.forward)
    assert list(fsig.parameters)[1:] == ["x", "pre_act_scaling_factor", "pre_weight_scaling_factor", "identity",
                                         "identity_scaling_factor", "identity_weight_scaling_factor"]
    q = dq.QuantAct()
    keys = ["x_min", "x_max", "act_scaling_factor", "pre_weight_scaling_factor", "identity_weight_scaling_factor"]
    assert list(q.state_dict().keys()) == keys
    assert [n for n, _ in q.named_buffers()] == keys
    assert all(b.shape == (1,) and b.dtype == torch.float32 for b in q.buffers())
    assert [float(q.state_dict()[k]) for k in keys] == [0.0, 0.0, 0.0, 1.0, 1.0]
    assert not list(q.parameters())
    # the drivers' two modules (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:475-476)
    a = dq.QuantAct(activation_bit=8, act_range_momentum=-1)
    b = dq.QuantAct(fixed_point_quantization=True, activation_bit=8, act_range_momentum=-1)
    assert (a.activation_bit, a.act_range_momentum, a.fixed_point_quantization) == (8, -1, False)
    assert b.fixed_point_quantization is True
    q2 = dq.QuantAct()
    q.x_min.fill_(-1.5)
    q2.load_state_dict(q.state_dict())
    assert float(q2.x_min) == -1.5


def test_repr_fix_and_unfix():
    q = dq.QuantAct(activation_bit=8)
    q.x_min.fill_(-1.256)
    q.x_max.fill_(2.5)
    assert repr(q) == ("QuantAct(activation_bit=8, full_precision_flag=False, quant_mode=symmetric, "
                       "Act_min: -1.26, Act_max: 2.50)")
    q.fix()
    assert (q.running_stat, q.fix_flag) == (False, True)
    q.unfix()
    assert (q.running_stat, q.fix_flag) == (True, False)


# ------------------------------------------------------------------ errors
def test_quantact_errors_as_specified():
    x = torch.zeros(2, 6)
    with pytest.raises(ValueError, match="unknown quant mode"):
        dq.QuantAct(quant_mode="other")(x)
    with pytest.raises(NotImplementedError, match="asymmetric"):
        dq.QuantAct(quant_mode="asymmetric")(x)
    with pytest.raises(NotImplementedError, match="act_percentile"):
        dq.QuantAct(act_percentile=99.9)(x)
    with pytest.raises(NotImplementedError, match="fixed_point_quantization"):
        dq.QuantAct()(x, torch.ones(1))
    with pytest.raises(NotImplementedError, match="fixed_point_quantization"):
        dq.QuantAct()((x, torch.ones(1)))  # the tuple input
    with pytest.raises(NotImplementedError, match="identity"):
        dq.QuantAct()(x, None, None, x)
    # no CPU path: with and without a previous scale, and in full precision
    for q, args in ((dq.QuantAct(), (x,)), (dq.QuantAct(fixed_point_quantization=True), (x, torch.ones(1))),
                    (dq.QuantAct(fixed_point_quantization=True), ((x, torch.ones(1)),)),
                    (dq.QuantAct(full_precision_flag=True), (x,))):
        with pytest.raises(L.DQRMError):
            q(*args)


def test_quantlinear_activation_scale_errors():
    x = torch.zeros(2, 6)
    with pytest.raises(ValueError, match="prev_act_scaling_factor"):  # the reference: a NameError
        _layer(bias_bit=4, quantize_activation=True)(x)
    with pytest.raises(NotImplementedError, match="without"):
        _layer(bias_bit=4)(x, torch.ones(1))
    for bad in (torch.ones(3), torch.ones(1, 3), torch.ones(0), 0.5):
        with pytest.raises(ValueError, match="ONE element"):
            _layer(bias_bit=4, quantize_activation=True)(x, bad)
        with pytest.raises(ValueError, match="ONE element"):
            _layer(bias_bit=4, quantize_activation=True)((x, bad))
    # a good scale reaches the device check: there is no CPU path
    for prev in (torch.ones(1), torch.ones(1, 1)):
        with pytest.raises(L.DQRMError):
            _layer(bias_bit=4, quantize_activation=True)(x, prev)
    # nn.Module's own machinery still works on the layer and on a stack of them (.to / .float / .cpu)
    assert _layer(bias_bit=4, quantize_activation=True).float().to("cpu").weight.dtype == torch.float32
    assert len(dq.create_mlp([6, 3], -1, quantize_activation=True).cpu().float()) == 2
    assert dq.QuantAct().float().to("cpu").x_min.shape == (1,)
    # full precision ignores the flag and the scale, as the reference does (:210-211)
    with pytest.raises(L.DQRMError):
        _layer(bias_bit=4, quantize_activation=True, full_precision_flag=True)(x)


# ------------------------------------------------------------------ mlp plumbing
def test_create_mlp_passes_quantize_activation_and_apply_mlp_takes_a_scale():
    sig = inspect.signature(dq.create_mlp)
    assert list(sig.parameters)[-1] == "quantize_activation" and sig.parameters["quantize_activation"].default is False
    assert list(sig.parameters)[:6] == ["ln", "sigmoid_layer", "weight_bit", "full_precision_flag", "per_channel",
                                        "fused"]
    np.random.seed(3)
    on = dq.create_mlp([13, 8, 4], 1, quantize_activation=True)
    np.random.seed(3)
    off = dq.create_mlp([13, 8, 4], 1)
    assert [l.quantize_activation for l in on if isinstance(l, dq.QuantLinear)] == [True, True]
    assert [l.quantize_activation for l in off if isinstance(l, dq.QuantLinear)] == [False, False]
    assert [l.activation for l in on[::2]] == ["relu", "sigmoid"]
    assert all(torch.equal(a.weight, b.weight) for a, b in zip(on[::2], off[::2]))  # the same draws
    asig = inspect.signature(dq.apply_mlp)
    assert list(asig.parameters) == ["x", "layers", "prev_act_scaling_factor"]
    assert asig.parameters["prev_act_scaling_factor"].default is None

    calls = []

    class Stub(dq.QuantLinear):
        def forward(self, x, prev_act_scaling_factor=None):
            calls.append(prev_act_scaling_factor)
            return x + 1.0, prev_act_scaling_factor * 2.0

    out = dq.apply_mlp(torch.zeros(2, 3), nn.ModuleList([Stub(), nn.ReLU(), Stub()]), torch.tensor([0.5]))
    assert [float(c) for c in calls] == [0.5, 1.0] and torch.equal(out, torch.full((2, 3), 2.0))
    with pytest.raises(ValueError, match="prev_act_scaling_factor"):  # a quantize_activation stack needs one
        dq.apply_mlp(torch.zeros(2, 13), on)


# ------------------------------------------------------------------ the C ABI
def test_abi_symbols_struct_and_version():
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    dq.build(verbose=False)
    lib = L.load()
    assert lib.dqrm_abi_version() == 12
    for name in ("dqrm_act_quant_workspace_bytes", "dqrm_act_quant_fwd", "dqrm_act_quant_bwd",
                 "dqrm_linear_wquant_qact", "dqrm_linear_fwd_qact", "dqrm_linear_bwd_qact"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    # dqrm_act_quant: 2 x i32 + 2 x f32 + 3 pointers; dqrm_linear unchanged
    assert C.sizeof(L.ActQuant) == 16 + 3 * 8
    assert C.sizeof(L.Linear) == 24 + 5 * 8


def test_act_calls_reject_bad_arguments_without_device():
    dq.build(verbose=False)
    lib = L.load()
    assert lib.dqrm_act_quant_fwd(None, 0x10, 4, 0x20, None, None) == L.DQRM_E_INVALID
    assert b"null dqrm_act_quant" in lib.dqrm_last_error()
    q = L.ActQuant()
    q.activation_bit, q.running_stat, q.momentum, q.one_minus_momentum = 8, 1, 0.95, 0.05
    q.x_min, q.x_max, q.scale = 0x100, 0x200, 0x300
    for bits in (1, 0, 33, -4):
        q.activation_bit = bits
        assert lib.dqrm_act_quant_fwd(C.byref(q), 0x10, 4, 0x20, None, None) == L.DQRM_E_INVALID
        assert b"activation_bit" in lib.dqrm_last_error()
    q.activation_bit = 8
    for field in ("x_min", "x_max", "scale"):
        old = getattr(q, field)
        setattr(q, field, None)
        assert lib.dqrm_act_quant_fwd(C.byref(q), 0x10, 4, 0x20, None, None) == L.DQRM_E_INVALID
        assert b"null x_min / x_max / scale" in lib.dqrm_last_error()
        setattr(q, field, old)
    assert lib.dqrm_act_quant_fwd(C.byref(q), 0x10, -1, 0x20, None, None) == L.DQRM_E_INVALID
    assert b"negative numel" in lib.dqrm_last_error()
    assert lib.dqrm_act_quant_fwd(C.byref(q), None, 4, 0x20, None, None) == L.DQRM_E_INVALID
    assert b"null x" in lib.dqrm_last_error()
    q.running_stat = 0
    assert lib.dqrm_act_quant_fwd(C.byref(q), 0x10, 4, None, None, None) == L.DQRM_E_INVALID
    assert b"null y" in lib.dqrm_last_error()
    q.running_stat = 1
    big = 1 << 20
    assert lib.dqrm_act_quant_workspace_bytes(big) > 0 and lib.dqrm_act_quant_workspace_bytes(7) == 0
    assert lib.dqrm_act_quant_workspace_bytes(-1) == L.DQRM_E_INVALID
    assert lib.dqrm_act_quant_fwd(C.byref(q), 0x10, big, 0x20, None, None) == L.DQRM_E_INVALID
    assert b"workspace" in lib.dqrm_last_error()
    # numel == 0: a no-op before any pointer is looked at
    assert lib.dqrm_act_quant_fwd(C.byref(q), None, 0, None, None, None) == L.DQRM_OK
    assert lib.dqrm_act_quant_bwd(None, 0x10, 4, 0x20, None) == L.DQRM_E_INVALID
    assert b"null scale" in lib.dqrm_last_error()
    assert lib.dqrm_act_quant_bwd(0x300, 0x10, -2, 0x20, None) == L.DQRM_E_INVALID
    assert lib.dqrm_act_quant_bwd(0x300, None, 4, 0x20, None) == L.DQRM_E_INVALID
    assert lib.dqrm_act_quant_bwd(0x300, 0x10, 4, None, None) == L.DQRM_E_INVALID
    assert b"null dy / dx" in lib.dqrm_last_error()
    assert lib.dqrm_act_quant_bwd(0x300, None, 0, None, None) == L.DQRM_OK


def test_qact_linear_calls_reject_bad_arguments_without_device():
    dq.build(verbose=False)
    lib = L.load()
    assert lib.dqrm_linear_wquant_qact(None, 0x10, 0x20, None) == L.DQRM_E_INVALID
    assert b"null layer" in lib.dqrm_last_error()
    c = L.Linear()
    c.in_features, c.out_features, c.weight_bit, c.bias_bit = 4, 2, 4, 4
    c.weight, c.bias, c.weight_integer, c.bias_integer, c.scale = 0x10, 0x20, 0x30, 0x40, 0x50
    for prev, cos in ((None, 0x70), (0x60, None)):
        assert lib.dqrm_linear_wquant_qact(C.byref(c), prev, cos, None) == L.DQRM_E_INVALID
        assert b"null prev / out_scale" in lib.dqrm_last_error()
        assert lib.dqrm_linear_fwd_qact(C.byref(c), 0, 0x80, prev, cos, 3, 0x90, None) == L.DQRM_E_INVALID
        assert b"null prev / out_scale" in lib.dqrm_last_error()
        assert lib.dqrm_linear_bwd_qact(C.byref(c), 0, 0x80, None, 0x90, prev, cos, 3, None, 0xa0, 0xb0,
                                        None) == L.DQRM_E_INVALID
        assert b"null prev / out_scale" in lib.dqrm_last_error()
    assert lib.dqrm_linear_fwd_qact(C.byref(c), 3, 0x80, 0x60, 0x70, 3, 0x90, None) == L.DQRM_E_INVALID
    assert b"act" in lib.dqrm_last_error()
    assert lib.dqrm_linear_fwd_qact(C.byref(c), 0, None, 0x60, 0x70, 3, 0x90, None) == L.DQRM_E_INVALID
    assert b"null x" in lib.dqrm_last_error()
    assert lib.dqrm_linear_fwd_qact(C.byref(c), 0, 0x80, 0x60, 0x70, -1, 0x90, None) == L.DQRM_E_INVALID
    assert lib.dqrm_linear_fwd_qact(C.byref(c), 0, None, 0x60, 0x70, 0, None, None) == L.DQRM_OK  # B == 0
    assert lib.dqrm_linear_bwd_qact(C.byref(c), 1, 0x80, None, 0x90, 0x60, 0x70, 3, None, 0xa0, 0xb0,
                                    None) == L.DQRM_E_INVALID
    assert b"null y" in lib.dqrm_last_error()
    assert lib.dqrm_linear_bwd_qact(C.byref(c), 0, 0x80, None, 0x90, 0x60, 0x70, 0, None, 0xa0, 0xb0,
                                    None) == L.DQRM_E_INVALID  # the backward needs B >= 1, as dqrm_linear_bwd
    c.bias_bit = 0  # quantized only: there is no full-precision form
    assert lib.dqrm_linear_fwd_qact(C.byref(c), 0, 0x80, 0x60, 0x70, 3, 0x90, None) == L.DQRM_E_INVALID
    assert b"bias_bit" in lib.dqrm_last_error()


# ------------------------------------------------------------------ the restatement's invariants
def test_restatement_range_init_by_add_minmax_and_ema():
    a = A.ActRef(bits=8, momentum=-1)
    a.forward(torch.zeros(3, 4))  # all equal: the bounds stay equal, the scale takes the clamp
    assert float(a.x_min) == 0.0 == float(a.x_max)
    assert float(a.scale) == float(np.float32(1e-8) / np.float32(127))
    a.forward(torch.tensor([[-1.0, 2.0]]))  # "initialization" again: an add onto equal bounds
    assert (float(a.x_min), float(a.x_max)) == (-1.0, 2.0)
    a.forward(torch.tensor([[-0.5, 3.0]]))
    assert (float(a.x_min), float(a.x_max)) == (-1.0, 3.0)
    a.fix()
    y, s = a.forward(torch.tensor([[-9.0, 9.0, 0.1]]))
    assert (float(a.x_min), float(a.x_max)) == (-1.0, 3.0) and float(s) == float(np.float32(3.0) / np.float32(127))
    assert y[0, 0] == -128 * s and y[0, 1] == 127 * s  # the clamp is asymmetric
    # the quirk: equal non-zero bounds are added to, not replaced
    b = A.ActRef(bits=8, momentum=0.95)
    b.forward(torch.full((2, 2), 0.375))
    assert float(b.x_min) == 0.375 == float(b.x_max)
    b.forward(torch.tensor([[-1.0, 2.0]]))
    assert (float(b.x_min), float(b.x_max)) == (0.375 - 1.0, 0.375 + 2.0)
    b.forward(torch.tensor([[-4.0, 8.0]]))
    m, m1 = np.float32(0.95), np.float32(1.0 - 0.95)
    assert float(b.x_min) == float(np.float32(np.float32(-0.625) * m) + np.float32(np.float32(-4.0) * m1))
    assert float(b.x_max) == float(np.float32(np.float32(2.375) * m) + np.float32(np.float32(8.0) * m1))


def test_restatement_backward_and_layer_shapes():
    a = A.ActRef(bits=8, momentum=-1)
    x = torch.randn(5, 7, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    y, s = a.forward(x)
    dy = torch.randn(5, 7, generator=torch.Generator().manual_seed(1))
    y.backward(dy)
    assert torch.equal(x.grad, (dy * s) / s)
    W, b, x, dy, prev = A.exact_case(7, 13, 5, 8, True, seed=3)
    y, cos, (sc, wi, bi, pre, z), (dx, dw, db) = A.layer_forward_backward(x, W, b, dy, prev, 8, True)
    assert cos.shape == (1, 5) and torch.equal(cos.view(-1), sc * prev)
    assert torch.equal(y, torch.round(pre) * cos)
    want = A.backward_from_d(dy, x, wi, sc, prev)
    for got, w in zip((dx, dw, db), want):
        assert torch.equal(got, w)
    y, cos, _, _ = A.layer_forward_backward(x, W, b, dy, prev, 8, False)
    assert cos.shape == (1, 1)


def test_exact_cases_contain_round_half_even_ties():
    """The exact-data cases exercise the rounding: pre-round values with every quarter fraction,
    exact .5 ties among them, rounded to the even neighbour."""
    for (B, K, O), bits, pc in [((7, 13, 5), 8, True), ((64, 415, 1), 4, False), ((33, 512, 256), 4, True),
                                ((130, 70, 66), 8, False)]:
        W, b, x, dy, prev = A.exact_case(B, K, O, bits, pc, seed=7 + B)
        _, _, (s, wi, bi, pre, _), _ = A.layer_forward_backward(x, W, b, dy, prev, bits, pc)
        pre64 = (x.double() / prev.double()) @ wi.double().T + bi.double()
        assert torch.equal(pre.double(), pre64)  # the construction: exact in any order
        frac = pre64 - torch.floor(pre64)
        assert set(np.unique(frac.numpy())) == {0.0, 0.25, 0.5, 0.75}
        ties = pre64[frac == 0.5]
        assert ties.numel() > 0 and bool((torch.round(ties) % 2 == 0).all())
        assert bool((torch.round(ties) > ties).any()) and bool((torch.round(ties) < ties).any())
        assert float(wi.abs().max()) == R.qmax(bits)
        if O >= 60:  # enough biases that some saturate the clamp
            assert bool((bi.abs() >= R.qmax(bits)).any())
