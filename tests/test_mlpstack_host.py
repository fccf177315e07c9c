"""CPU checks of MLPStack's host side: the dqrm_mlp exports in the header and the binding, their
argument validation (before any device call), the two size queries, MLPStack's construction errors,
and the numpy restatement of the update against torch on the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import cpu_mlpstack as S
import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dqrm_mlp_fwd", "dqrm_mlp_bwd_scratch_bytes", "dqrm_mlp_bwd", "dqrm_mlp_sgd_workspace_bytes", "dqrm_mlp_sgd")


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


class FakeStack:
    """A valid dqrm_mlp over made-up device addresses: every call on it must stop in validation."""

    def __init__(self, widths=(6, 4, 3), per_channel=(1, 1), quantized=(1, 1), acts=(1, 0)):
        n = len(widths) - 1
        self.lin = (L.Linear * n)()
        for i in range(n):
            l = self.lin[i]
            l.in_features, l.out_features, l.weight_bit, l.bias_bit = widths[i], widths[i + 1], 4, 4
            l.per_channel = per_channel[i]
            base = 0x10000 * (i + 1)
            l.weight, l.bias, l.weight_integer, l.bias_integer, l.scale = (base + 0x1000 * j for j in range(1, 6))
        self.quantized = (C.c_int32 * n)(*quantized)
        self.act = (C.c_int32 * n)(*acts)
        self.c = L.MLP()
        self.c.num_layers = n
        self.c.layers, self.c.quantized, self.c.act = self.lin, self.quantized, self.act
        self.n = n

    def ptrs(self, first=0x900000):
        return (C.c_void_p * self.n)(*[first + 0x1000 * i for i in range(self.n)])


def _calls(lib, s, B=5, y=None, dw=None, db=None, scratch=0x700000, scratch_bytes=1 << 20, ws=0x800000,
           ws_bytes=1 << 20, x=0x500000, dy=0x600000, flags=1, gscale=None, stack=True):
    """The three exports on the stack, with valid (made-up) arguments unless overridden."""
    y = s.ptrs(0x900000) if y is None else y
    dw = s.ptrs(0xA00000) if dw is None else dw
    db = s.ptrs(0xB00000) if db is None else db
    c = C.byref(s.c) if stack else None
    return {
        "fwd": lambda: lib.dqrm_mlp_fwd(c, flags, x, B, y, None),
        "bwd": lambda: lib.dqrm_mlp_bwd(c, x, y, dy, B, None, dw, db, scratch, scratch_bytes, None),
        "sgd": lambda: lib.dqrm_mlp_sgd(c, flags, dw, db, gscale, 0.1, ws, ws_bytes, None),
    }


def _rejected(lib, calls, msg, which=("fwd", "bwd", "sgd")):
    for name in which:
        assert calls[name]() == L.DQRM_E_INVALID, name
        assert msg in lib.dqrm_last_error(), (name, lib.dqrm_last_error())


def test_header_binding_and_struct(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12 and lib.dqrm_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert int(re.search(r"^#define\s+DQRM_MLP_MAX_LAYERS\s+(\d+)", src, flags=re.M).group(1)) == \
        L.DQRM_MLP_MAX_LAYERS == 16
    assert L.DQRM_MLP_FRESH == 1 and L.DQRM_MLP_REQUANT == 1
    # dqrm_mlp: 2 x i32 + 3 pointers
    assert C.sizeof(L.MLP) == 8 + 3 * 8
    assert "MLPStack" in dq.__all__ and dq.MLPStack is dq.mlp.MLPStack


def test_null_stack_and_arrays_rejected(lib):
    s = FakeStack()
    _rejected(lib, _calls(lib, s, stack=False), b"null stack")
    assert lib.dqrm_mlp_bwd_scratch_bytes(None, 5) == 0 and lib.dqrm_mlp_sgd_workspace_bytes(None) == 0
    for field in ("layers", "quantized", "act"):
        s = FakeStack()
        setattr(s.c, field, None)
        _rejected(lib, _calls(lib, s), b"null layers / quantized / act")


def test_num_layers_out_of_range_rejected(lib):
    for n in (0, -1, 17):
        s = FakeStack()
        s.c.num_layers = n
        _rejected(lib, _calls(lib, s), b"num_layers")
        assert lib.dqrm_mlp_bwd_scratch_bytes(C.byref(s.c), 5) == 0
    s = FakeStack(widths=[4] * 17, per_channel=[1] * 16, quantized=[1] * 16, acts=[1] * 16)  # 16 layers pass this check
    s.lin[3].weight_bit = 1
    _rejected(lib, _calls(lib, s), b"layer 3: weight_bit")


def test_width_chain_act_bits_and_layer_pointers_rejected(lib):
    s = FakeStack()
    s.lin[1].in_features = 5
    _rejected(lib, _calls(lib, s), b"does not match")
    s = FakeStack()
    s.lin[0].out_features = 0
    _rejected(lib, _calls(lib, s), b"must be positive")
    for bad in (-1, 3):
        s = FakeStack(acts=(1, bad))
        _rejected(lib, _calls(lib, s), b"act must be")
    for field, bad in (("weight_bit", 1), ("weight_bit", 33), ("bias_bit", 1), ("bias_bit", 33)):
        s = FakeStack()
        setattr(s.lin[1], field, bad)
        _rejected(lib, _calls(lib, s), b"weight_bit / bias_bit")
    for field in ("weight", "bias"):
        s = FakeStack()
        setattr(s.lin[0], field, None)
        _rejected(lib, _calls(lib, s), b"null weight / bias")
    for field in ("weight_integer", "bias_integer", "scale"):
        s = FakeStack()
        setattr(s.lin[1], field, None)
        _rejected(lib, _calls(lib, s), b"null weight_integer")
    # a full-precision layer needs neither bits nor integer buffers: the call gets past the layer
    # checks and stops at the next bad argument
    s = FakeStack(quantized=(1, 0))
    s.lin[1].weight_bit, s.lin[1].weight_integer = 0, None
    _rejected(lib, _calls(lib, s, x=None), b"null x", which=("fwd", "bwd"))


def test_null_tensors_and_entries_rejected(lib):
    s = FakeStack()
    _rejected(lib, _calls(lib, s, x=None), b"null x", which=("fwd", "bwd"))
    _rejected(lib, _calls(lib, s, dy=None), b"null x / dy", which=("bwd",))
    assert lib.dqrm_mlp_fwd(C.byref(s.c), 0, 0x500000, 5, None, None) == L.DQRM_E_INVALID
    assert b"null y array" in lib.dqrm_last_error()
    null = C.cast(None, C.POINTER(C.c_void_p))
    assert lib.dqrm_mlp_bwd(C.byref(s.c), 0x500000, null, 0x600000, 5, None, s.ptrs(), s.ptrs(), 0x700000, 1 << 20,
                            None) == L.DQRM_E_INVALID
    assert b"null y array" in lib.dqrm_last_error()
    hole = s.ptrs()
    hole[1] = None
    _rejected(lib, _calls(lib, s, y=hole), b"null y[1]", which=("fwd", "bwd"))
    _rejected(lib, _calls(lib, s, dw=hole), b"null dw[1]", which=("bwd", "sgd"))
    _rejected(lib, _calls(lib, s, db=hole), b"null db[1]", which=("bwd", "sgd"))
    _rejected(lib, _calls(lib, s, gscale=hole), b"null gscale[1]", which=("sgd",))
    for name, k in (("dw", 6), ("db", 7)):
        args = [C.byref(s.c), 0x500000, s.ptrs(), 0x600000, 5, None, s.ptrs(), s.ptrs(), 0x700000, 1 << 20, None]
        args[k] = null
        assert lib.dqrm_mlp_bwd(*args) == L.DQRM_E_INVALID
        assert b"null %s array" % name.encode() in lib.dqrm_last_error()
        args = [C.byref(s.c), 1, s.ptrs(), s.ptrs(), None, 0.1, None, 0, None]
        args[k - 4] = null
        assert lib.dqrm_mlp_sgd(*args) == L.DQRM_E_INVALID
        assert b"null %s array" % name.encode() in lib.dqrm_last_error()


def test_batch_size_flags_scratch_and_workspace_rejected(lib):
    s = FakeStack()
    _rejected(lib, _calls(lib, s, B=-1), b"bad batch size", which=("fwd", "bwd"))
    _rejected(lib, _calls(lib, s, B=0), b"bad batch size", which=("bwd",))
    _rejected(lib, _calls(lib, s, B=1 << 31), b"bad batch size", which=("fwd", "bwd"))
    _rejected(lib, _calls(lib, s, flags=2), b"unknown flags", which=("fwd", "sgd"))
    # B == 0 in the forward: DQRM_OK and no launch (a launch on these addresses, or on a machine
    # without a device, could not return DQRM_OK)
    assert _calls(lib, s, B=0)["fwd"]() == L.DQRM_OK
    assert _calls(lib, s, B=0, x=None, flags=0)["fwd"]() == L.DQRM_OK
    need = lib.dqrm_mlp_bwd_scratch_bytes(C.byref(s.c), 5)
    assert need == 2 * 5 * 4 * 4
    _rejected(lib, _calls(lib, s, scratch_bytes=need - 1), b"scratch", which=("bwd",))
    _rejected(lib, _calls(lib, s, scratch=None), b"scratch", which=("bwd",))
    mixed = FakeStack(per_channel=(1, 0))
    need = lib.dqrm_mlp_sgd_workspace_bytes(C.byref(mixed.c))
    assert need == (4 + 3) * 4
    _rejected(lib, _calls(lib, mixed, ws_bytes=need - 1), b"workspace", which=("sgd",))
    _rejected(lib, _calls(lib, mixed, ws=None), b"workspace", which=("sgd",))


def test_size_queries(lib):
    s = FakeStack(widths=(13, 512, 256, 64, 1), per_channel=(1, 1, 1, 1), quantized=(1, 1, 1, 1), acts=(1, 1, 1, 2))
    for B in (1, 33, 2048):
        assert lib.dqrm_mlp_bwd_scratch_bytes(C.byref(s.c), B) == 2 * B * 512 * 4
    assert lib.dqrm_mlp_bwd_scratch_bytes(C.byref(s.c), 0) == 0
    assert lib.dqrm_mlp_bwd_scratch_bytes(C.byref(FakeStack(widths=(9, 7), per_channel=(1,), quantized=(1,),
                                                            acts=(0,)).c), 33) == 0  # one layer: no hidden tensor
    assert lib.dqrm_mlp_sgd_workspace_bytes(C.byref(s.c)) == 0  # all per channel
    mixed = FakeStack(widths=(13, 512, 256, 64, 1), per_channel=(1, 0, 1, 1), quantized=(1, 1, 1, 1), acts=(1, 1, 1, 2))
    assert lib.dqrm_mlp_sgd_workspace_bytes(C.byref(mixed.c)) == (512 + 256 + 64 + 1) * 4
    # the only per-tensor layer is full precision: nothing to requantize per tensor
    fp = FakeStack(widths=(13, 512, 256, 64, 1), per_channel=(1, 0, 1, 1), quantized=(1, 0, 1, 1), acts=(1, 1, 1, 2))
    assert lib.dqrm_mlp_sgd_workspace_bytes(C.byref(fp.c)) == 0


# ------------------------------------------------------------------ MLPStack's own errors
def test_mlpstack_needs_a_fused_list():
    np.random.seed(0)
    plain = dq.create_mlp([6, 4, 3], -1, fused=False)
    with pytest.raises(ValueError, match="fuse_activations"):
        dq.MLPStack(plain)
    assert dq.fuse_activations(plain) == 2
    stack = dq.MLPStack(plain)
    assert stack.layers == [plain[0], plain[2]] and not stack.is_fresh()
    with pytest.raises(ValueError, match="fuse_activations"):
        dq.MLPStack([plain[0], nn.Identity()])
    with pytest.raises(ValueError, match="fuse_activations"):
        dq.MLPStack([dq.FusedActivation("relu"), plain[0]])
    with pytest.raises(ValueError):
        dq.MLPStack([])
    # a plain list, and a layer without an activation after it
    assert len(dq.MLPStack([plain[0], plain[1], plain[2]]).layers) == 2
    # the list is left as it was
    assert [type(m).__name__ for m in plain] == ["QuantLinear", "FusedActivation"] * 2
    assert list(plain.state_dict().keys())[:2] == ["0.weight", "0.bias"]


def test_mlpstack_rejects_quantize_activation_and_long_stacks():
    np.random.seed(0)
    with pytest.raises(NotImplementedError):
        dq.MLPStack(dq.create_mlp([6, 4, 3], -1, quantize_activation=True))
    np.random.seed(0)
    assert len(dq.MLPStack(dq.create_mlp([3] * 17, -1)).layers) == 16
    with pytest.raises(ValueError, match="16"):
        dq.MLPStack(dq.create_mlp([3] * 18, -1))


def test_mlpstack_on_the_cpu_raises_dqrm_error():
    np.random.seed(0)
    layers = dq.create_mlp([6, 4, 3], -1)
    stack = dq.MLPStack(layers)
    with pytest.raises(L.DQRMError):
        stack(torch.zeros(2, 6))
    for p in layers.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(L.DQRMError):
        stack.sgd_step(0.1)
    with pytest.raises(L.DQRMError):
        stack.requantize()


# ------------------------------------------------------------------ the restatement of the update
@pytest.mark.parametrize("lr", [0.1, 24.0])
def test_numpy_update_is_torchs_and_differs_from_a_single_rounding(lr):
    rs = np.random.RandomState(5)
    W = rs.standard_normal((37, 130)).astype(np.float32)
    g = rs.standard_normal((37, 130)).astype(np.float32)
    p = nn.Parameter(torch.from_numpy(W.copy()))
    p.grad = torch.from_numpy(g.copy())
    p.data.add_(-lr * p.grad)
    got = S.sgd(W, g, lr)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, p.detach().numpy())
    differ = int((S.sgd_single_rounding(W, g, lr) != got).sum())
    print(f"lr {lr}: {differ} of {W.size} elements differ between two roundings and one")
    assert differ >= 1
    # the scaled form rounds three times, in dqrm_dense_update's order
    s = rs.uniform(0.5, 2.0, (37, 1)).astype(np.float32)
    t = torch.from_numpy(W.copy()) + (np.float32(-lr) * torch.from_numpy(g)) * torch.from_numpy(s)
    np.testing.assert_array_equal(S.sgd(W, g, lr, s), t.numpy())


def test_tie_case_contains_ties():
    W, b = S.tie_case(32, 13, 4, seed=3)
    s, wi, bi = S.quantize(W, b, 4, True)
    r = W / s.reshape(-1, 1)
    ties = np.abs(r - np.floor(r)) == 0.5
    assert ties.sum() > 20 and np.array_equal(wi[ties] % 2, np.zeros(int(ties.sum()), np.float32))  # half to even
    rb = b / s
    assert (np.abs(rb - np.floor(rb)) == 0.5).sum() >= 8
