"""CPU checks of the MLP half of the simulated-DP buffer: the numpy restatement against the torch-CPU
fixture, the two exports' argument validation (before any device call), the header / binding /
library agreement, and the bookkeeping of SimulatedDenseBuffers and the three hooks through
injected CPU kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import cpu_simdp as S
import deep_quantized_recommendation_model_dqrm_amd as dq
import gen_inputs as G
from deep_quantized_recommendation_model_dqrm_amd import _lib as L
from deep_quantized_recommendation_model_dqrm_amd import linear as LIN
from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients as H
from deep_quantized_recommendation_model_dqrm_amd.dense import DenseChannels, SimulatedDenseBuffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dqrm_dense_ec_accumulate", "dqrm_dense_sim_update")


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "simdp_mlp.npz"))


def _flat_params(params):
    return np.concatenate([np.concatenate([W.reshape(-1), b.reshape(-1)]) for W, b in params])


# ------------------------------------------------------------------ the restatement
def test_fixture_inputs_and_size(fx, golden_dir):
    assert fx["shapes"].tolist() == [list(s) for s in S.SHAPES] and int(fx["seed"]) == S.SEED
    assert np.float32(fx["lr"]) == np.float32(S.LR) and int(fx["windows"]) == 2
    inputs = [S.grads(w, k) for N in (3, 4) for w in range(2) for k in range(N)]
    assert str(fx["inputs_checksum"]) == G.checksum(inputs, S.layer_params())
    # the channel lengths the issue asks for, and the crafted rows
    ch = DenseChannels(S.torch_layers())
    assert sorted(set(ch.len.tolist())) == [1, 2, 3, 4, 5, 13, 64, 130, 1100]
    g0, g1 = S.grads(0, 0), S.grads(0, 1)
    assert g0[0][0][0].max() == 127.0 and {0.5, 1.5, 2.5, -0.5, -1.5} <= set(g0[0][0][0].tolist())
    assert not g0[1][0][1].any() and S.grads(0, 2)[1][0][1].any()
    np.testing.assert_array_equal(g1[2][0], (np.float32(3.5) * g0[2][0]).astype(np.float32))
    biggest = max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir)
                  if f.endswith(".npz") and f != "simdp_mlp.npz")
    assert os.path.getsize(os.path.join(golden_dir, "simdp_mlp.npz")) <= biggest


@pytest.mark.parametrize("N", [3, 4])
def test_restatement_equals_fixture(fx, N):
    st = S.SimState()
    params = [(W.copy(), b.copy()) for W, b in S.layer_params()]
    for w in range(2):
        for k in range(N):
            st.micro_step(S.grads(w, k))
            for what in ("e", "buf", "s"):
                np.testing.assert_array_equal(st.flat(what), fx[f"n{N}_w{w}_k{k}_{what}"], err_msg=f"{what} w{w} k{k}")
        st.update(params, N, S.LR)
        np.testing.assert_array_equal(_flat_params(params), fx[f"n{N}_w{w}_p"])
        st.zero()
        assert not st.flat("buf").any() and not st.flat("s").any() and st.flat("e").any()


def test_fixture_holds_ties_saturation_and_the_set_zero_row(fx):
    s0 = fx["n3_w0_k0_s"]
    assert s0[0] == 1.0                                             # the row whose max is 127
    e0 = fx["n3_w0_k0_e"][:6]
    np.testing.assert_array_equal(e0, np.array([0, 0.5, -0.5, 0.5, -0.5, 0.5], np.float32))  # ties to even
    step1 = fx["n3_w0_k1_buf"] - fx["n3_w0_k0_buf"]
    assert step1.min() == -128 and step1.max() == 127               # 3.5 x: saturated
    zrow = 5 * 13 + 5 + 64                                          # layer 1, row 1
    tiny = np.float32(1e-8) / np.float32(127)
    assert s0[5 + 1 + 1] == tiny and fx["n3_w0_k2_s"][5 + 1 + 1] == tiny  # set once, kept
    assert not fx["n3_w0_k1_buf"][zrow: zrow + 64].any()
    assert set(np.abs(fx["n3_w0_k2_buf"][zrow: zrow + 64]).tolist()) <= {127.0, 128.0}
    for k in (1, 2):                                                 # the scales of a window do not move
        np.testing.assert_array_equal(fx[f"n3_w0_k{k}_s"], s0)
    assert not np.array_equal(fx["n3_w1_k0_s"], s0)                  # ... and are taken anew after zeroing


def test_division_differs_from_reciprocal_for_n3(fx):
    """What the fixture pins: s / N, not s * (1 / N)."""
    s = fx["n3_w0_k0_s"]
    assert ((s / np.float32(3)).astype(np.float32) != (s * (np.float32(1) / np.float32(3))).astype(np.float32)).any()


# ------------------------------------------------------------------ ABI
def test_header_binding_and_library_agree(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12 and lib.dqrm_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.dqrm_dense_ec_accumulate.argtypes) == 6 and len(lib.dqrm_dense_sim_update.argtypes) == 6
    assert lib.dqrm_dense_sim_update.argtypes[3] is C.c_int and lib.dqrm_dense_sim_update.argtypes[4] is C.c_float
    assert "SimulatedDenseBuffers" in dq.__all__ and dq.SimulatedDenseBuffers is SimulatedDenseBuffers


def _fake_set(num_channels=7):
    """A valid dqrm_dense_set over made-up device addresses: every call on it must stop in validation."""
    s = L.DenseSet()
    s.num_channels, s.max_len, s.total_elems = num_channels, 64, 64 * num_channels
    s.grad, s.param, s.len, s.wire_off = 0x100000, 0x200000, 0x300000, 0x400000
    return s


def test_validation_before_any_launch(lib):
    s = _fake_set()
    SC, E, B = 0x500000, 0x600000, 0x700000
    inv = L.DQRM_E_INVALID
    assert lib.dqrm_dense_ec_accumulate(None, 8, SC, E, B, None) == inv and b"null dense set" in lib.dqrm_last_error()
    assert lib.dqrm_dense_sim_update(None, SC, B, 3, 0.1, None) == inv and b"null dense set" in lib.dqrm_last_error()
    for bits in (-1, 0, 1, 17, 32):
        assert lib.dqrm_dense_ec_accumulate(C.byref(s), bits, SC, E, B, None) == inv, bits
        assert b"bits must be 2..16" in lib.dqrm_last_error()
    for args in ((None, E, B), (SC, None, B), (SC, E, None)):
        assert lib.dqrm_dense_ec_accumulate(C.byref(s), 8, *args, None) == inv, args
        assert b"null scale, err or buf" in lib.dqrm_last_error()
    for args in ((None, B), (SC, None)):
        assert lib.dqrm_dense_sim_update(C.byref(s), *args, 3, 0.1, None) == inv, args
        assert b"null scale or buf" in lib.dqrm_last_error()
    for n in (0, -1):
        assert lib.dqrm_dense_sim_update(C.byref(s), SC, B, n, 0.1, None) == inv, n
        assert b"num_gpus < 1" in lib.dqrm_last_error()
    s.grad = None  # a null channel table
    assert lib.dqrm_dense_ec_accumulate(C.byref(s), 8, SC, E, B, None) == inv
    assert lib.dqrm_dense_sim_update(C.byref(s), SC, B, 3, 0.1, None) == inv


def test_empty_set_is_ok(lib):
    s = L.DenseSet()  # num_channels == 0: nothing to do, no pointer looked at
    assert lib.dqrm_dense_ec_accumulate(C.byref(s), 8, None, None, None, None) == L.DQRM_OK
    assert lib.dqrm_dense_sim_update(C.byref(s), None, None, 3, 0.1, None) == L.DQRM_OK
    assert lib.dqrm_dense_ec_accumulate(C.byref(s), 1, None, None, None, None) == L.DQRM_E_INVALID
    assert lib.dqrm_dense_sim_update(C.byref(s), None, None, 0, 0.1, None) == L.DQRM_E_INVALID


# ------------------------------------------------------------------ SimulatedDenseBuffers on the CPU
def _set_grads(layers, gs):
    for l, (gW, gb) in zip(layers, gs):
        l.weight.grad = torch.from_numpy(gW.copy())
        l.bias.grad = torch.from_numpy(gb.copy())


def test_buffers_through_injected_kernels_equal_fixture(fx):
    layers = S.torch_layers()
    ch = DenseChannels(layers)
    k = S.NumpySimKernels(ch)
    sb = SimulatedDenseBuffers(layers, grad_bits=8, kernels=k)
    assert sb.scale.shape == (ch.num_channels,) and sb.err.shape == sb.buf.shape == (ch.total_elems,)
    N = 3
    for w in range(2):
        for j in range(N):
            _set_grads(layers, S.grads(w, j))
            sb.accumulate()
            np.testing.assert_array_equal(sb.err.numpy(), fx[f"n{N}_w{w}_k{j}_e"])
            np.testing.assert_array_equal(sb.buf.numpy(), fx[f"n{N}_w{w}_k{j}_buf"])
            np.testing.assert_array_equal(sb.scale.numpy(), fx[f"n{N}_w{w}_k{j}_s"])
        assert sb.micro_steps == N
        sb.update(S.LR, N)
        got = _flat_params([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in layers])
        np.testing.assert_array_equal(got, fx[f"n{N}_w{w}_p"])
        sb.zero()
        assert sb.micro_steps == 0
    assert k.calls[:4] == ["prepare", "ec_accumulate", "prepare", "ec_accumulate"] and "sim_update" in k.calls


def test_buffers_views_names_versions_and_zeroing():
    layers = S.torch_layers()
    names = [[n for n, _ in l.named_buffers()] for l in layers]
    keys = [list(l.state_dict().keys()) for l in layers]
    layers[2].error_compensation_bias.fill_(0.25)  # a layer's own error compensation is taken over
    sb = SimulatedDenseBuffers(layers, kernels=S.NumpySimKernels(DenseChannels(layers)))
    ch = sb.channels
    assert float(sb.err[int(ch.wire_off[ch.bias_index[2]])]) == 0.25
    layers[2].error_compensation_bias.zero_()
    assert not sb.err.any()                       # ... as a view from then on
    _set_grads(layers, S.grads(0, 0))
    sb.accumulate()

    def check_views():
        for l, ws, bi in zip(layers, ch.weight_slices, ch.bias_index):
            w0, b0 = int(ch.wire_off[ws.start]), int(ch.wire_off[bi])
            o, i = l.weight.shape
            assert l.weight_scaling_factor.shape == (o,) and l.weight_scaling_factor.data_ptr() == sb.scale[ws].data_ptr()
            assert l.bias_scaling_factor.data_ptr() == sb.scale[bi].data_ptr()
            assert l.error_compensation_weight.shape == (o, i) and l.weight_grad_buffer.shape == (o, i)
            assert l.error_compensation_weight.data_ptr() == sb.err[w0:].data_ptr()
            assert l.error_compensation_bias.data_ptr() == sb.err[b0:].data_ptr()
            assert l.weight_grad_buffer.data_ptr() == sb.buf[w0:].data_ptr()
            assert l.bias_grad_buffer.data_ptr() == sb.buf[b0:].data_ptr() and l.bias_grad_buffer.shape == (o,)
            assert "weight_grad_buffer" not in l._buffers and "bias_grad_buffer" not in l._buffers

    check_views()
    assert [[n for n, _ in l.named_buffers()] for l in layers] == names
    assert [list(l.state_dict().keys()) for l in layers] == keys
    assert all(float(l.weight_scaling_factor.min()) > 0 and float(l.bias_scaling_factor) > 0 for l in layers)
    layers[0].weight_scaling_factor = torch.ones(5)  # something replaced an attribute: the next call binds it again
    _set_grads(layers, S.grads(0, 1))
    sb.accumulate()
    check_views()
    vers = [(l.weight._version, l.bias._version) for l in layers]
    epoch = LIN.raw_write_epoch()
    before = [l.weight.detach().clone() for l in layers]
    sb.update(0.1, 2)
    assert LIN.raw_write_epoch() > epoch
    assert all(l.weight._version > v[0] and l.bias._version > v[1] for l, v in zip(layers, vers))
    assert all(not torch.equal(l.weight.detach(), b) for l, b in zip(layers, before))
    e = sb.err.clone()
    assert e.any() and sb.buf.any()
    sb.zero()
    assert not sb.buf.any() and not sb.scale.any() and torch.equal(sb.err, e)  # zeroing keeps e
    check_views()
    assert all(not l.weight_grad_buffer.any() and not l.weight_scaling_factor.any() for l in layers)
    assert torch.equal(layers[3].error_compensation_weight.reshape(-1),
                       e[int(ch.wire_off[ch.weight_slices[3].start]):][:2 * 1100])


def test_buffers_argument_errors():
    layers = S.torch_layers()
    for bits in (1, 17, 32, True):
        with pytest.raises(ValueError, match="grad_bits"):
            SimulatedDenseBuffers(layers, grad_bits=bits, kernels=S.NumpySimKernels(DenseChannels(layers)))
    sb = SimulatedDenseBuffers(layers, kernels=S.NumpySimKernels(DenseChannels(layers)))
    with pytest.raises(ValueError, match="gradient"):
        sb.accumulate()  # no .grad yet
    with pytest.raises(ValueError, match="num_gpus"):
        sb.update(0.1, 0)
    with pytest.raises(L.DQRMError, match="no CPU path"):
        SimulatedDenseBuffers(layers)  # the product's kernels are HIP


# ------------------------------------------------------------------ the three hooks on the CPU
class _Model(nn.Module):
    """bot_l / top_l as create_mlp leaves them (QuantLinear + activations), plus one nn.Linear,
    which the hooks must leave alone; no embedding module."""

    def __init__(self, plain_only=False):
        super().__init__()
        q = S.torch_layers()
        self.emb_l = nn.ModuleList()
        if plain_only:
            self.bot_l = nn.ModuleList([nn.Linear(13, 5), nn.ReLU()])
            self.top_l = nn.ModuleList([nn.Linear(5, 1)])
        else:
            self.bot_l = nn.ModuleList([q[0], nn.ReLU(), q[1], nn.ReLU()])
            self.top_l = nn.ModuleList([q[2], nn.Linear(4, 4), q[3], q[4], nn.Sigmoid()])
        self.qlayers = [] if plain_only else q
        self._dqrm_sim_dense_kernels = S.NumpySimKernels


def _plain_grads(model):
    for m in list(model.bot_l) + list(model.top_l):
        if type(m) is nn.Linear:
            m.weight.grad = torch.ones_like(m.weight)
            m.bias.grad = torch.ones_like(m.bias)


@pytest.mark.parametrize("emb_q,upd_emb", [(True, True), (False, True), (True, False)])
def test_hooks_mlp_branch_on_cpu(fx, emb_q, upd_emb):
    model = _Model()
    plain = model.top_l[1]
    w_plain = plain.weight.detach().clone()
    names = [[n for n, _ in l.named_buffers()] for l in model.qlayers]
    keys = list(model.state_dict().keys())
    H.grad_buffer_zeroing(model)
    assert "_dqrm_sim_dense" not in model.__dict__  # lazy: zeroing before any micro-step makes nothing
    H.weights_update_added_quantization(model, S.LR, 3, emb_q, upd_emb)
    assert "_dqrm_sim_dense" not in model.__dict__
    N = 3
    for w in range(2):
        for k in range(N):
            _set_grads(model.qlayers, S.grads(w, k))
            _plain_grads(model)
            H.grad_buffer_update_added_quantization(model, N, emb_grad_quantized=emb_q)
            sb = model._dqrm_sim_dense[1]
            assert sb.channels.layers == model.qlayers  # bot_l then top_l, QuantLinear only
            assert sb.grad_bits == 8 and sb.micro_steps == k + 1
            np.testing.assert_array_equal(sb.buf.numpy(), fx[f"n{N}_w{w}_k{k}_buf"])
            np.testing.assert_array_equal(sb.err.numpy(), fx[f"n{N}_w{w}_k{k}_e"])
        assert model._dqrm_sim_dense[1] is sb  # one state, kept on the model
        H.weights_update_added_quantization(model, S.LR, N, emb_q, upd_emb)
        got = _flat_params([(l.weight.detach().numpy(), l.bias.detach().numpy()) for l in model.qlayers])
        np.testing.assert_array_equal(got, fx[f"n{N}_w{w}_p"])
        e = sb.err.clone()
        H.grad_buffer_zeroing(model)
        assert not sb.buf.any() and not sb.scale.any() and torch.equal(sb.err, e) and e.any()
        np.testing.assert_array_equal(model.qlayers[3].error_compensation_weight.numpy().reshape(-1),
                                      fx[f"n{N}_w{w}_k{N - 1}_e"][70 + 195 + 524:][:2200])
    assert torch.equal(plain.weight.detach(), w_plain)  # nn.Linear is not this branch's
    assert [[n for n, _ in l.named_buffers()] for l in model.qlayers] == names
    assert list(model.state_dict().keys()) == keys


def test_hooks_without_quantlinear_do_nothing():
    model = _Model(plain_only=True)
    before = [p.detach().clone() for p in model.parameters()]
    _plain_grads(model)
    H.grad_buffer_zeroing(model)
    H.grad_buffer_update_added_quantization(model, 2)
    H.weights_update_added_quantization(model, 0.1, 2)
    H.grad_buffer_zeroing(model)
    assert "_dqrm_sim_dense" not in model.__dict__
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))

    class NoMLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.emb_l = nn.ModuleList()

    m = NoMLP()  # bot_l / top_l absent: as before this branch existed
    H.grad_buffer_update_added_quantization(m, 2)
    H.weights_update_added_quantization(m, 0.1, 2)
    H.grad_buffer_zeroing(m)
    assert "_dqrm_sim_dense" not in m.__dict__


def test_dqrmnet_has_the_route():
    assert callable(dq.DQRMNet.micro_step) and callable(dq.DQRMNet.apply_micro_steps)
    assert "micro_step" in dq.DQRMNet.__doc__ and "Not built" in dq.DQRMNet.__doc__
    np.random.seed(0)
    m = dq.DQRMNet([6, 9], 4, [3, 4], [7, 1], device="cpu")  # a description only
    with pytest.raises(L.DQRMError, match="no CPU path"):
        m.apply_micro_steps(0.1, 2)
    with pytest.raises(ValueError, match="number_of_gpus"):
        m.micro_step(None, None, None, 0)
