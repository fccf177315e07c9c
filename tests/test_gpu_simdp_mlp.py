"""GPU: the MLP half of the simulated-DP buffer (dqrm_dense_ec_accumulate / dqrm_dense_sim_update,
dense.SimulatedDenseBuffers), the three hooks' MLP branch and DQRMNet.micro_step /
apply_micro_steps. Every comparison is bit for bit: against the torch-CPU fixture
(tests/golden/simdp_mlp.npz), the numpy restatement (tests/cpu_simdp.py) and, for the tables, the
oracle functions the module-path test uses.

Shapes. The fixture's layers have channels of 1, 2, 3, 4, 5, 13, 64, 130 and 1100 floats (below a
wave, a wave, two waves and a tail, many iterations) and 20 channels, so five workgroups of four
waves. The model tests use 13-64-16 / 22-130-1 stacks, tables of 6, 700 and 40000 rows, D = 16,
B = 128, N = 3."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import cpu_simdp as S
import gen_inputs as G
import oracle as O

pytestmark = pytest.mark.gpu

ROWS, D, B, N3 = [6, 700, 40000], 16, 128, 3
LN_BOT, LN_TOP = [13, 64, 16], [22, 130, 1]
MODEL_SHAPES = [(64, 13), (16, 64), (130, 22), (1, 130)]
LR = 0.1
FRESH, REQUANT = 1, 2


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "simdp_mlp.npz"))


def _np(t):
    return t.detach().cpu().numpy().copy()


def _eq(got, want, what):
    np.testing.assert_array_equal(_np(got) if isinstance(got, torch.Tensor) else got, want, err_msg=what)


def _flat_params(layers):
    return np.concatenate([np.concatenate([_np(l.weight).reshape(-1), _np(l.bias).reshape(-1)]) for l in layers])


def _set_grads(layers, gs):
    for l, (gW, gb) in zip(layers, gs):
        l.weight.grad = torch.from_numpy(gW.copy()).cuda()
        l.bias.grad = torch.from_numpy(gb.copy()).cuda()


def _run_kernels(dq, N, bits, on_micro_step, on_update, windows=2):
    """The fixture's sequence on the HIP kernels: N micro-steps, update, zeroing, per window."""
    layers = S.torch_layers(device="cuda")
    sb = dq.SimulatedDenseBuffers(layers, grad_bits=bits)
    assert isinstance(sb.kernels, dq.dense.HipDenseKernels)
    for w in range(windows):
        for k in range(N):
            _set_grads(layers, S.grads(w, k))
            sb.accumulate()
            on_micro_step(w, k, sb)
        sb.update(S.LR, N)
        on_update(w, sb, layers)
        e = sb.err.clone()
        sb.zero()
        assert not sb.buf.any() and not sb.scale.any() and torch.equal(sb.err, e)


# (a) the two kernels against the torch-CPU fixture
@pytest.mark.parametrize("N", [3, 4])
def test_kernels_equal_fixture(dq, fx, N):
    def micro(w, k, sb):
        _eq(sb.scale, fx[f"n{N}_w{w}_k{k}_s"], f"s w{w} k{k}")
        _eq(sb.buf, fx[f"n{N}_w{w}_k{k}_buf"], f"buf w{w} k{k}")
        _eq(sb.err, fx[f"n{N}_w{w}_k{k}_e"], f"e w{w} k{k}")

    def upd(w, sb, layers):
        _eq(_flat_params(layers), fx[f"n{N}_w{w}_p"], f"p w{w}")
        _eq(sb.buf, fx[f"n{N}_w{w}_k{N - 1}_buf"], "the update reads only")
        _eq(sb.err, fx[f"n{N}_w{w}_k{N - 1}_e"], "the update reads only")
        _eq(sb.scale, fx[f"n{N}_w{w}_k{N - 1}_s"], "the update reads only")

    _run_kernels(dq, N, 8, micro, upd)


# (b) the same at 4 bits against the numpy restatement
def test_kernels_bits4_equal_restatement(dq):
    st = S.SimState(bits=4)
    params = [(W.copy(), b.copy()) for W, b in S.layer_params()]

    def micro(w, k, sb):
        st.micro_step(S.grads(w, k))
        for what, t in (("s", sb.scale), ("buf", sb.buf), ("e", sb.err)):
            _eq(t, st.flat(what), f"{what} w{w} k{k}")
        assert float(sb.buf.abs().max()) <= 8 * (k + 1)

    def upd(w, sb, layers):
        st.update(params, 3, S.LR)
        _eq(_flat_params(layers), np.concatenate([np.concatenate([W.reshape(-1), b]) for W, b in params]), f"p w{w}")
        st.zero()

    _run_kernels(dq, 3, 4, micro, upd)


# (c) run to run
def test_kernels_same_bits_twice(dq):
    runs = []
    for _ in range(2):
        rec = []
        _run_kernels(dq, 3, 8, lambda w, k, sb: rec.extend([_np(sb.scale), _np(sb.buf), _np(sb.err)]),
                     lambda w, sb, layers: rec.append(_flat_params(layers)), windows=1)
        runs.append(rec)
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ the tables' side, by the oracle
def _oracle_emb_window(Wo, steps, N, lr):
    """One window of the tables by the oracle, as test_simulated_dp_module_api does: steps =
    [(P [T, B], dy [T, B, D])]; Wo is updated in place; returns the first micro-step's scales [T]."""
    s_fwd = [O.table_scale(w, 4) for w in Wo]
    scales = []
    for t in range(len(Wo)):
        rv = [O.emb_bwd_coalesce(ROWS[t], P[t], np.arange(B), dy[t], s_fwd[t])[:2] for P, dy in steps]
        s = O.grad_scale(rv[0][1], 8)  # the first micro-step's scale is kept
        buf = {}
        for r_k, v_k in rv:
            for row, q in zip(r_k.tolist(), O.quantize(v_k, s, 8)):
                buf[row] = buf[row] + q if row in buf else q.copy()
        b_rows = np.array(sorted(buf), dtype=np.int64)
        O.simulated_dp_apply(Wo[t], b_rows, np.stack([buf[r] for r in b_rows.tolist()]), s, N, lr)
        scales.append(s)
    return np.asarray(scales, np.float32)


# (d) the hooks on a small model under autograd
class SmallDLRM(nn.Module):
    """emb_l / bot_l / top_l as DLRM_Net exposes them, the stacks from create_mlp."""

    def __init__(self, dq, Ws):
        super().__init__()
        self.dq = dq
        self.emb_l = dq.QuantEmbeddingBagCollection(ROWS, D, weights=[torch.from_numpy(w) for w in Ws], grad_mode="dp")
        np.random.seed(5)
        self.bot_l = dq.create_mlp(LN_BOT, -1, per_channel=True).cuda()
        self.top_l = dq.create_mlp(LN_TOP, len(LN_TOP) - 2, per_channel=True).cuda()
        self.interact = dq.DotInteraction()

    def forward(self, dense, lS_o, lS_i):
        x = self.dq.apply_mlp(dense, self.bot_l)
        ly = self.emb_l(lS_o, lS_i, layout="btd")
        return self.dq.apply_mlp(self.interact(x, ly), self.top_l)


def test_hooks_mlp_branch_under_autograd(dq):
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients as H

    Ws = G.table_weights(ROWS, D, 21)
    model = SmallDLRM(dq, Ws)
    lins = [l for l in list(model.bot_l) + list(model.top_l) if isinstance(l, dq.QuantLinear)]
    assert [tuple(l.weight.shape) for l in lins] == MODEL_SHAPES
    Wo = [w.copy() for w in Ws]
    params = [(_np(l.weight), _np(l.bias)) for l in lins]
    st = S.SimState(MODEL_SHAPES)
    H.grad_buffer_zeroing(model)
    assert "_dqrm_sim_dense" not in model.__dict__
    steps = []
    rs = np.random.RandomState(3)
    for k in range(N3):
        P = G.pooling_one(ROWS, B, 40 + k, dist="zipf")
        model.zero_grad(set_to_none=True)
        out = model(torch.from_numpy(rs.rand(B, 13).astype(np.float32)).cuda(),
                    torch.arange(B, device="cuda").repeat(len(ROWS), 1), torch.from_numpy(P).cuda())
        out.pow(2).mean().backward()
        steps.append((P, _np(model.emb_l._pending[1].detach().permute(1, 0, 2))))
        st.micro_step([(_np(l.weight.grad), _np(l.bias.grad)) for l in lins])
        H.grad_buffer_update_added_quantization(model, N3)
        sb = model._dqrm_sim_dense[1]
        assert sb.channels.layers == lins and sb.micro_steps == k + 1
        for what, t in (("s", sb.scale), ("buf", sb.buf), ("e", sb.err)):
            _eq(t, st.flat(what), f"{what} k{k}")
    H.weights_update_added_quantization(model, LR, N3)
    st.update(params, N3, LR)
    for i, (l, (W, b)) in enumerate(zip(lins, params)):
        _eq(l.weight, W, f"layer {i} weight")
        _eq(l.bias, b, f"layer {i} bias")
        _eq(l.weight_scaling_factor, st.st[i]["sw"], f"layer {i} weight_scaling_factor")
        _eq(l.error_compensation_bias, st.st[i]["eb"], f"layer {i} error_compensation_bias")
        _eq(l.weight_grad_buffer, st.st[i]["bw"], f"layer {i} weight_grad_buffer")
    scales = _oracle_emb_window(Wo, steps, N3, LR)
    _eq(model.emb_l.emb_scaling_factor, scales, "emb_scaling_factor")
    for t in range(len(ROWS)):
        _eq(model.emb_l.table_weight(t), Wo[t], f"table {t}")
    H.grad_buffer_zeroing(model)
    assert not sb.buf.any() and not sb.scale.any()
    _eq(sb.err, st.flat("e"), "zeroing keeps e")


# (e) DQRMNet.micro_step / apply_micro_steps over two windows
def _net(dq, Ws, seed=9):
    np.random.seed(seed)
    return dq.DQRMNet(ROWS, D, LN_BOT, LN_TOP, per_channel=True, device="cuda",
                      emb_weights=[torch.from_numpy(w.copy()) for w in Ws])


def _data(dq, step):
    rs = np.random.RandomState(500 + step)
    x = torch.from_numpy(rs.standard_normal((B, LN_BOT[0])).astype(np.float32)).cuda()
    t = torch.from_numpy(rs.randint(0, 2, B).astype(np.float32)).cuda()
    P = G.pooling_one(ROWS, B, 70 + step, dist="zipf")
    return x, dq.LookupBatch.pooling_one(torch.from_numpy(P).cuda()), t, P


def test_dqrmnet_micro_steps_two_windows(dq):
    Ws = G.table_weights(ROWS, D, 22)
    m, tw = _net(dq, Ws), _net(dq, Ws)
    lins = m.bot_stack.layers + m.top_stack.layers
    assert [tuple(l.weight.shape) for l in lins] == MODEL_SHAPES
    Wo = [w.copy() for w in Ws]
    params = [(_np(l.weight), _np(l.bias)) for l in lins]
    st = S.SimState(MODEL_SHAPES)
    for w in range(2):
        steps = []
        for k in range(N3):
            x, batch, t, P = _data(dq, w * N3 + k)
            E = m.micro_step(x, batch, t, N3)
            if w == 0:  # nothing is written before the first update: a twin's plain step agrees
                tE = tw.train_step(x, batch, t, 0.0, update=False)
                _eq(E, _np(tE), f"loss k{k}")
                _eq(m.emb_grad, _np(tw.emb_grad), f"emb_grad k{k}")
            st.micro_step([(_np(l.weight.grad), _np(l.bias.grad)) for l in lins])
            steps.append((P, _np(m.emb_grad.permute(1, 0, 2))))
            sb = m._sim_dense
            for what, tns in (("s", sb.scale), ("buf", sb.buf), ("e", sb.err)):
                _eq(tns, st.flat(what), f"{what} w{w} k{k}")
        for i, (l, (W, b)) in enumerate(zip(lins, params)):  # a micro-step writes no parameter
            _eq(l.weight, W, f"w{w} layer {i} weight before the update")
        scales = _oracle_emb_window(Wo, steps, N3, LR)
        _eq(m.emb_scaling_factor, scales, f"w{w} emb_scaling_factor")
        epoch = m.tables.write_epoch
        m.apply_micro_steps(LR, N3)
        st.update(params, N3, LR)
        st.zero()
        for i, (l, (W, b)) in enumerate(zip(lins, params)):
            _eq(l.weight, W, f"w{w} layer {i} weight")
            _eq(l.bias, b, f"w{w} layer {i} bias")
            _eq(l.error_compensation_weight, st.st[i]["ew"], f"w{w} layer {i} error_compensation_weight")
        for t_ in range(len(ROWS)):
            _eq(m.tables.table_weight(t_), Wo[t_], f"w{w} table {t_}")
        assert m.bot_stack.is_fresh() and m.top_stack.is_fresh()
        assert m.tables.write_epoch == epoch + 1 and m._prefetched is None
        assert not sb.buf.any() and not sb.scale.any() and not m.emb_scaling_factor.any()
        assert not m._sim_emb.payloads
    x, batch, t, _ = _data(dq, 99)
    assert m.step_launches(batch) == m.step_launches(batch, fresh=True)
    E = m.train_step(x, batch, t, LR)
    assert m._last_flags == FRESH | REQUANT
    assert np.isfinite(_np(E))


def test_dqrmnet_apply_without_requantize_leaves_the_stacks_stale(dq):
    m = _net(dq, G.table_weights(ROWS, D, 23))
    for k in range(2):
        x, batch, t, _ = _data(dq, 200 + k)
        m.micro_step(x, batch, t, 2)
    m.apply_micro_steps(LR, 2, requantize=False)
    assert not m.bot_stack.is_fresh() and not m.top_stack.is_fresh()
    x, batch, t, _ = _data(dq, 202)
    m.train_step(x, batch, t, LR)
    assert m._last_flags == REQUANT


# (f) the error cases
def test_dqrmnet_micro_step_errors(dq):
    m = _net(dq, G.table_weights(ROWS, D, 24))
    with pytest.raises(ValueError, match="0 micro-steps accumulated but num_gpus=3"):
        m.apply_micro_steps(LR, N3)
    x, batch, t, _ = _data(dq, 300)
    m.micro_step(x, batch, t, N3)
    m.micro_step(x, batch, t, N3)
    before = _flat_params(m.bot_stack.layers + m.top_stack.layers)
    W = _np(m.tables.W)
    with pytest.raises(ValueError, match="2 micro-steps accumulated but num_gpus=3"):
        m.apply_micro_steps(LR, N3)
    _eq(_flat_params(m.bot_stack.layers + m.top_stack.layers), before, "a refused update writes nothing")
    _eq(m.tables.W, W, "a refused update writes nothing")
    assert len(m._sim_emb.payloads) == 2 and m._sim_dense.micro_steps == 2
    with pytest.raises(ValueError, match="number_of_gpus"):
        m.micro_step(x, batch, t, 0)
    m.micro_step(x, batch, t, N3)
    m.apply_micro_steps(LR, N3)  # the third one completes the window
    m.quantize_embedding(8)
    with pytest.raises(RuntimeError, match="quantize_embedding"):
        m.micro_step(x, batch, t, N3)
    with pytest.raises(RuntimeError, match="quantize_embedding"):
        m.apply_micro_steps(LR, N3)
