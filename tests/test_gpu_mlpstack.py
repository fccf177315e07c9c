"""GPU: MLPStack (dqrm_mlp_fwd / _bwd / _sgd, mlp.py) against tests/cpu_mlpstack.py, tests/cpu_linear.py
and a twin stack built from the same numpy seed that runs apply_mlp and the per-layer calls.

Stacks (cpu_mlpstack.STACKS): A = [13, 32, 16] ReLU, B = [20, 32, 1] sigmoid last, C = [130, 37, 5]
(rows longer than a wave's stride, row counts that are no multiple of 4). B = 33. Every comparison
is bit for bit; np.testing.assert_array_equal takes NaNs at the same positions as equal."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import cpu_linear as R
import cpu_mlpstack as S
import gen_inputs as G

pytestmark = pytest.mark.gpu

PC = {"chan": (True, True), "tensor": (False, False), "mixed": (True, False), "mixed2": (False, True)}
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _build(dq, name, bits=4, pc="chan", seed=31, fp_layer=None):
    """(ModuleList, [QuantLinear]) of stack `name` on the GPU, from one numpy seed."""
    ln, sig = S.STACKS[name]
    np.random.seed(seed)
    layers = dq.create_mlp(ln, sig, weight_bit=bits, per_channel=True).cuda()
    lins = [l for l in layers if isinstance(l, dq.QuantLinear)]
    for l, p in zip(lins, PC[pc]):
        l.per_channel = p
    if fp_layer is not None:
        lins[fp_layer].full_precision_flag = True
    return layers, lins


def _pair(dq, *a, **kw):
    return _build(dq, *a, **kw) + _build(dq, *a, **kw)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _eq(got, want, what):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    want = _np(want) if isinstance(want, torch.Tensor) else want
    np.testing.assert_array_equal(got, want, err_msg=what)


def _set_grads(lins, grads):
    for l, (dw, db) in zip(lins, grads):
        l.weight.grad = torch.from_numpy(dw).cuda()
        l.bias.grad = torch.from_numpy(db).cuda()


def _set_params(l, W, b):
    with torch.no_grad():
        l.weight.copy_(torch.from_numpy(W))
        l.bias.copy_(torch.from_numpy(b))


def _wquant(l):
    """The per-layer quantization, as QuantLinear.forward runs it."""
    l._scale_buffer()
    l._lib.dqrm_linear_wquant(C.byref(l._c_struct()), torch.cuda.current_stream().cuda_stream)


def _reference_update(lins, lr):
    """The reference-style update of a twin: torch's own."""
    for l in lins:
        for p in (l.weight, l.bias):
            p.data.add_(-lr * p.grad)


def _fill_buffers(lins, value=SENTINEL):
    for l in lins:
        if not l.full_precision_flag:
            l._scale_buffer()
        for t in (l.weight_integer, l.bias_integer, l.fc_scaling_factor):
            t.fill_(value)


def _buffers(l):
    return (("fc_scaling_factor", l.fc_scaling_factor), ("weight_integer", l.weight_integer),
            ("bias_integer", l.bias_integer))


def _assert_buffers_equal(lins, tlins, what):
    for k, (l, t) in enumerate(zip(lins, tlins)):
        if l.full_precision_flag:
            continue
        for (name, a), (_, w) in zip(_buffers(l), _buffers(t)):
            _eq(a, w, f"{what}: layer {k} {name}")


def _inputs(name, seed=41):
    ln, _ = S.STACKS[name]
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((S.BATCH, ln[0])).astype(np.float32)).cuda()
    dy = torch.from_numpy(rs.standard_normal((S.BATCH, ln[-1])).astype(np.float32)).cuda()
    return x, dy


def _shapes(lins):
    return [tuple(l.weight.shape) for l in lins]


# ------------------------------------------------------------------ 1. dqrm_mlp_sgd against the restatement
def _sgd_against_restatement(dq, name, bits, pc, fp_layer=None):
    for lr in (0.1, 24.0):
        layers, lins, _, tlins = _pair(dq, name, bits, pc, fp_layer=fp_layer)
        grads = S.random_grads(_shapes(lins), seed=7)
        _set_grads(lins, grads)
        _set_grads(tlins, grads)
        want = [(_np(l.weight), _np(l.bias)) for l in lins]
        stack = dq.MLPStack(layers)
        # without REQUANT: the update alone, no integer buffer or scale is touched
        _fill_buffers(lins)
        stack.sgd_step(lr, requantize=False)
        assert not stack.is_fresh()
        want = [(S.sgd(W, dw, lr), S.sgd(b, db, lr)) for (W, b), (dw, db) in zip(want, grads)]
        for k, (l, (W, b)) in enumerate(zip(lins, want)):
            _eq(l.weight, W, f"lr {lr} layer {k} weight (update only)")
            _eq(l.bias, b, f"lr {lr} layer {k} bias (update only)")
            for bname, t in _buffers(l):
                assert bool((t == SENTINEL).all()), f"lr {lr} layer {k}: {bname} written without REQUANT"
        # with REQUANT, a second step on top
        stack.sgd_step(lr)
        assert stack.is_fresh()
        want = [(S.sgd(W, dw, lr), S.sgd(b, db, lr)) for (W, b), (dw, db) in zip(want, grads)]
        for _ in range(2):
            _reference_update(tlins, lr)
        for k, (l, t, (W, b)) in enumerate(zip(lins, tlins, want)):
            _eq(l.weight, W, f"lr {lr} layer {k} weight")
            _eq(l.bias, b, f"lr {lr} layer {k} bias")
            _eq(t.weight, W, f"lr {lr} layer {k} twin weight")
            _eq(t.bias, b, f"lr {lr} layer {k} twin bias")
            if l.full_precision_flag:
                for bname, buf in _buffers(l):
                    assert bool((buf == SENTINEL).all()), f"lr {lr} layer {k}: full-precision {bname} written"
                continue
            s, wi, bi = S.quantize(W, b, bits, bool(l.per_channel))
            _eq(l.fc_scaling_factor, s, f"lr {lr} layer {k} scale against cpu_linear.quantize")
            _eq(l.weight_integer, wi, f"lr {lr} layer {k} weight_integer against cpu_linear.quantize")
            _eq(l.bias_integer, bi, f"lr {lr} layer {k} bias_integer against cpu_linear.quantize")
            _wquant(t)
        _assert_buffers_equal(lins, tlins, f"lr {lr} against the twin's dqrm_linear_wquant")


@pytest.mark.parametrize("pc", ["chan", "tensor", "mixed", "mixed2"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sgd_step_against_the_restatement(dq, name, bits, pc):
    _sgd_against_restatement(dq, name, bits, pc)


@pytest.mark.parametrize("name,pc,fp_layer", [("A", "tensor", 0), ("C", "mixed", 1), ("B", "chan", 0)])
def test_sgd_step_leaves_a_full_precision_layers_buffers_alone(dq, name, pc, fp_layer):
    _sgd_against_restatement(dq, name, 4, pc, fp_layer=fp_layer)


def test_update_is_two_roundings_not_one(dq):
    """The GPU result is the separately rounded form where it differs from a single rounding."""
    layers, lins = _build(dq, "C")
    grads = S.random_grads(_shapes(lins), seed=7)
    _set_grads(lins, grads)
    W = _np(lins[0].weight)
    dq.MLPStack(layers).sgd_step(0.1)
    two, one = S.sgd(W, grads[0][0], 0.1), S.sgd_single_rounding(W, grads[0][0], 0.1)
    assert int((two != one).sum()) >= 1
    _eq(lins[0].weight, two, "weight")


def test_sgd_step_rejects_bad_gradients_and_writes_nothing(dq):
    layers, lins = _build(dq, "A")
    stack = dq.MLPStack(layers)
    grads = S.random_grads(_shapes(lins), seed=7)
    before = [(_np(l.weight), _np(l.bias)) for l in lins]

    def rejected(match):
        with pytest.raises(ValueError, match=match):
            stack.sgd_step(0.1)
        for k, (l, (W, b)) in enumerate(zip(lins, before)):
            _eq(l.weight, W, f"layer {k} weight")
            _eq(l.bias, b, f"layer {k} bias")

    rejected("layer 0's weight.grad is None")
    _set_grads(lins, grads)
    lins[1].bias.grad = None
    rejected("layer 1's bias.grad is None")
    _set_grads(lins, grads)
    lins[1].weight.grad = torch.zeros(32, 16, device="cuda").t()  # the right shape, not contiguous
    rejected("layer 1's weight.grad must be a contiguous float32")
    # (torch itself refuses to give a float32 parameter a gradient of another dtype)
    _set_grads(lins, grads)
    with pytest.raises(ValueError, match="grad_scales"):
        stack.sgd_step(0.1, grad_scales=[torch.ones(33, device="cuda")])
    with pytest.raises(ValueError, match="grad_scales"):
        stack.sgd_step(0.1, grad_scales=[torch.ones(33, device="cuda"), torch.ones(16, device="cuda")])


# ------------------------------------------------------------------ 2. edge rows
@pytest.mark.parametrize("pc", ["chan", "tensor"])
def test_rows_that_become_zero_take_the_clamp(dq, pc):
    """g = W / lr with lr a power of two: W + (-lr) * g == 0 exactly. Per channel one row of layer
    0, per tensor the whole of layer 1 (the clamp acts on the tensor's maximum there)."""
    lr = 0.5
    layers, lins, _, tlins = _pair(dq, "A", 4, pc)
    grads = S.random_grads(_shapes(lins), seed=8)
    if pc == "chan":
        k, rows = 0, [5]
    else:
        k, rows = 1, list(range(16))
    grads[k][0][rows] = _np(lins[k].weight)[rows] / np.float32(lr)
    grads[k][1][rows] = _np(lins[k].bias)[rows] / np.float32(lr)
    _set_grads(lins, grads)
    _set_grads(tlins, grads)
    dq.MLPStack(layers).sgd_step(lr)
    _reference_update(tlins, lr)
    for t in tlins:
        _wquant(t)
    l = lins[k]
    assert bool((l.weight[rows] == 0).all()) and bool((l.bias[rows] == 0).all())
    s = _np(l.fc_scaling_factor)
    assert (s[rows] if pc == "chan" else s)[0] == np.float32(1e-8) / np.float32(7)
    assert bool((l.weight_integer[rows] == 0).all()) and bool((l.bias_integer[rows] == 0).all())
    for j, (a, t) in enumerate(zip(lins, tlins)):
        _eq(a.weight, t.weight, f"layer {j} weight")
        sq, wi, bi = S.quantize(_np(a.weight), _np(a.bias), 4, pc == "chan")
        _eq(a.fc_scaling_factor, sq, f"layer {j} scale")
        _eq(a.weight_integer, wi, f"layer {j} weight_integer")
        _eq(a.bias_integer, bi, f"layer {j} bias_integer")
    _assert_buffers_equal(lins, tlins, "against the twin")


@pytest.mark.parametrize("pc", ["chan", "tensor"])
def test_round_half_even_ties_after_the_update(dq, pc):
    """Layer 0 starts at 2 * T and receives g = T / lr, lr = 0.5: the update lands exactly on T,
    cpu_mlpstack.tie_case's weights, whose quotients by the scale are integers and exact halves."""
    lr = 0.5
    layers, lins, _, tlins = _pair(dq, "A", 4, pc)
    T_W, T_b = S.tie_case(32, 13, 4, seed=3)
    if pc == "tensor":  # one scale for the tensor: give every row the same power of two
        s_row = np.abs(T_W).max(axis=1, keepdims=True) / 7
        T_W, T_b = (T_W / s_row / 8).astype(np.float32), (T_b / s_row[:, 0] / 8).astype(np.float32)
    grads = S.random_grads(_shapes(lins), seed=9)
    grads[0] = ((T_W / np.float32(lr)).astype(np.float32), (T_b / np.float32(lr)).astype(np.float32))
    for l in (lins[0], tlins[0]):
        _set_params(l, 2 * T_W, 2 * T_b)
    _set_grads(lins, grads)
    _set_grads(tlins, grads)
    dq.MLPStack(layers).sgd_step(lr)
    _reference_update(tlins, lr)
    _wquant(tlins[0])
    l = lins[0]
    _eq(l.weight, T_W, "the update lands on the tie case")
    _eq(l.bias, T_b, "the update lands on the tie case (bias)")
    s, wi, bi = S.quantize(T_W, T_b, 4, pc == "chan")
    q = T_W / s.reshape(-1, 1)
    ties = np.abs(q - np.floor(q)) == 0.5
    assert ties.sum() > 20
    got = _np(l.weight_integer)
    assert np.array_equal(got[ties] % 2, np.zeros(int(ties.sum()), np.float32))  # half to even
    _eq(l.fc_scaling_factor, s, "scale")
    _eq(got, wi, "weight_integer")
    _eq(l.bias_integer, bi, "bias_integer")
    _assert_buffers_equal(lins[:1], tlins[:1], "against the twin")


@pytest.mark.parametrize("pc", ["chan", "tensor"])
def test_a_nan_weight_is_treated_as_wquant_treats_it(dq, pc):
    layers, lins, _, tlins = _pair(dq, "A", 4, pc)
    grads = S.random_grads(_shapes(lins), seed=10)
    _set_grads(lins, grads)
    _set_grads(tlins, grads)
    for l in (lins[0], tlins[0]):
        l.weight.data[3, 5] = float("nan")
    dq.MLPStack(layers).sgd_step(0.1)
    _reference_update(tlins, 0.1)
    for t in tlins:
        _wquant(t)
    assert bool(torch.isnan(lins[0].weight[3, 5])) and int(torch.isnan(lins[0].weight).sum()) == 1
    assert bool(torch.isfinite(lins[0].fc_scaling_factor).all())  # fmaxf drops the NaN from the maximum
    for j, (a, t) in enumerate(zip(lins, tlins)):
        _eq(a.weight, t.weight, f"layer {j} weight")
        _eq(a.bias, t.bias, f"layer {j} bias")
    _assert_buffers_equal(lins, tlins, "against the twin")


# ------------------------------------------------------------------ 3. the gscale form
def test_grad_scales_equal_dqrm_dense_update(dq):
    from deep_quantized_recommendation_model_dqrm_amd.dense import DenseChannels, HipDenseKernels

    lr = 0.1
    layers, lins, _, tlins = _pair(dq, "A")
    grads = S.random_grads(_shapes(lins), seed=11)
    _set_grads(lins, grads)
    _set_grads(tlins, grads)
    before = [(_np(l.weight), _np(l.bias)) for l in lins]
    ch = DenseChannels(tlins)
    rs = np.random.RandomState(12)
    s = torch.from_numpy(rs.uniform(0.01, 2.0, ch.num_channels).astype(np.float32)).cuda()
    k = HipDenseKernels(ch, "cuda")
    k.prepare()
    k.update(s, lr)
    # a layer's channels are its rows, then its bias: gscale[l] is that slice of the channel scales
    scales = [s[ws.start:bi + 1].contiguous() for ws, bi in zip(ch.weight_slices, ch.bias_index)]
    stack = dq.MLPStack(layers)
    stack.sgd_step(lr, grad_scales=scales)
    assert stack.is_fresh()
    for j, (a, t, (W, b), (dw, db), sc) in enumerate(zip(lins, tlins, before, grads, scales)):
        sc = _np(sc)
        assert not np.array_equal(_np(a.weight), W)
        _eq(a.weight, t.weight, f"layer {j} weight against dqrm_dense_update")
        _eq(a.bias, t.bias, f"layer {j} bias against dqrm_dense_update")
        _eq(a.weight, S.sgd(W, dw, lr, sc[:-1].reshape(-1, 1)), f"layer {j} weight against the restatement")
        _eq(a.bias, S.sgd(b, db, lr, sc[-1]), f"layer {j} bias against the restatement")
        _wquant(t)
    _assert_buffers_equal(lins, tlins, "against the twin")


# ------------------------------------------------------------------ 4. forward / backward == layer by layer
def _grad_fn_names(t):
    names, todo, done = [], [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in done:
            continue
        done.add(f)
        names.append(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


@pytest.mark.parametrize("x_grad", [True, False], ids=["x-grad", "x-no-grad"])
@pytest.mark.parametrize("name,pc", [("A", "chan"), ("B", "mixed"), ("C", "tensor"), ("C", "chan")])
def test_stack_forward_backward_equal_the_layer_by_layer_path(dq, name, pc, x_grad):
    layers, lins, twin, tlins = _pair(dq, name, 4, pc)
    x, dy = _inputs(name)
    stack = dq.MLPStack(layers)
    xs, xt = x.clone().requires_grad_(x_grad), x.clone().requires_grad_(x_grad)
    ys = stack(xs)
    yt = dq.apply_mlp(xt, twin)
    names = _grad_fn_names(ys)
    assert names.count("_StackFnBackward") == 1 and "_LinearFnBackward" not in names
    assert _grad_fn_names(yt).count("_LinearFnBackward") == len(lins)
    ys.backward(dy)
    yt.backward(dy)
    _eq(ys, yt, "y")
    assert bool(torch.isfinite(ys).all())
    if x_grad:
        _eq(xs.grad, xt.grad, "x.grad")
    else:
        assert xs.grad is None
    for k, (a, t) in enumerate(zip(lins, tlins)):
        _eq(a.weight.grad, t.weight.grad, f"layer {k} weight.grad")
        _eq(a.bias.grad, t.bias.grad, f"layer {k} bias.grad")
        assert float(a.weight.grad.abs().max()) > 0
    _assert_buffers_equal(lins, tlins, "the buffers the forward wrote")
    # a layer called on its own afterwards sees the buffers the stack's kernels wrote
    _eq(lins[0](x)[0], tlins[0](x)[0], "layer 0 on its own")


def test_empty_batch(dq):
    layers, lins = _build(dq, "A")
    stack = dq.MLPStack(layers)
    x = torch.empty(0, 13, device="cuda", requires_grad=True)
    y = stack(x)
    assert tuple(y.shape) == (0, 16)
    y.sum().backward()
    assert tuple(x.grad.shape) == (0, 13)
    for l in lins:
        assert bool((l.weight.grad == 0).all()) and bool((l.bias.grad == 0).all())


# ------------------------------------------------------------------ 5. three training steps, 8. determinism
def _train(dq, name, pc, use_stack, steps=3, lr=0.1):
    """Per step: y, the grads, and after the update W, b, the integers and the scales."""
    layers, lins = _build(dq, name, 4, pc)
    stack = dq.MLPStack(layers) if use_stack else None
    out = []
    for step in range(steps):
        x, dy = _inputs(name, seed=50 + step)
        for p in layers.parameters():
            p.grad = None
        if use_stack:
            assert stack.is_fresh() == (step > 0)
            y = stack(x)
        else:
            y = dq.apply_mlp(x, layers)
        y.backward(dy)
        rec = [("y", _np(y))]
        rec += [(f"layer {k} {n}.grad", _np(p.grad)) for k, l in enumerate(lins)
                for n, p in (("weight", l.weight), ("bias", l.bias))]
        if use_stack:
            stack.sgd_step(lr)
        else:
            _reference_update(lins, lr)
            for l in lins:
                _wquant(l)
        for k, l in enumerate(lins):
            rec += [(f"layer {k} weight", _np(l.weight)), (f"layer {k} bias", _np(l.bias))]
            rec += [(f"layer {k} {n}", _np(t)) for n, t in _buffers(l)]
        out.append(rec)
    return out


@pytest.mark.parametrize("name,pc", [("A", "chan"), ("B", "tensor"), ("C", "mixed")])
def test_three_training_steps_equal_the_reference_style_loop(dq, name, pc):
    got, want = _train(dq, name, pc, True), _train(dq, name, pc, False)
    for step, (g, w) in enumerate(zip(got, want)):
        assert [n for n, _ in g] == [n for n, _ in w]
        for (what, a), (_, b) in zip(g, w):
            _eq(a, b, f"step {step}: {what}")
    assert not np.array_equal(got[0][0][1], got[2][0][1])


def test_training_steps_are_deterministic(dq):
    first, second = _train(dq, "C", "mixed", True), _train(dq, "C", "mixed", True)
    for step, (g, w) in enumerate(zip(first, second)):
        for (what, a), (_, b) in zip(g, w):
            _eq(a, b, f"step {step}: {what} run to run")


# ------------------------------------------------------------------ 6. a fresh forward reads the integers
@pytest.mark.parametrize("how", ["sgd_step", "requantize"])
def test_fresh_forward_reads_the_integers_and_does_not_rewrite_them(dq, how):
    layers, lins, twin, tlins = _pair(dq, "A")
    x, dy = _inputs("A")
    stack = dq.MLPStack(layers)
    if how == "sgd_step":
        grads = S.random_grads(_shapes(lins), seed=13)
        _set_grads(lins, grads)
        _set_grads(tlins, grads)
        stack.sgd_step(0.1)
        _reference_update(tlins, 0.1)
    else:
        stack.requantize()
    assert stack.is_fresh()
    want = dq.apply_mlp(x, twin)
    _eq(stack(x), want, "fresh forward")
    assert stack.is_fresh()
    lins[0].weight_integer.fill_(float("nan"))
    y = stack(x)
    assert bool(torch.isnan(y).all()), "a fresh forward must read weight_integer as it stands"
    assert bool(torch.isnan(lins[0].weight_integer).all()), "a fresh forward must not rewrite weight_integer"
    stack.invalidate()
    assert not stack.is_fresh()
    y = stack(x)
    assert bool(torch.isfinite(y).all())
    _eq(y, want, "after invalidate()")
    assert not stack.is_fresh()  # only sgd_step and requantize make it fresh


# ------------------------------------------------------------------ 7. staleness is caught
def _fresh_pair(dq):
    layers, lins, twin, tlins = _pair(dq, "A")
    grads = S.random_grads(_shapes(lins), seed=14)
    _set_grads(lins, grads)
    _set_grads(tlins, grads)
    stack = dq.MLPStack(layers)
    stack.sgd_step(0.1)
    _reference_update(tlins, 0.1)
    assert stack.is_fresh()
    return stack, layers, lins, twin, tlins


def _add_one(layers, lins):
    with torch.no_grad():
        lins[1].weight.add_(1)


def _load_state_dict(layers, lins):
    sd = {k: (v * 0.5 if k.endswith("weight") else v.clone()) for k, v in layers.state_dict().items()}
    layers.load_state_dict(sd)


def _replace_data(layers, lins):
    lins[0].weight.data = (lins[0].weight.data * 0.25).contiguous()


def _change_bits(layers, lins):
    lins[1].weight_bit = 8


@pytest.mark.parametrize("change", [_add_one, _load_state_dict, _replace_data, _change_bits],
                         ids=["add_", "load_state_dict", "replace-data", "weight_bit"])
def test_staleness_is_caught(dq, change):
    stack, layers, lins, twin, tlins = _fresh_pair(dq)
    x, _ = _inputs("A")
    change(layers, lins)
    change(twin, tlins)
    assert not stack.is_fresh()
    y, want = stack(x), dq.apply_mlp(x, twin)
    assert bool(torch.isfinite(y).all())
    _eq(y, want, "the forward after the change")
    _assert_buffers_equal(lins, tlins, "the buffers after the change")


class StackDLRM(nn.Module):
    """test_gpu_mlp.FusedMLPDLRM (fused): emb_l / bot_l / top_l as DLRM_Net exposes them;
    use_stacks runs the MLPs through an MLPStack each, otherwise through apply_mlp."""

    def __init__(self, dq, rows, D, Ws, use_stacks):
        super().__init__()
        self.dq = dq
        self.emb_l = dq.QuantEmbeddingBagCollection(rows, D, weights=[torch.from_numpy(w) for w in Ws],
                                                    grad_mode="dp")

        def ql(i, o):
            q = dq.QuantLinear(weight_bit=4, bias_bit=4, per_channel=True)
            q.set_param(nn.Linear(i, o).cuda())
            return q

        Z = D * (len(rows) + 1)
        self.bot_l = nn.ModuleList([ql(13, 24), nn.ReLU(), ql(24, D), nn.ReLU()])
        self.top_l = nn.ModuleList([ql(Z, 20), nn.ReLU(), ql(20, 1)])
        assert dq.fuse_activations(self.bot_l) == 2 and dq.fuse_activations(self.top_l) == 1
        self.stacks = (dq.MLPStack(self.bot_l), dq.MLPStack(self.top_l)) if use_stacks else None

    def mlp(self, x, which):
        if self.stacks is not None:
            return self.stacks[which](x)
        return self.dq.apply_mlp(x, (self.bot_l, self.top_l)[which])

    def forward(self, dense, lS_o, lS_i):
        x = self.mlp(dense, 0)
        ly = self.emb_l(lS_o, lS_i, layout="btd")
        return self.mlp(torch.cat([x.unsqueeze(1), ly], dim=1).flatten(1), 1)


def test_staleness_after_the_dp_hooks(dq):
    """The hooks' dense update writes the weights through raw pointers: the package's raw-write
    epoch makes the stacks quantize again."""
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients_parallel_comm as H

    rows, D, B, lr = [4, 300], 16, 96, 0.1
    lS_i = torch.from_numpy(G.pooling_one(rows, B, 20)).cuda()
    lS_o = torch.arange(B, device="cuda").repeat(len(rows), 1)
    torch.manual_seed(1)
    dense = torch.rand(B, 13, device="cuda")
    z = torch.rand(B, D * 3, device="cuda")
    outs = []
    for use_stacks in (True, False):
        torch.manual_seed(0)
        model = StackDLRM(dq, rows, D, G.table_weights(rows, D, 12), use_stacks)
        mlp = [l for l in list(model.bot_l) + list(model.top_l) if isinstance(l, dq.QuantLinear)]
        # one step of the MLPs alone, after which the stacks are fresh
        (model.mlp(dense, 0).pow(2).mean() + model.mlp(z, 1).pow(2).mean()).backward()
        if use_stacks:
            for s in model.stacks:
                s.sgd_step(lr)
                assert s.is_fresh()
        else:
            _reference_update(mlp, lr)
        # one DP iteration at world size 1
        H.clear_gradients(model)
        model(dense, lS_o, lS_i).pow(2).mean().backward()
        before = [_np(l.weight) for l in mlp]
        H.grad_update_parallel_comm(model, 1, emb_grad_quantized=True, num_bits=8, mlp_layer_quantized=True)
        H.weight_update_parallel_comm(model, lr, emb_grad_quantized=True, num_gpus=1, mlp_layer_quantized=True)
        assert all(not np.array_equal(_np(l.weight), W0) for l, W0 in zip(mlp, before))
        if use_stacks:
            assert not any(s.is_fresh() for s in model.stacks)
        y = model(dense, lS_o, lS_i)
        outs.append([_np(y)] + [_np(t) for l in mlp for t in (l.weight, l.bias, l.weight_integer,
                                                               l.fc_scaling_factor)])
    for k, (a, w) in enumerate(zip(*outs)):
        _eq(a, w, f"stacks against apply_mlp after the hooks (tensor {k})")
    assert np.isfinite(outs[0][0]).all()


# ------------------------------------------------------------------ 9. graph capture
def test_a_training_step_in_a_captured_graph(dq):
    """Forward, torch.autograd.grad and sgd_step of a fresh stack captured on one stream; two
    replays leave the parameters and outputs of two eager steps on a twin."""
    lr = 0.1
    layers, lins, twin, tlins = _pair(dq, "A", 4, "mixed")
    stack = dq.MLPStack(layers)
    params = [p for l in lins for p in (l.weight, l.bias)]
    tparams = [p for l in tlins for p in (l.weight, l.bias)]
    xs = [_inputs("A", seed=60 + k)[0] for k in range(3)]
    dy = _inputs("A")[1]
    x = xs[0].clone()

    def step():
        y = stack(x)
        grads = torch.autograd.grad(y, params, dy)
        for p, g in zip(params, grads):
            p.grad = g
        stack.sgd_step(lr)
        return (y,) + grads

    def twin_step(xv):
        y = dq.apply_mlp(xv, twin)
        grads = torch.autograd.grad(y, tparams, dy)
        for p, g in zip(tparams, grads):
            p.data.add_(-lr * g)
        return (y,) + grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # the eager warm-up step: the stack is fresh afterwards
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    twin_step(xs[0])
    assert stack.is_fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for xv in xs[1:]:
        x.copy_(xv)
        for t in out:
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = twin_step(xv)
        for a, w, what in zip(out, want, ["y"] + [f"grad {k}" for k in range(len(params))]):
            _eq(a, w, what)
            assert bool(torch.isfinite(a).all())
        for k, (p, t) in enumerate(zip(params, tparams)):
            _eq(p, t, f"parameter {k} after the replay")
    for t in tlins:
        _wquant(t)
    _assert_buffers_equal(lins, tlins, "after the replays")
