"""GPU: the quantize_activation stack (dqrm_mlp_qact_prepare / _fwd_qact / _bwd_qact, MLPStack).

1. dqrm_mlp_qact_prepare against L calls of dqrm_linear_wquant_qact: out_scale and bias_integer,
   bit for bit (np.testing.assert_array_equal takes NaNs at the same positions as equal).
2. MLPStack: a fresh forward, a non-fresh forward and apply_mlp agree bit for bit on every layer's
   output, the returned scale and every gradient; the stack after sgd_step equals a twin updated by
   hand; and exact data against tests/cpu_act.py's restatement, compared as tests/test_gpu_act.py
   compares it (bit for bit, the Sigmoid's output within cpu_mlp.sigmoid_bound).

Shapes are the smallest at which the kernel can go wrong: one output, a layer of more outputs than
a workgroup has threads (300 > 256), the 16 layers the descriptor list holds, a per-channel last
layer of 65 outputs (no multiple of a wave)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cpu_act as A
import cpu_linear as R
import cpu_mlp as M

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _eq(got, want, what):
    np.testing.assert_array_equal(got.detach().cpu().numpy(), want.detach().cpu().numpy(), err_msg=what)


def _lins(dq, layers):
    return [l for l in layers if isinstance(l, dq.QuantLinear)]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ================================================================== 1. the prepare launch
SHAPES = {
    "chan-out65": dict(ln=[9, 65], per_channel_last=True),
    "13-24-9-1": dict(ln=[13, 24, 9, 1]),
    "13-24-9-1-chan-last": dict(ln=[13, 24, 9, 1], per_channel_last=True),
    "16-layers-of-3": dict(ln=[3] * 17),
    "out300": dict(ln=[7, 300]),
    "zero-weights": dict(ln=[13, 24, 9, 1], zero_layer=1),
}
PREVS = {"2^-3": 2.0 ** -3, "0.0123": 0.0123}


def _prepare_case(dq, ln, per_channel_last=False, zero_layer=None, bias_bit=4, seed=3):
    np.random.seed(seed)
    layers = dq.create_mlp(ln, len(ln) - 2, weight_bit=4, quantize_activation=True).cuda()
    lins = _lins(dq, layers)
    for l in lins:
        l.bias_bit = bias_bit
    if per_channel_last:
        lins[-1].per_channel = True
    if zero_layer is not None:
        with torch.no_grad():
            lins[zero_layer].weight.zero_()
            lins[zero_layer].bias[0] = 0.0  # 0 * (1 / c): a NaN before the clamp where 1 / c is infinite
    return layers, lins


def _per_layer_reference(dq, lins, prev):
    """L calls of dqrm_linear_wquant_qact, each layer's prev the one before's out_scale: the
    out_scales and bias integers they leave (and fresh weight integers and scales)."""
    lib, st = dq._lib.load(), _stream()
    scales, p = [], prev
    for l in lins:
        l._scale_buffer()
        cos = torch.full((1, l.out_features if l.per_channel else 1), SENTINEL, device="cuda")
        dq._lib.check(lib.dqrm_linear_wquant_qact(C.byref(l._c_struct()), p.data_ptr(), cos.data_ptr(), st),
                      "dqrm_linear_wquant_qact")
        scales.append(cos)
        p = cos
    return scales, [l.bias_integer.clone() for l in lins]


@pytest.mark.parametrize("prev", list(PREVS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_prepare_equals_per_layer_wquant_qact(dq, shape, prev):
    lib = dq._lib.load()
    for bias_bit in (4, 8, 16, 32):
        layers, lins = _prepare_case(dq, bias_bit=bias_bit, **SHAPES[shape])
        p = torch.tensor([PREVS[prev]], dtype=torch.float32, device="cuda")
        want_scales, want_bi = _per_layer_reference(dq, lins, p)
        keep = [(l.fc_scaling_factor.clone(), l.weight_integer.clone()) for l in lins]
        stack = dq.MLPStack(layers)
        got_scales = [torch.full_like(s, SENTINEL) for s in want_scales]
        for l in lins:
            l.bias_integer.fill_(SENTINEL)
        arr = (C.c_void_p * len(lins))(*[s.data_ptr() for s in got_scales])
        dq._lib.check(lib.dqrm_mlp_qact_prepare(C.byref(stack._c_struct()), p.data_ptr(), arr, _stream()),
                      "dqrm_mlp_qact_prepare")
        for k, l in enumerate(lins):
            what = f"{shape} prev {prev} bias_bit {bias_bit} layer {k}"
            _eq(got_scales[k], want_scales[k], what + ": out_scale")
            _eq(l.bias_integer, want_bi[k], what + ": bias_integer")
            _eq(l.fc_scaling_factor, keep[k][0], what + ": fc_scaling_factor is only read")
            _eq(l.weight_integer, keep[k][1], what + ": weight_integer is untouched")
            assert not (got_scales[k] == SENTINEL).any()
        nb = 2 ** (bias_bit - 1) - 1
        assert float(torch.cat([b.reshape(-1) for b in want_bi]).nan_to_num().abs().max()) <= nb + 1


def test_prepare_tiny_scale_and_infinite_reciprocal(dq):
    """A zero layer's 1e-8 clamp under an activation scale so small that c underflows to 0: 1 / c is
    infinite and the bias integers are whatever the clamp makes of +-inf and, where the bias is 0,
    of 0 * inf: exactly what the per-layer call leaves."""
    lib = dq._lib.load()
    layers, lins = _prepare_case(dq, bias_bit=8, **SHAPES["zero-weights"])
    p = torch.tensor([1e-38], dtype=torch.float32, device="cuda")
    want_scales, want_bi = _per_layer_reference(dq, lins, p)
    assert float(lins[1].fc_scaling_factor) == float(np.float32(1e-8) / np.float32(7))
    assert float(want_scales[1]) == 0.0
    print("bias integers of the zero layer:", want_bi[1][:4].tolist())
    stack = dq.MLPStack(layers)
    got = [torch.full_like(s, SENTINEL) for s in want_scales]
    for l in lins:
        l.bias_integer.fill_(SENTINEL)
    arr = (C.c_void_p * len(lins))(*[s.data_ptr() for s in got])
    dq._lib.check(lib.dqrm_mlp_qact_prepare(C.byref(stack._c_struct()), p.data_ptr(), arr, _stream()),
                  "dqrm_mlp_qact_prepare")
    for k, l in enumerate(lins):
        _eq(got[k], want_scales[k], f"layer {k}: out_scale")
        _eq(l.bias_integer, want_bi[k], f"layer {k}: bias_integer")


# ================================================================== 2. the stack
STACKS = {"bottom": ([13, 24, 9], -1), "top": ([13, 24, 9, 1], 2)}  # create_mlp's ReLU / Sigmoid placements


def _three(dq, ln, sigmoid_layer, seed=21, n=3):
    out = []
    for _ in range(n):
        np.random.seed(seed)
        out.append(dq.create_mlp(ln, sigmoid_layer, weight_bit=4, quantize_activation=True).cuda())
    return out


def _layer_outputs(dq, stack, x, prev, fresh):
    """dqrm_mlp_fwd_qact on the stack's struct with tensors of the test's own: every layer's y and
    out_scale."""
    lib, lins = dq._lib.load(), stack.layers
    stack._prepare(x)  # sizes the layers' fc_scaling_factor, as every call of the stack does
    B = x.shape[0]
    ys = [torch.full((B, l.out_features), SENTINEL, device="cuda") for l in lins]
    scales = [torch.full((1, 1), SENTINEL, device="cuda") for _ in lins]
    A_ = C.c_void_p * len(lins)
    dq._lib.check(lib.dqrm_mlp_fwd_qact(C.byref(stack._c_struct()), 1 if fresh else 0, x.data_ptr(), prev.data_ptr(),
                                        A_(*[s.data_ptr() for s in scales]), B, A_(*[y.data_ptr() for y in ys]),
                                        _stream()), "dqrm_mlp_fwd_qact")
    return ys, scales


def _autograd(run, layers, x, dy):
    for p in layers.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    y, s = run(xg)
    y.backward(dy)
    grads = [(l.weight.grad.clone(), l.bias.grad.clone()) for l in layers if hasattr(l, "weight")]
    return y.detach(), s, xg.grad, grads


@pytest.mark.parametrize("B", [1, 7, 130])
@pytest.mark.parametrize("name", list(STACKS))
def test_fresh_nonfresh_and_apply_mlp_agree(dq, name, B):
    ln, sig = STACKS[name]
    fresh_l, stale_l, plain_l = _three(dq, ln, sig)
    rs = np.random.RandomState(50 + B)
    x = torch.from_numpy(rs.standard_normal((B, ln[0])).astype(np.float32)).cuda()
    dy = torch.from_numpy(rs.standard_normal((B, ln[-1])).astype(np.float32)).cuda()
    prev = torch.tensor([0.0123], dtype=torch.float32, device="cuda")
    # apply_mlp, every layer's output and scale through forward hooks
    outs = []
    lins = _lins(dq, plain_l)
    hooks = [l.register_forward_hook(lambda m, a, out: outs.append((out[0].detach(), out[1]))) for l in lins]

    def run_plain(xg):
        h, s = xg, prev
        for layer in plain_l:
            if isinstance(layer, dq.QuantLinear):
                h, s = layer(h, s)
            else:
                h = layer(h)
        return h, s

    y_p, s_p, dx_p, g_p = _autograd(run_plain, plain_l, x, dy)
    for hk in hooks:
        hk.remove()
    _eq(y_p, dq.apply_mlp(x, plain_l, prev), "the loop above is apply_mlp")
    fresh, stale = dq.MLPStack(fresh_l), dq.MLPStack(stale_l)
    fresh.requantize()
    assert fresh.is_fresh() and not stale.is_fresh()
    for what, stack, is_fresh in (("fresh", fresh, True), ("not fresh", stale, False)):
        ys, scales = _layer_outputs(dq, stack, x, prev, is_fresh)
        for k, (y_k, s_k) in enumerate(outs[:len(lins)]):
            _eq(ys[k], y_k, f"{what}: layer {k} y")
            _eq(scales[k], s_k, f"{what}: layer {k} out_scale")
        y, s, dx, g = _autograd(lambda xg, st=stack: st(xg, prev), stack.module_list, x, dy)
        assert stack.is_fresh() == is_fresh
        assert tuple(s.shape) == (1, 1) and stack.layers[-1].correct_output_scale is s
        _eq(y, y_p, f"{what}: y")
        _eq(s, s_p, f"{what}: the returned scale")
        _eq(dx, dx_p, f"{what}: dx")
        assert float(dx_p.abs().max()) > 0
        for k, ((dw, db), (pw, pb)) in enumerate(zip(g, g_p)):
            assert float(pw.abs().max()) > 0
            _eq(dw, pw, f"{what}: layer {k} dw")
            _eq(db, pb, f"{what}: layer {k} db")


def test_per_channel_last_layer_and_input_without_grad(dq):
    ln = [13, 24, 65]
    a_l, b_l = _three(dq, ln, -1, n=2)
    for layers in (a_l, b_l):
        _lins(dq, layers)[-1].per_channel = True
    rs = np.random.RandomState(8)
    x = torch.from_numpy(rs.standard_normal((7, 13)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rs.standard_normal((7, 65)).astype(np.float32)).cuda()
    prev = torch.tensor([2.0 ** -3], device="cuda")
    stack = dq.MLPStack(a_l)
    y, s = stack(x, prev)  # x needs no gradient: the first layer's dx is not launched
    y.backward(dy)
    h, sp = x, prev
    for layer in b_l:
        h, sp = layer(h, sp) if isinstance(layer, dq.QuantLinear) else (layer(h), sp)
    h.backward(dy)
    assert tuple(s.shape) == (1, 65)
    _eq(y, h, "y")
    _eq(s, sp, "the per-channel scale")
    for k, (l, r) in enumerate(zip(_lins(dq, a_l), _lins(dq, b_l))):
        _eq(l.weight.grad, r.weight.grad, f"layer {k} dw")
        _eq(l.bias.grad, r.bias.grad, f"layer {k} db")


def test_sgd_step_then_forward_equals_a_twin_updated_by_hand(dq):
    ln, sig = STACKS["top"]
    s_l, t_l = _three(dq, ln, sig, n=2)
    rs = np.random.RandomState(9)
    B, lr = 33, 0.1
    x = torch.from_numpy(rs.standard_normal((B, ln[0])).astype(np.float32)).cuda()
    x2 = torch.from_numpy(rs.standard_normal((B, ln[0])).astype(np.float32)).cuda()
    dy = torch.from_numpy(rs.standard_normal((B, 1)).astype(np.float32)).cuda()
    prev = torch.tensor([0.0123], dtype=torch.float32, device="cuda")
    stack = dq.MLPStack(s_l)
    y, _ = stack(x, prev)
    y.backward(dy)
    dq.apply_mlp(x, t_l, prev).backward(dy)
    stack.sgd_step(lr, requantize=True)
    assert stack.is_fresh()
    with torch.no_grad():
        for p in t_l.parameters():
            p.data.add_(-lr * p.grad)
    for k, (l, r) in enumerate(zip(_lins(dq, s_l), _lins(dq, t_l))):
        _eq(l.weight, r.weight, f"layer {k} weight")
        _eq(l.bias, r.bias, f"layer {k} bias")
    prev2 = torch.tensor([0.0345], dtype=torch.float32, device="cuda")  # the activation scale moves every forward
    y2, s2 = stack(x2, prev2)
    assert stack.is_fresh()
    want = dq.apply_mlp(x2, t_l, prev2)
    _eq(y2, want, "the fresh forward after sgd_step")
    for k, (l, r) in enumerate(zip(_lins(dq, s_l), _lins(dq, t_l))):
        _eq(l.fc_scaling_factor, r.fc_scaling_factor, f"layer {k} fc_scaling_factor")
        _eq(l.weight_integer, r.weight_integer, f"layer {k} weight_integer")
        _eq(l.bias_integer, r.bias_integer, f"layer {k} bias_integer")
        _eq(l.correct_output_scale, r.correct_output_scale, f"layer {k} correct_output_scale")
    _eq(s2, _lins(dq, t_l)[-1].correct_output_scale, "the returned scale")


@pytest.mark.parametrize("ln,sigmoid_layer", [([13, 64, 16], -1), ([27, 32, 1], 1)], ids=["bottom", "top"])
@pytest.mark.parametrize("fresh", [True, False], ids=["fresh", "not-fresh"])
def test_exact_stack_against_the_restatement(dq, ln, sigmoid_layer, fresh):
    """tests/test_gpu_act.py's exact-data comparison (its step 1), on the stack: every scale is a
    power of two and every sum exact in any order, so the ReLU layers' outputs and the ReLU stack's
    gradients are bit for bit the restatement's; the Sigmoid's output is held to
    cpu_mlp.sigmoid_bound."""
    B, bits = 33, 4
    params = A.exact_stack(ln, bits, seed=41 + ln[0])
    x = A.exact_act_input(B, ln[0], seed=43)
    dy = torch.from_numpy((np.random.RandomState(44).randint(-8, 9, (B, ln[-1])) / 8.0).astype(np.float32))
    prev = torch.tensor([A.P_EXACT])
    ref_params = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in params]
    xr = x.clone().requires_grad_(True)
    y_r, seen, zs = A.stack_forward(xr, ref_params, prev, bits, sigmoid_layer)
    y_r.backward(dy)
    np.random.seed(0)
    layers = dq.create_mlp(ln, sigmoid_layer, weight_bit=bits, quantize_activation=True).cuda()
    lins = _lins(dq, layers)
    with torch.no_grad():
        for l, (W, b) in zip(lins, params):
            l.weight.copy_(W)
            l.bias.copy_(b)
    stack = dq.MLPStack(layers)
    if fresh:
        stack.requantize()
    ys, scales = _layer_outputs(dq, stack, x.cuda(), prev.cuda(), fresh)
    for k, (l, (W_r, b_r)) in enumerate(zip(lins, ref_params)):
        sc = R.weight_scale(W_r.detach(), bits, False)
        _eq(l.fc_scaling_factor, sc, f"layer {k} fc_scaling_factor")
        _eq(l.weight_integer, R.SymQuant.apply(W_r.detach(), bits, sc), f"layer {k} weight_integer")
    for k, xi in enumerate(seen):
        assert torch.equal(xi, xi.round()) and float(xi.abs().max()) * R.qmax(bits) * ln[k] < 2 ** 24
        if k == sigmoid_layer:
            sig = torch.sigmoid(zs[k].double())
            err = (ys[k].cpu().double() - sig).abs()
            print(f"layer {k} sigmoid(z): max err {float(err.max()):.3e}")
            assert bool((err <= M.sigmoid_bound(sig)).all()), f"layer {k} sigmoid(z)"
        else:
            _eq(ys[k], torch.relu(zs[k]), f"layer {k} output")
    if sigmoid_layer < 0:
        xg = x.cuda().requires_grad_(True)
        y, s = stack(xg, prev.cuda())
        y.backward(dy.cuda())
        _eq(y, y_r, "y")
        _eq(xg.grad, xr.grad, "x.grad")
        for k, (l, (W_r, b_r)) in enumerate(zip(lins, ref_params)):
            assert float(W_r.grad.abs().max()) > 0
            _eq(l.weight.grad, W_r.grad, f"layer {k} weight.grad")
            _eq(l.bias.grad, b_r.grad, f"layer {k} bias.grad")


def test_stack_errors_on_the_device(dq):
    np.random.seed(0)
    layers = dq.create_mlp([6, 4, 3], -1, quantize_activation=True).cuda()
    stack = dq.MLPStack(layers)
    x = torch.zeros(2, 6, device="cuda")
    with pytest.raises(ValueError, match="prev_act_scaling_factor"):
        stack(x)
    with pytest.raises(ValueError, match="ONE element"):
        stack(x, torch.ones(2, device="cuda"))
    with pytest.raises(ValueError, match="float32 on the input's device"):
        stack(x, torch.ones(1))
    _lins(dq, layers)[0].per_channel = True
    with pytest.raises(ValueError, match="per_channel"):
        stack(x, torch.ones(1, device="cuda"))
    np.random.seed(0)
    plain = dq.MLPStack(dq.create_mlp([6, 4, 3], -1).cuda())
    with pytest.raises(NotImplementedError, match="prev_act_scaling_factor"):
        plain(x, torch.ones(1, device="cuda"))
