"""GPU: QuantAct (act.py over csrc/dqrm_act.hip) and the activation-quantized QuantLinear
(dqrm_linear_wquant_qact / _fwd_qact / _bwd_qact) against the CPU restatement of the reference's
arithmetic (tests/cpu_act.py). Everything is compared bit for bit, with one exception that the
arithmetic forces: a Sigmoid's forward goes through expf, which IEEE does not specify, so it is
held to cpu_mlp.sigmoid_bound as in tests/test_gpu_mlp.py; its backward is compared bit for bit
on a caller-chosen y (the C call) or on the y the kernel wrote (the composition test).

QuantAct shapes: [1,1]; [7,13]; [130,479] (62270 elements: the multi-workgroup range pass, four
partial workgroups, a ragged float4 tail); [2048,479] once (sixty partial workgroups). Layer
shapes: cpu_linear.SHAPES, and BIG_SHAPE once for the 64 x 64 tile."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import cpu_act as A
import cpu_linear as R
import cpu_mlp as M

pytestmark = pytest.mark.gpu

ACTS = {A.NONE: None, A.RELU: "relu", A.SIGMOID: "sigmoid"}
CASES = [(s, bits, pc) for s in R.SHAPES for bits in (4, 8) for pc in (True, False)]
IDS = ["B{}-in{}-out{}-b{}-{}".format(*s, bits, "chan" if pc else "tensor") for s, bits, pc in CASES]
EXACT_CASES = CASES + [(R.BIG_SHAPE, 4, True)]
EXACT_IDS = IDS + ["big-b4-chan"]


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


def _check_bound(got, want64, bound, what):
    err = (got.double() - want64).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


# ================================================================== 1. QuantAct
ACT_SHAPES = [((1, 1), 8), ((7, 13), 8), ((7, 13), 16), ((130, 479), 8), ((130, 479), 16)]
SEQ_CASES = [(s, b, m, seed) for s, b in ACT_SHAPES for m in (-1, 0.95) for seed in (0, 1)]
SEQ_CASES += [((2048, 479), 8, 0.95, 1), ((2048, 479), 16, -1, 0)]  # the large shape, once per momentum
SEQ_IDS = ["{}x{}-b{}-{}-{}".format(*s, b, "minmax" if m == -1 else "ema", "zeros-first" if seed == 0 else "const-first")
           for s, b, m, seed in SEQ_CASES]


@pytest.mark.parametrize("shape,bits,momentum,seed", SEQ_CASES, ids=SEQ_IDS)
def test_quantact_sequence_bit_exact(dq, shape, bits, momentum, seed):
    """Three batches through one module (the first all equal, so the x_min == x_max branch is
    taken twice, with the 1e-8 clamp when it is all zero), then fix() and a fourth that leaves the
    range alone: y, x_min, x_max and act_scaling_factor after each."""
    ref = A.ActRef(bits, momentum)
    mod = dq.QuantAct(activation_bit=bits, act_range_momentum=momentum).cuda()
    batches = A.act_batches(shape, seed)
    for i, x in enumerate(batches):
        if i == 3:
            ref.fix()
            mod.fix()
        y_r, s_r = ref.forward(x)
        y, s = mod(x.cuda())
        assert s is mod.act_scaling_factor and s.shape == (1,) and mod.x_min.shape == (1,)
        _eq(mod.x_min, ref.x_min, f"x_min after batch {i}")
        _eq(mod.x_max, ref.x_max, f"x_max after batch {i}")
        _eq(s, s_r, f"act_scaling_factor after batch {i}")
        _eq(y, y_r, f"y of batch {i}")
    if seed == 0:
        assert float(batches[0].abs().max()) == 0.0  # the clamp was the first scale
    n = R.qmax(bits)
    if bits == 8 and shape[0] > 1:  # the fixed range is narrower than the fourth batch: both clamps are hit
        q = (y_r / s_r).round()
        assert float(q.max()) == n and float(q.min()) == -n - 1


def test_quantact_full_precision_follows_the_range_only(dq):
    x = A.act_batches((130, 479), 1)[1]
    ref = A.ActRef(8, -1)
    ref.update_range(x)
    mod = dq.QuantAct(activation_bit=8, act_range_momentum=-1, full_precision_flag=True).cuda()
    xg = x.cuda()
    assert mod(xg) is xg
    _eq(mod.x_min, ref.x_min, "x_min")
    _eq(mod.x_max, ref.x_max, "x_max")
    assert float(mod.act_scaling_factor) == 0.0


@pytest.mark.parametrize("shape", [(7, 13), (130, 479)], ids=["7x13", "130x479"])
def test_quantact_backward_and_no_grad_input(dq, shape):
    x = A.act_batches(shape, 1)[1]
    dy = torch.from_numpy(np.random.RandomState(5).standard_normal(shape).astype(np.float32))
    ref = A.ActRef(8, -1)
    xr = x.clone().requires_grad_(True)
    y_r, s_r = ref.forward(xr)
    y_r.backward(dy)
    mod = dq.QuantAct(activation_bit=8, act_range_momentum=-1).cuda()
    xg = x.cuda().requires_grad_(True)
    y, s = mod(xg)
    assert not s.requires_grad
    y.backward(dy.cuda())
    _eq(y, y_r, "y")
    _eq(xg.grad, xr.grad, "x.grad")
    # quant_input's case: the dense features need no gradient, so no backward node exists at all
    y2, _ = mod(x.cuda())
    assert not y2.requires_grad and y2.grad_fn is None
    # the tuple input and fixed_point_quantization with a previous scale take the same branch
    mod2 = dq.QuantAct(activation_bit=8, act_range_momentum=-1, fixed_point_quantization=True).cuda()
    y3, s3 = mod2((x.cuda(), s))
    _eq(y3, y_r, "y through the tuple input")
    _eq(s3, s_r, "scale through the tuple input")


def test_quantact_c_calls_numel_zero_and_unaligned(dq):
    """numel == 0 leaves the range alone; a 4-byte-aligned x / y takes the scalar kernel and gives
    the same bits as the float4 one."""
    L = dq._lib
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    x = A.act_batches((130, 479), 1)[1].cuda().reshape(-1)
    rng = torch.tensor([-0.5, 0.75, 0.0], device="cuda")
    q = L.ActQuant()
    q.activation_bit, q.running_stat, q.momentum, q.one_minus_momentum = 8, 1, -1.0, 2.0
    q.x_min, q.x_max, q.scale = rng[0:1].data_ptr(), rng[1:2].data_ptr(), rng[2:3].data_ptr()
    ws = torch.empty(lib.dqrm_act_quant_workspace_bytes(x.numel()), dtype=torch.uint8, device="cuda")
    assert lib.dqrm_act_quant_fwd(C.byref(q), x.data_ptr(), 0, x.data_ptr(), ws.data_ptr(), st) == L.DQRM_OK
    assert rng.tolist() == [-0.5, 0.75, 0.0]
    y = torch.empty_like(x)
    L.check(lib.dqrm_act_quant_fwd(C.byref(q), x.data_ptr(), x.numel(), y.data_ptr(), ws.data_ptr(), st), "fwd")
    q.running_stat = 0
    buf_x, buf_y = torch.empty(x.numel() + 1, device="cuda"), torch.empty(x.numel() + 1, device="cuda")
    buf_x[1:].copy_(x)
    L.check(lib.dqrm_act_quant_fwd(C.byref(q), buf_x[1:].data_ptr(), x.numel(), buf_y[1:].data_ptr(), None, st), "fwd")
    _eq(buf_y[1:], y, "scalar kernel against the float4 kernel")
    ref = A.ActRef(8, -1)
    ref.x_min, ref.x_max = torch.tensor([-0.5]), torch.tensor([0.75])
    y_r, s_r = ref.forward(x.cpu())
    _eq(y, y_r, "y")
    _eq(rng[2:3], s_r, "scale")


# ================================================================== 2 / 3. the layer
def _layer(dq, W, b, bits, per_channel, activation=None):
    lin = nn.Linear(W.shape[1], W.shape[0])
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    q = dq.QuantLinear(weight_bit=bits, bias_bit=bits, per_channel=per_channel, quantize_activation=True)
    q.set_param(lin.cuda())
    q.activation = activation
    return q


def _module_step(layer, x, dy, prev, x_grad=True):
    xg = x.cuda().requires_grad_(x_grad)
    layer.weight.grad = layer.bias.grad = None
    y, cos = layer(xg, prev.cuda())
    assert cos is layer.correct_output_scale and not cos.requires_grad
    y.backward(dy.cuda())
    return y.detach(), cos, (xg.grad if x_grad else None, layer.weight.grad, layer.bias.grad)


class CLayer:
    """The bare C calls on caller-owned buffers."""

    def __init__(self, dq, W, b, bits, per_channel, prev):
        self.L = dq._lib
        self.lib = self.L.load()
        O_, K = W.shape
        self.W, self.b = W.cuda().contiguous(), b.cuda().contiguous()
        self.wi, self.bi = torch.empty_like(self.W), torch.empty_like(self.b)
        self.s = torch.empty(O_ if per_channel else 1, device="cuda")
        self.cos = torch.empty(O_ if per_channel else 1, device="cuda")
        self.prev = prev.cuda()
        c = self.L.Linear()
        c.in_features, c.out_features, c.weight_bit, c.bias_bit, c.per_channel = K, O_, bits, bits, int(per_channel)
        c.weight, c.bias = self.W.data_ptr(), self.b.data_ptr()
        c.weight_integer, c.bias_integer, c.scale = self.wi.data_ptr(), self.bi.data_ptr(), self.s.data_ptr()
        self.c, self.K, self.O = c, K, O_
        self.st = torch.cuda.current_stream().cuda_stream

    def wquant(self):
        self.L.check(self.lib.dqrm_linear_wquant_qact(C.byref(self.c), self.prev.data_ptr(), self.cos.data_ptr(),
                                                      self.st), "wquant_qact")

    def fwd(self, x, act=A.NONE):
        x = x.cuda().contiguous()
        y = torch.empty(x.shape[0], self.O, device="cuda")
        self.L.check(self.lib.dqrm_linear_fwd_qact(C.byref(self.c), act, x.data_ptr(), self.prev.data_ptr(),
                                                   self.cos.data_ptr(), x.shape[0], y.data_ptr(), self.st), "fwd_qact")
        return y

    def bwd(self, x, dy, act=A.NONE, y=None, want_dx=True):
        x, dy = x.cuda().contiguous(), dy.cuda().contiguous()
        y = None if y is None else y.cuda().contiguous()
        dx = torch.empty_like(x) if want_dx else None
        dw, db = torch.empty_like(self.W), torch.empty_like(self.b)
        self.L.check(self.lib.dqrm_linear_bwd_qact(C.byref(self.c), act, x.data_ptr(),
                                                   None if y is None else y.data_ptr(), dy.data_ptr(),
                                                   self.prev.data_ptr(), self.cos.data_ptr(), x.shape[0],
                                                   dx.data_ptr() if want_dx else None, dw.data_ptr(), db.data_ptr(),
                                                   self.st), "bwd_qact")
        return dx, dw, db


@pytest.fixture(scope="module")
def exact_refs():
    """The restatement's results per exact case, computed once and shared by the activations."""
    cache = {}

    def get(shape, bits, pc, act):
        key = (shape, bits, pc, act)
        if key not in cache:
            B, K, O_ = shape
            W, b, x, dy, prev = A.exact_case(B, K, O_, bits, pc, seed=7 + B)
            cache[key] = (W, b, x, dy, prev) + A.layer_forward_backward(x, W, b, dy, prev, bits, pc, act)
        return cache[key]

    return get


@pytest.mark.parametrize("act", [A.NONE, A.RELU, A.SIGMOID], ids=["none", "relu", "sigmoid"])
@pytest.mark.parametrize("shape,bits,per_channel", EXACT_CASES, ids=EXACT_IDS)
def test_layer_exact_data_bit_exact(dq, exact_refs, shape, bits, per_channel, act):
    """y, out_scale, bias_integer, dx, dw, db on data whose every product and partial sum is exact
    in any order (cpu_act.exact_case; tests/test_act_host.py asserts that the pre-round values
    contain exact .5 ties). Sigmoid: the forward within the sigmoid bound of the exact z, the
    backward bit for bit on a y from {0, 1/4, 1/2, 3/4, 1} through the C call."""
    B, K, O_ = shape
    W, b, x, dy, prev, y_r, cos_r, (s_r, wi_r, bi_r, pre_r, z_r), (dx_r, dw_r, db_r) = \
        exact_refs(shape, bits, per_channel, act if act != A.SIGMOID else A.NONE)
    c = CLayer(dq, W, b, bits, per_channel, prev)
    c.wquant()
    _eq(c.s, s_r, "scale")
    _eq(c.wi, wi_r, "weight_integer")
    _eq(c.cos, cos_r.view(-1), "out_scale")
    _eq(c.bi, bi_r, "bias_integer")
    layer = _layer(dq, W, b, bits, per_channel, ACTS[act])
    if act == A.SIGMOID:
        sig = torch.sigmoid(z_r.double())
        _check_bound(c.fwd(x, act).cpu(), sig, M.sigmoid_bound(sig), "C sigmoid(z)")
        y_m, cos, _ = _module_step(layer, x, dy, prev)
        _check_bound(y_m.cpu(), sig, M.sigmoid_bound(sig), "module sigmoid(z)")
        _eq(cos, cos_r, "module correct_output_scale")
        y = torch.from_numpy((np.random.RandomState(B + 1000).randint(0, 5, (B, O_)) / 4.0).astype(np.float32))
        want = A.backward_from_d(M.sigmoid_d(dy, y), x, wi_r, s_r, prev)
        want64 = A.backward_from_d(M.sigmoid_d(dy.double(), y.double()), x, wi_r, s_r, prev)
        for w, w64 in zip(want, want64):
            assert torch.equal(w.double(), w64)  # the construction: exact in any order
        for got, w, what in zip(c.bwd(x, dy, act, y), want, ("dx", "dw", "db")):
            _eq(got, w, "C sigmoid backward " + what)
        return
    _eq(c.fwd(x, act), y_r, "C y")
    y_m, cos, (dx, dw, db) = _module_step(layer, x, dy, prev)
    assert cos.shape == (1, O_ if per_channel else 1)
    _eq(cos, cos_r, "module correct_output_scale")
    _eq(layer.bias_integer, bi_r, "module bias_integer")
    _eq(y_m, y_r, "module y")
    _eq(dx, dx_r, "module x.grad")
    _eq(dw, dw_r, "module weight.grad")
    _eq(db, db_r, "module bias.grad")
    dx, dw, db = c.bwd(x, dy, act, y_r)
    _eq(dx, dx_r, "C dx")
    _eq(dw, dw_r, "C dw")
    _eq(db, db_r, "C db")
    dx, dw, db = c.bwd(x, dy, act, y_r, want_dx=False)
    assert dx is None
    _eq(dw, dw_r, "C dw (dx NULL)")
    _eq(db, db_r, "C db (dx NULL)")
    _, _, (dx, dw, db) = _module_step(layer, x, dy, prev, x_grad=False)
    assert dx is None
    _eq(dw, dw_r, "module weight.grad (input needs no gradient)")
    _eq(db, db_r, "module bias.grad (input needs no gradient)")


def _plain(dq, weight, bias):
    """A full-precision dqrm_linear over the given operands (the already-tested chain)."""
    L = dq._lib
    c = L.Linear()
    c.out_features, c.in_features = weight.shape
    c.weight, c.bias = weight.data_ptr(), bias.data_ptr()
    return c


@pytest.mark.parametrize("act", [A.NONE, A.RELU, A.SIGMOID], ids=["none", "relu", "sigmoid"])
@pytest.mark.parametrize("shape,bits,per_channel", EXACT_CASES, ids=EXACT_IDS)
def test_layer_random_data_equals_composition_of_tested_calls(dq, shape, bits, per_channel, act):
    """One ulp before the rounding can move a whole quantum, so the expectation is built from the
    existing contract instead of a differently ordered CPU product: dqrm_linear_fwd(quantized=0)
    over (x / p, weight_integer, bias_integer) gives the pre-round value, torch rounds, scales and
    activates; dqrm_linear_bwd(quantized=0) over (x / p, g = d * cos) gives the three chains, torch
    divides. Bit for bit (a Sigmoid's y within its bound; its backward from the y the kernel wrote)."""
    B, K, O_ = shape
    L, lib, st = dq._lib, dq._lib.load(), torch.cuda.current_stream().cuda_stream
    W, b, x, dy, prev = A.random_case(B, K, O_, seed=100 + K)
    s_r = R.weight_scale(W, bits, per_channel)
    c = CLayer(dq, W, b, bits, per_channel, prev)
    c.wquant()
    _eq(c.s, s_r, "scale")
    _eq(c.wi, R.SymQuant.apply(W, bits, s_r), "weight_integer")
    cos_r = s_r * prev
    _eq(c.cos, cos_r, "out_scale")
    _eq(c.bi, R.SymQuant.apply(b, bits, cos_r), "bias_integer")
    xg, dyg, p = x.cuda(), dy.cuda(), prev.cuda()
    x_int = xg / p
    plain = _plain(dq, c.wi, c.bi)
    pre = torch.empty(B, O_, device="cuda")
    L.check(lib.dqrm_linear_fwd(C.byref(plain), 0, x_int.data_ptr(), B, pre.data_ptr(), st), "fwd")
    if O_ > 1:  # (the single row of out = 1 is random_case's all-zero row)
        assert float((pre - pre.round()).abs().max()) > 0.01  # the rounding has work to do
    z = torch.round(pre) * c.cos.view(1, -1)
    y = c.fwd(x, act)
    if act == A.SIGMOID:
        sig = torch.sigmoid(z.double())
        _check_bound(y.double(), sig, M.sigmoid_bound(sig), "sigmoid(z)")
        d = M.sigmoid_d(dyg, y)
    else:
        _eq(y, torch.relu(z) if act == A.RELU else z, "y")
        d = M.relu_d(dyg, y) if act == A.RELU else dyg
    g = (d * c.cos.view(1, -1)).contiguous()
    dxc, dwc, dbc = torch.empty_like(x_int), torch.empty_like(c.W), torch.empty_like(c.b)
    L.check(lib.dqrm_linear_bwd(C.byref(plain), 0, x_int.data_ptr(), g.data_ptr(), B, dxc.data_ptr(), dwc.data_ptr(),
                                dbc.data_ptr(), st), "bwd")
    dx, dw, db = c.bwd(x, dy, act, y)
    _eq(dx, dxc / p, "dx")
    _eq(dw, dwc / c.s.view(-1, 1), "dw")
    _eq(db, dbc / c.cos, "db")
    _, dw, db = c.bwd(x, dy, act, y, want_dx=False)
    _eq(dw, dwc / c.s.view(-1, 1), "dw (dx NULL)")
    _eq(db, dbc / c.cos, "db (dx NULL)")


# ================================================================== 4. module and stack
def _stacks(dq, ln, sigmoid_layer, seed, bits=4):
    np.random.seed(seed)
    fused = dq.create_mlp(ln, sigmoid_layer, weight_bit=bits, quantize_activation=True)
    np.random.seed(seed)
    plain = dq.create_mlp(ln, sigmoid_layer, weight_bit=bits, quantize_activation=True, fused=False)
    assert [type(l).__name__ for l in fused][1::2] == ["FusedActivation"] * (len(ln) - 1)
    assert all(isinstance(l, (nn.ReLU, nn.Sigmoid)) for l in list(plain)[1::2])
    return fused.cuda(), plain.cuda()


def _qact_stack_step(dq, qact, layers, x, dy):
    xg = x.cuda().requires_grad_(True)
    for p in layers.parameters():
        p.grad = None
    h, s = qact(xg)
    y = dq.apply_mlp(h, layers, prev_act_scaling_factor=s)
    y.backward(dy.cuda())
    grads = [(l.weight.grad.clone(), l.bias.grad.clone()) for l in layers if isinstance(l, dq.QuantLinear)]
    return y.detach(), xg.grad, grads


def test_stack_fused_equals_unfused_bit_for_bit(dq):
    """QuantAct -> a ReLU stack with quantize_activation: the fused layers against torch's ReLU
    between the same layers, outputs and every gradient."""
    fused, plain = _stacks(dq, [13, 64, 16], -1, seed=31)
    rs = np.random.RandomState(32)
    x = torch.from_numpy(rs.standard_normal((130, 13)).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal((130, 16)).astype(np.float32))
    qa, qb = (dq.QuantAct(activation_bit=8, act_range_momentum=-1).cuda() for _ in range(2))
    yf, dxf, gf = _qact_stack_step(dq, qa, fused, x, dy)
    yp, dxp, gp = _qact_stack_step(dq, qb, plain, x, dy)
    assert 0.05 < float((yp > 0).float().mean()) < 0.95 and float(dxp.abs().max()) > 0
    _eq(yf, yp, "output")
    _eq(dxf, dxp, "x.grad")
    for k, ((wf, bf), (wp, bp)) in enumerate(zip(gf, gp)):
        assert float(wp.abs().max()) > 0
        _eq(wf, wp, f"layer {k} weight.grad")
        _eq(bf, bp, f"layer {k} bias.grad")
    # a per-channel scale cannot feed the next layer (neither can it in the reference)
    np.random.seed(1)
    chan = dq.create_mlp([13, 8, 4], -1, per_channel=True, quantize_activation=True).cuda()
    h, s = qa(x.cuda())
    with pytest.raises(ValueError, match="ONE element"):
        dq.apply_mlp(h, chan, prev_act_scaling_factor=s)


def _set_params(layers, params):
    with torch.no_grad():
        for l, (W, b) in zip([l for l in layers if hasattr(l, "weight")], params):
            l.weight.copy_(W)
            l.bias.copy_(b)


@pytest.mark.parametrize("ln,sigmoid_layer,fixed_point", [([13, 64, 16], -1, False), ([27, 32, 1], 1, True)],
                         ids=["bottom", "top"])
def test_exact_stack_against_restatement_over_two_sgd_steps(dq, ln, sigmoid_layer, fixed_point):
    """The drivers' sequence (quant_input -> bot_l, quant_feature_outputs -> top_l) on exact data
    against the restatement, two SGD steps with lr = 2^-6.

    Step 1: every scale is a power of two and every sum exact in any order. The ReLU (bottom)
    stack's y, x.grad and every parameter gradient are compared bit for bit, and so are the
    weights after the optimizer's step. The top stack ends in a Sigmoid: the value before it is
    exact, its y is held to the sigmoid bound, and, since torch's sigmoid and the kernel's differ in
    their last bits, the restatement's gradients are carried over so that step 2 starts from the
    same weights on both sides.
    Step 2: the scales are no powers of two any more; the scales and the quantized integers of
    every layer are compared bit for bit. A layer's forward is still order-independent while its
    x / prev are integers, which holds for the first layer always and for a later one only while
    (q * cos) / cos gives q back exactly (checked on the restatement): the layers' outputs are
    compared bit for bit up to the first layer for which it does not. The step-2 gradients are sums
    of rounded g = d * cos and depend on the summation order of the CPU product; the fused /
    unfused and the composition tests cover them."""
    B, bits, lr = 33, 4, 2.0 ** -6
    params = A.exact_stack(ln, bits, seed=41 + ln[0])
    x = A.exact_act_input(B, ln[0], seed=43)
    dy = torch.from_numpy((np.random.RandomState(44).randint(-8, 9, (B, ln[-1])) / 8.0).astype(np.float32))
    np.random.seed(0)
    layers = dq.create_mlp(ln, sigmoid_layer, weight_bit=bits, quantize_activation=True).cuda()
    _set_params(layers, params)
    qact = dq.QuantAct(activation_bit=8, act_range_momentum=-1, fixed_point_quantization=fixed_point).cuda()
    ref_act = A.ActRef(8, -1)
    ref_params = [(W.clone().requires_grad_(True), b.clone().requires_grad_(True)) for W, b in params]
    opt = torch.optim.SGD(layers.parameters(), lr=lr)
    opt_r = torch.optim.SGD([t for pair in ref_params for t in pair], lr=lr)
    qlayers = [l for l in layers if isinstance(l, dq.QuantLinear)]
    for step in (1, 2):
        opt.zero_grad(set_to_none=True)
        opt_r.zero_grad(set_to_none=True)
        xr = x.clone().requires_grad_(True)
        h_r, s_r = ref_act.forward(xr)
        y_r, seen, zs = A.stack_forward(h_r, ref_params, s_r, bits, sigmoid_layer)
        y_r.backward(dy)
        xg = x.cuda().requires_grad_(True)
        outs = []
        hooks = [l.register_forward_hook(lambda m, a, out: outs.append(out[0].detach())) for l in qlayers]
        # quant_feature_outputs' form: a previous scale with fixed_point_quantization changes nothing
        h, s = qact((xg, torch.ones(1, device="cuda"))) if fixed_point else qact(xg)
        y = dq.apply_mlp(h, layers, prev_act_scaling_factor=s)
        for hk in hooks:
            hk.remove()
        y.backward(dy.cuda())
        _eq(h, h_r, f"step {step}: QuantAct y")
        _eq(s, s_r, f"step {step}: act_scaling_factor")
        assert float(s) == 2.0 ** -3
        for k, (l, (W_r, b_r)) in enumerate(zip(qlayers, ref_params)):
            sc = R.weight_scale(W_r.detach(), bits, False)
            _eq(l.fc_scaling_factor, sc, f"step {step}: layer {k} fc_scaling_factor")
            _eq(l.weight_integer, R.SymQuant.apply(W_r.detach(), bits, sc), f"step {step}: layer {k} weight_integer")
        compared = 0
        for k, xi in enumerate(seen):
            # a layer's sums are exact in any order while its x / prev are integers small enough
            if not (torch.equal(xi, xi.round()) and float(xi.abs().max()) * R.qmax(bits) * ln[k] < 2 ** 24):
                break
            if k == sigmoid_layer:
                sig = torch.sigmoid(zs[k].double())
                _check_bound(outs[k].cpu(), sig, M.sigmoid_bound(sig), f"step {step}: layer {k} sigmoid(z)")
            else:
                _eq(outs[k], torch.relu(zs[k]), f"step {step}: layer {k} output")
            compared += 1
        assert compared == len(qlayers) if step == 1 else compared >= 1
        if compared == len(qlayers) and sigmoid_layer < 0:
            _eq(y, y_r, f"step {step}: y")
        if step == 2:
            break
        if sigmoid_layer < 0:
            _eq(xg.grad, xr.grad, "step 1: x.grad")
            for k, (l, (W_r, b_r)) in enumerate(zip(qlayers, ref_params)):
                assert float(W_r.grad.abs().max()) > 0
                _eq(l.weight.grad, W_r.grad, f"step 1: layer {k} weight.grad")
                _eq(l.bias.grad, b_r.grad, f"step 1: layer {k} bias.grad")
        else:
            for l, (W_r, b_r) in zip(qlayers, ref_params):
                assert float(l.weight.grad.abs().max()) > 0
                l.weight.grad.copy_(W_r.grad)
                l.bias.grad.copy_(b_r.grad)
        opt.step()
        opt_r.step()
        for k, (l, (W_r, b_r)) in enumerate(zip(qlayers, ref_params)):
            assert not torch.equal(W_r.detach(), params[k][0])
            _eq(l.weight, W_r, f"after step 1: layer {k} weight")
            _eq(l.bias, b_r, f"after step 1: layer {k} bias")


def test_deterministic_and_batch_invariant(dq):
    B, K, O_ = 130, 70, 66
    W, b, x, dy, prev = A.random_case(B, K, O_, seed=5)
    layer = _layer(dq, W, b, 4, True, "relu")
    first = _module_step(layer, x, dy, prev)
    second = _module_step(layer, x, dy, prev)
    _eq(first[0], second[0], "y run to run")
    for a, c, what in zip(first[2], second[2], ("dx", "dw", "db")):
        _eq(a, c, what + " run to run")
    y7, _, (dx7, _, _) = _module_step(layer, x[:7].contiguous(), dy[:7].contiguous(), prev)
    _eq(y7, first[0][:7], "y of rows 0..6 alone against rows 0..6 of the batch")
    _eq(dx7, first[2][0][:7], "x.grad of rows 0..6 alone against rows 0..6 of the batch")
    # a fixed QuantAct is a function of the element alone
    qa = dq.QuantAct(activation_bit=8, act_range_momentum=-1).cuda()
    ya, _ = qa(x.cuda())
    qa.fix()
    yb, _ = qa(x[:7].contiguous().cuda())
    _eq(yb, ya[:7], "QuantAct rows 0..6 alone")


def test_weight_only_path_is_untouched_by_the_flagged_kernels(dq):
    """The weight-only layer next to an activation-quantized one over the same weights: scale and
    weight_integer agree bit for bit (dqrm_linear_wquant_qact does what dqrm_linear_wquant does
    for them) and the weight-only layer still returns (y, None)."""
    W, b, x, dy, prev = A.random_case(33, 70, 66, seed=9)
    for pc in (True, False):
        qa = _layer(dq, W, b, 4, pc)
        wo = _layer(dq, W, b, 4, pc)
        wo.quantize_activation = False
        y, none = wo(x.cuda())
        assert none is None
        qa(x.cuda(), prev.cuda())
        _eq(qa.fc_scaling_factor, wo.fc_scaling_factor, "fc_scaling_factor")
        _eq(qa.weight_integer, wo.weight_integer, "weight_integer")


# ================================================================== 5. C validation on the device
def test_c_validation_and_no_ops_on_the_device(dq):
    L, lib, st = dq._lib, dq._lib.load(), torch.cuda.current_stream().cuda_stream
    W, b, x, dy, prev = A.exact_case(7, 13, 5, 8, True, seed=3)
    c = CLayer(dq, W, b, 8, True, prev)
    c.wquant()
    y = torch.full((7, 5), 3.0, device="cuda")
    xg = x.cuda()
    # B == 0: nothing written
    assert lib.dqrm_linear_fwd_qact(C.byref(c.c), 0, xg.data_ptr(), c.prev.data_ptr(), c.cos.data_ptr(), 0,
                                    y.data_ptr(), st) == L.DQRM_OK
    assert lib.dqrm_linear_fwd_qact(C.byref(c.c), 0, xg.data_ptr(), None, c.cos.data_ptr(), 7, y.data_ptr(),
                                    st) == L.DQRM_E_INVALID
    assert lib.dqrm_linear_fwd_qact(C.byref(c.c), 7, xg.data_ptr(), c.prev.data_ptr(), c.cos.data_ptr(), 7,
                                    y.data_ptr(), st) == L.DQRM_E_INVALID
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    # the module on an empty batch
    layer = _layer(dq, W, b, 8, True)
    y0, cos0 = layer(torch.empty(0, 13, device="cuda"), prev.cuda())
    assert y0.shape == (0, 5) and cos0.shape == (1, 5)
    _eq(cos0.view(-1), c.cos, "correct_output_scale of an empty batch")
