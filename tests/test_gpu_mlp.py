"""GPU: the MLP's ReLU / Sigmoid fused into QuantLinear's kernels (dqrm_linear_fwd_act / _bwd_act,
QuantLinear.activation, mlp.py) against tests/cpu_mlp.py and against the unfused package layer
followed by the torch activation.

Shapes (B, in, out) are tests/cpu_linear.py's: (7, 13, 5), (64, 415, 1) (the sigmoid's real place:
a one-column output), (33, 512, 256), (130, 70, 66), and (1040, 1030, 1050), the only one on the
64 x 64 workgroup tile."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from torch import nn

import cpu_linear as R
import cpu_mlp as M
import gen_inputs as G
import oracle as O

pytestmark = pytest.mark.gpu

CASES = [(s, bits, pc) for s in R.SHAPES for bits in (4, 8) for pc in (True, False)]
IDS = ["B{}-in{}-out{}-b{}-{}".format(*s, bits, "chan" if pc else "tensor") for s, bits, pc in CASES]
EXACT_CASES = CASES + [(R.BIG_SHAPE, 4, True)]
EXACT_IDS = IDS + ["big-b4-chan"]
SHAPE_IDS = ["B{}-in{}-out{}".format(*s) for s in R.SHAPES]
QUANT = pytest.mark.parametrize("full_precision", [False, True], ids=["quant", "fp32"])


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _layer(dq, W, b, bits, per_channel, full_precision=False, activation=None):
    lin = nn.Linear(W.shape[1], W.shape[0])
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    q = dq.QuantLinear(weight_bit=bits, bias_bit=bits, full_precision_flag=full_precision, per_channel=per_channel)
    q.set_param(lin.cuda())
    q.activation = activation
    return q


def _module_step(layer, x, dy, x_grad=True, after=None):
    """y, x.grad, weight.grad, bias.grad of one forward + backward through the module (and
    `after`, a torch activation applied to its output)."""
    xg = x.cuda().requires_grad_(x_grad)
    layer.weight.grad = layer.bias.grad = None
    y, prev = layer(xg)
    assert prev is None
    if after is not None:
        y = after(y)
    y.backward(dy.cuda())
    return (y.detach().cpu(), xg.grad.cpu() if x_grad else None, layer.weight.grad.cpu(), layer.bias.grad.cpu())


class CLayer:
    """The bare C calls on caller-owned buffers."""

    def __init__(self, dq, W, b, bits, per_channel):
        self.L = dq._lib
        self.lib = self.L.load()
        O_, K = W.shape
        self.W, self.b = W.cuda().contiguous(), b.cuda().contiguous()
        self.wi, self.bi = torch.empty_like(self.W), torch.empty_like(self.b)
        self.s = torch.empty(O_ if per_channel else 1, device="cuda")
        c = self.L.Linear()
        c.in_features, c.out_features, c.weight_bit, c.bias_bit, c.per_channel = K, O_, bits, bits, int(per_channel)
        c.weight, c.bias = self.W.data_ptr(), self.b.data_ptr()
        c.weight_integer, c.bias_integer, c.scale = self.wi.data_ptr(), self.bi.data_ptr(), self.s.data_ptr()
        self.c, self.K, self.O = c, K, O_
        self.st = torch.cuda.current_stream().cuda_stream

    def wquant(self):
        self.L.check(self.lib.dqrm_linear_wquant(C.byref(self.c), self.st), "wquant")

    def fwd(self, x, quantized=1, act=None):
        x = x.cuda().contiguous()
        y = torch.full((x.shape[0], self.O), float("nan"), device="cuda")
        if act is None:
            rc = self.lib.dqrm_linear_fwd(C.byref(self.c), quantized, x.data_ptr(), x.shape[0], y.data_ptr(), self.st)
        else:
            rc = self.lib.dqrm_linear_fwd_act(C.byref(self.c), quantized, act, x.data_ptr(), x.shape[0], y.data_ptr(),
                                              self.st)
        self.L.check(rc, "fwd")
        return y.cpu()

    def bwd(self, x, dy, quantized=1, want_dx=True, act=None, y=None):
        x, dy = x.cuda().contiguous(), dy.cuda().contiguous()
        y = None if y is None else y.cuda().contiguous()
        dx = torch.full_like(x, float("nan")) if want_dx else None
        dw, db = torch.full_like(self.W, float("nan")), torch.full_like(self.b, float("nan"))
        if act is None:
            rc = self.lib.dqrm_linear_bwd(C.byref(self.c), quantized, x.data_ptr(), dy.data_ptr(), x.shape[0],
                                          dx.data_ptr() if want_dx else None, dw.data_ptr(), db.data_ptr(), self.st)
        else:
            rc = self.lib.dqrm_linear_bwd_act(C.byref(self.c), quantized, act, x.data_ptr(),
                                              None if y is None else y.data_ptr(), dy.data_ptr(), x.shape[0],
                                              dx.data_ptr() if want_dx else None, dw.data_ptr(), db.data_ptr(),
                                              self.st)
        self.L.check(rc, "bwd")
        return (dx.cpu() if want_dx else None), dw.cpu(), db.cpu()


def _eq(got, want, what):
    np.testing.assert_array_equal(got.numpy(), want.numpy(), err_msg=what)


def _check_bound(got, want64, bound, what):
    err = (got.double() - want64).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


# ------------------------------------------------------------------ 1. act = NONE is today's kernel
@QUANT
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_act_none_equals_the_plain_exports(dq, shape, full_precision):
    B, K, O_ = shape
    W, b, x, dy = R.random_case(B, K, O_, seed=100 + K)
    c = CLayer(dq, W, b, 4, True)
    c.wquant()
    q = int(not full_precision)
    _eq(c.fwd(x, q, act=M.NONE), c.fwd(x, q), "y")
    want = c.bwd(x, dy, q)
    for y in (None, torch.full((B, O_), float("nan"))):  # y is ignored with NONE, and may be NULL
        for a, w, what in zip(c.bwd(x, dy, q, act=M.NONE, y=y), want, ("dx", "dw", "db")):
            _eq(a, w, what)
    _, dw, db = c.bwd(x, dy, q, want_dx=False, act=M.NONE)
    _eq(dw, want[1], "dw (dx NULL)")
    _eq(db, want[2], "db (dx NULL)")


# ------------------------------------------------------------------ 2. ReLU, exact data
@functools.lru_cache(maxsize=None)
def _relu_reference(shape, bits, per_channel, full_precision=False):
    """The inputs and the CPU restatement's z, y and gradients, computed once per case."""
    B, K, O_ = shape
    W, b, x, dy = R.exact_case(B, K, O_, bits, per_channel, seed=7 + B)
    return (W, b, x, dy) + M.forward_backward(x, W, b, dy, bits, per_channel, M.RELU, full_precision)


def _relu_exact(dq, shape, bits, per_channel, full_precision=False):
    W, b, x, dy, z, y_r, dx_r, dw_r, db_r = _relu_reference(shape, bits, per_channel, full_precision)
    pos, neg = float((z > 0).float().mean()), float((z < 0).float().mean())
    print(f"z > 0: {pos:.3f}, z < 0: {neg:.3f}, z == 0: {int((z == 0).sum())}")
    assert pos >= 0.25 and neg >= 0.25
    q = int(not full_precision)
    layer = _layer(dq, W, b, bits, per_channel, full_precision, "relu")
    y, dx, dw, db = _module_step(layer, x, dy)
    _eq(y, y_r, "module y")
    _eq(dx, dx_r, "module x.grad")
    _eq(dw, dw_r, "module weight.grad")
    _eq(db, db_r, "module bias.grad")
    c = CLayer(dq, W, b, bits, per_channel)
    c.wquant()
    y = c.fwd(x, q, act=M.RELU)
    _eq(y, y_r, "C y")
    assert not bool(torch.signbit(y[y == 0]).any())  # -0 becomes +0
    dx, dw, db = c.bwd(x, dy, q, act=M.RELU, y=y)
    _eq(dx, dx_r, "C dx")
    _eq(dw, dw_r, "C dw")
    _eq(db, db_r, "C db")
    _, dw, db = c.bwd(x, dy, q, want_dx=False, act=M.RELU, y=y)
    _eq(dw, dw_r, "C dw (dx NULL)")
    _eq(db, db_r, "C db (dx NULL)")
    y, dx, dw, db = _module_step(layer, x, dy, x_grad=False)
    assert dx is None
    _eq(dw, dw_r, "module weight.grad (input needs no gradient)")
    _eq(db, db_r, "module bias.grad (input needs no gradient)")


@pytest.mark.parametrize("shape,bits,per_channel", EXACT_CASES, ids=EXACT_IDS)
def test_relu_exact_data_bit_exact(dq, shape, bits, per_channel):
    _relu_exact(dq, shape, bits, per_channel)


def test_relu_exact_data_full_precision(dq):
    _relu_exact(dq, (130, 70, 66), 4, True, full_precision=True)


def test_relu_exact_cases_contain_z_equal_zero():
    """The boundary of `z <= 0` (y = 0 and no gradient) occurs in the cases above."""
    assert any(bool((_relu_reference(*case)[4] == 0).any()) for case in EXACT_CASES)


def test_relu_keeps_nan(dq):
    W, b, x, dy = R.exact_case(7, 13, 5, 4, True, seed=3)
    x[2, 4] = float("nan")
    c = CLayer(dq, W, b, 4, True)
    c.wquant()
    y = c.fwd(x, 1, act=M.RELU)
    assert bool(torch.isnan(y[2]).all()) and not bool(torch.isnan(y[[0, 1, 3, 4, 5, 6]]).any())


# ------------------------------------------------------------------ 3. ReLU fused == unfused, random data
@QUANT
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_relu_fused_equals_layer_then_torch_relu(dq, shape, full_precision):
    B, K, O_ = shape
    W, b, x, dy = R.random_case(B, K, O_, seed=100 + K)
    fused = _module_step(_layer(dq, W, b, 4, True, full_precision, "relu"), x, dy)
    plain = _module_step(_layer(dq, W, b, 4, True, full_precision), x, dy, after=torch.relu)
    # (64, 415, 1)'s only weight row is random_case's all-zero one: y is the bias on one side of 0
    print(f"y > 0: {float((plain[0] > 0).float().mean()):.3f}")
    for a, w, what in zip(fused, plain, ("y", "x.grad", "weight.grad", "bias.grad")):
        _eq(a, w, what)


# ------------------------------------------------------------------ 4. sigmoid forward
@QUANT
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_sigmoid_forward_within_derived_bound(dq, shape, full_precision):
    """|y - sigma(z)| <= 1.01 * 2^-22 * sigma(z) + 2^-126 (cpu_mlp.sigmoid_bound), z read from the
    unfused layer and sigma evaluated in float64."""
    B, K, O_ = shape
    W, b, x, _ = R.random_case(B, K, O_, seed=100 + K)
    xc = x.cuda()
    z = _layer(dq, W, b, 4, True, full_precision)(xc)[0].detach().cpu()
    y = _layer(dq, W, b, 4, True, full_precision, "sigmoid")(xc)[0].detach().cpu()
    sig = torch.sigmoid(z.double())
    _check_bound(y, sig, M.sigmoid_bound(sig), "sigmoid(z)")


@pytest.mark.parametrize("shape,bits,per_channel", [(R.SHAPES[1], 8, True), (R.SHAPES[2], 8, False),
                                                     (R.SHAPES[3], 4, True), (R.BIG_SHAPE, 4, True)],
                         ids=["B64-in415-out1-b8", "B33-in512-out256-b8", "B130-in70-out66-b4", "big-b4"])
def test_sigmoid_forward_saturates_exactly(dq, shape, bits, per_channel):
    """Exact data, |z| up to the thousands: y finite and in [0, 1], exactly 1 where z >= 18
    (expf(-z) < 2^-25 vanishes in 1 + e), exactly 0 where z <= -104 (expf overflows)."""
    B, K, O_ = shape
    W, b, x, _ = R.exact_case(B, K, O_, bits, per_channel, seed=7 + B)
    z = R.forward(x, W, b, bits, per_channel)
    c = CLayer(dq, W, b, bits, per_channel)
    c.wquant()
    _eq(c.fwd(x), z, "z")
    y = c.fwd(x, 1, act=M.SIGMOID)
    print(f"max |z| {float(z.abs().max())}, z >= 18: {int((z >= 18).sum())}, z <= -104: {int((z <= -104).sum())}")
    assert bool(torch.isfinite(y).all()) and bool(((y >= 0) & (y <= 1)).all())
    assert float(z.abs().max()) > 104
    assert bool((y[z >= 18] == 1).all()) and bool((z >= 18).any())
    assert bool((y[z <= -104] == 0).all()) and bool((z <= -104).any())
    sig = torch.sigmoid(z.double())
    _check_bound(y, sig, M.sigmoid_bound(sig), "sigmoid(z)")


# ------------------------------------------------------------------ 5. sigmoid backward, exact data
@pytest.mark.parametrize("shape,bits,per_channel", EXACT_CASES, ids=EXACT_IDS)
def test_sigmoid_backward_exact_data_bit_exact(dq, shape, bits, per_channel):
    B, K, O_ = shape
    W, b, x, dy, y = M.sigmoid_exact_case(B, K, O_, bits, per_channel, seed=7 + B)
    assert set(np.unique(y.numpy())) == {0.0, 0.25, 0.5, 0.75, 1.0} or B * O_ < 40
    s, wi, _ = R.quantize(W, b, bits, per_channel)
    want = M.backward_from_d(M.sigmoid_d(dy, y), x, wi, s)
    # the construction: a float64 evaluation gives the same values
    want64 = M.backward_from_d(M.sigmoid_d(dy.double(), y.double()), x, wi, s)
    for w, w64 in zip(want, want64):
        assert torch.equal(w.double(), w64)
    c = CLayer(dq, W, b, bits, per_channel)
    c.wquant()
    _eq(c.wi.cpu(), wi, "weight_integer")
    for got, w, what in zip(c.bwd(x, dy, 1, act=M.SIGMOID, y=y), want, ("dx", "dw", "db")):
        _eq(got, w, what)
    _, dw, db = c.bwd(x, dy, 1, want_dx=False, act=M.SIGMOID, y=y)
    _eq(dw, want[1], "dw (dx NULL)")
    _eq(db, want[2], "db (dx NULL)")


# ------------------------------------------------------------------ 6. sigmoid backward, random data
def _sigmoid_backward_bounds(x, dy, y, wi, s, extra=3):
    """float64 gradients from the f32 y the forward wrote, and gamma(m + 3) * (sum of |products|):
    the chain bounds of test_gpu_linear.test_random_data_within_chain_bound (m = out+1 for dx,
    B+2 for dw / db) widened by the three roundings of d = (dy * (1 - y)) * y."""
    B, O_ = dy.shape
    x64, wi, s = x.double(), wi.double(), s.double().expand(O_)
    g64 = M.sigmoid_d(dy.double(), y.double()) * s
    ga = (dy.double().abs() * (1.0 - y.double()).abs() * y.double().abs()) * s
    return ((g64 @ wi, R.gamma(O_ + 1 + extra) * (ga @ wi.abs())),
            ((g64.T @ x64) / s.view(-1, 1), R.gamma(B + 2 + extra) * (ga.T @ x64.abs()) / s.view(-1, 1)),
            (g64.sum(0) / s, R.gamma(B + 2 + extra) * ga.sum(0) / s))


@QUANT
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_sigmoid_backward_random_data_within_chain_bound(dq, shape, full_precision):
    B, K, O_ = shape
    W, b, x, dy = R.random_case(B, K, O_, seed=100 + K)
    if full_precision:
        wi, s = W, torch.ones(O_)
    else:
        s, wi, _ = R.quantize(W, b, 4, True)
    layer = _layer(dq, W, b, 4, True, full_precision, "sigmoid")
    y, dx, dw, db = _module_step(layer, x, dy)
    for got, (want64, bound), what in zip((dx, dw, db), _sigmoid_backward_bounds(x, dy, y, wi, s), ("dx", "dw", "db")):
        _check_bound(got, want64, bound, what)


# ------------------------------------------------------------------ 7. determinism, batch invariance
@pytest.mark.parametrize("shape,activation", [((130, 70, 66), "relu"), ((64, 415, 1), "sigmoid")],
                         ids=["relu", "sigmoid"])
def test_deterministic_and_batch_invariant_with_activation(dq, shape, activation):
    B, K, O_ = shape
    W, b, x, dy = R.random_case(B, K, O_, seed=5)
    layer = _layer(dq, W, b, 4, True, activation=activation)
    first = _module_step(layer, x, dy)
    second = _module_step(layer, x, dy)
    for a, c, what in zip(first, second, ("y", "dx", "dw", "db")):
        _eq(a, c, what + " run to run")
    y7, dx7, _, _ = _module_step(layer, x[:7].contiguous(), dy[:7].contiguous())
    _eq(y7, first[0][:7], "y of rows 0..6 alone against rows 0..6 of the batch")
    _eq(dx7, first[1][:7], "x.grad of rows 0..6 alone against rows 0..6 of the batch")


# ------------------------------------------------------------------ 8. a stack end to end
def _stacks(dq, ln, sigmoid_layer, seed):
    """The same weights fused and unfused (INT4 per channel), on the GPU."""
    np.random.seed(seed)
    fused = dq.create_mlp(ln, sigmoid_layer, per_channel=True)
    np.random.seed(seed)
    plain = dq.create_mlp(ln, sigmoid_layer, per_channel=True, fused=False)
    assert [type(l).__name__ for l in fused][1::2] == ["FusedActivation"] * (len(ln) - 1)
    assert all(isinstance(l, (nn.ReLU, nn.Sigmoid)) for l in list(plain)[1::2])
    return fused.cuda(), plain.cuda()


def _stack_step(dq, layers, x, dy):
    """Output, x.grad and the parameter gradients through apply_mlp; and per QuantLinear the
    input it saw, the tensor after its activation and that tensor's gradient."""
    xg = x.cuda().requires_grad_(True)
    for p in layers.parameters():
        p.grad = None
    seen, hooks = [], []
    for i, l in enumerate(layers):
        if isinstance(l, dq.QuantLinear):
            hooks.append(l.register_forward_hook(lambda m, a, out, i=i: seen.append([i, a[0]])))
        else:
            def keep(m, a, out, i=i):
                out.retain_grad()
                seen[-1].append(out)
            hooks.append(l.register_forward_hook(keep))
    y = dq.apply_mlp(xg, layers)
    y.backward(dy.cuda())
    for h in hooks:
        h.remove()
    trace = [(i, a.detach().cpu(), out.detach().cpu(), out.grad.cpu()) for i, a, out in seen]
    grads = [(l.weight.grad.cpu(), l.bias.grad.cpu()) for l in layers if isinstance(l, dq.QuantLinear)]
    return y, xg.grad.cpu(), grads, trace


def _grad_fn_names(t):
    names, todo, done = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in done:
            continue
        done.add(f)
        names.add(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


def test_relu_stack_fused_equals_unfused_bit_for_bit(dq):
    fused, plain = _stacks(dq, [13, 32, 16], -1, seed=21)
    rs = np.random.RandomState(22)
    x = torch.from_numpy(rs.standard_normal((33, 13)).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal((33, 16)).astype(np.float32))
    yf, dxf, gf, _ = _stack_step(dq, fused, x, dy)
    yp, dxp, gp, _ = _stack_step(dq, plain, x, dy)
    assert "ReluBackward0" in _grad_fn_names(yp)
    assert not any(n.startswith(("ReluBackward", "SigmoidBackward", "ThresholdBackward")) for n in _grad_fn_names(yf))
    assert 0.1 < float((yp > 0).float().mean()) < 0.9
    _eq(yf.detach().cpu(), yp.detach().cpu(), "output")
    _eq(dxf, dxp, "x.grad")
    for k, ((wf, bf), (wp, bp)) in enumerate(zip(gf, gp)):
        _eq(wf, wp, f"layer {k} weight.grad")
        _eq(bf, bp, f"layer {k} bias.grad")


def test_sigmoid_stack_fused_against_unfused(dq):
    """Everything up to the last layer's z passes only through ReLU layers and is bit-identical;
    the output obeys the sigmoid bound; the gradients agree with the unfused stack's to the chain
    bound of the sigmoid backward test, evaluated layer by layer on the unfused stack's tensors."""
    fused, plain = _stacks(dq, [20, 32, 1], 1, seed=23)
    rs = np.random.RandomState(24)
    B = 33
    x = torch.from_numpy(rs.standard_normal((B, 20)).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal((B, 1)).astype(np.float32))
    yf, dxf, gf, tf = _stack_step(dq, fused, x, dy)
    yp, dxp, gp, tp = _stack_step(dq, plain, x, dy)
    assert {"ReluBackward0", "SigmoidBackward0"} <= _grad_fn_names(yp)
    assert not any(n.startswith(("ReluBackward", "SigmoidBackward", "ThresholdBackward")) for n in _grad_fn_names(yf))
    # the ReLU layer's output (the last layer's input) is bit-identical
    _eq(tf[0][2], tp[0][2], "first layer's output")
    _eq(tf[1][1], tp[1][1], "last layer's input")
    z = plain[2](tp[1][1].cuda())[0].detach().cpu()
    sig = torch.sigmoid(z.double())
    _check_bound(yf.detach().cpu(), sig, M.sigmoid_bound(sig), "sigmoid(z)")
    # the last layer: d = (dy * (1 - y)) * y on the unfused stack's y
    last, first = plain[2], plain[0]
    bounds = _sigmoid_backward_bounds(tp[1][1], dy, tp[1][2], last.weight_integer.cpu(), last.fc_scaling_factor.cpu())
    for got, ref, (_, bound), what in zip((tf[0][3], gf[1][0], gf[1][1]), (tp[0][3], gp[1][0], gp[1][1]), bounds,
                                          ("last layer dx", "last layer weight.grad", "last layer bias.grad")):
        _check_bound(got, ref.double(), bound, what)
    # the first layer (ReLU): d = dy where y > 0, dy the unfused stack's gradient of its output
    y1, dy1 = tp[0][2].double(), tp[0][3].double()
    s1 = first.fc_scaling_factor.cpu().double()
    ga = M.relu_d(dy1, y1).abs() * s1
    wi1, x64 = first.weight_integer.cpu().double(), x.double()
    for got, ref, bound, what in ((dxf, dxp, R.gamma(32 + 1 + 3) * (ga @ wi1.abs()), "x.grad"),
                                  (gf[0][0], gp[0][0], R.gamma(B + 2 + 3) * (ga.T @ x64.abs()) / s1.view(-1, 1),
                                   "first layer weight.grad"),
                                  (gf[0][1], gp[0][1], R.gamma(B + 2 + 3) * ga.sum(0) / s1, "first layer bias.grad")):
        _check_bound(got, ref.double(), bound, what)


# ------------------------------------------------------------------ 9. graph capture
def test_fused_stack_forward_backward_in_a_captured_graph(dq):
    """Forward and backward of the fused bottom stack captured on one stream: the replay writes
    the eager bits, so the calls allocate nothing a capture forbids and read nothing back."""
    fused, _ = _stacks(dq, [13, 32, 16], -1, seed=21)
    params = list(fused.parameters())
    rs = np.random.RandomState(25)
    xs = [torch.from_numpy(rs.standard_normal((33, 13)).astype(np.float32)).cuda() for _ in range(2)]
    dy = torch.from_numpy(rs.standard_normal((33, 16)).astype(np.float32)).cuda()
    x = xs[0].clone()

    def step():
        y = dq.apply_mlp(x, fused)
        return (y,) + torch.autograd.grad(y, params, dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for xv in xs[::-1]:
        x.copy_(xv)
        for t in out:
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().cpu() for t in out]
        want = [t.detach().cpu() for t in step()]
        for a, w, what in zip(got, want, ["y"] + [f"grad {k}" for k in range(len(params))]):
            _eq(a, w, what)
            assert bool(torch.isfinite(a).all())


# ------------------------------------------------------------------ 10. the DP hooks
class FusedMLPDLRM(nn.Module):
    """test_gpu_linear.QuantMLPDLRM's model: emb_l / bot_l / top_l as DLRM_Net exposes them, the
    MLPs applied by apply_mlp; `fused` puts the ReLUs into the layers."""

    def __init__(self, dq, rows, D, Ws, fused):
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
        if fused:
            assert dq.fuse_activations(self.bot_l) == 2 and dq.fuse_activations(self.top_l) == 1

    def forward(self, dense, lS_o, lS_i):
        x = self.dq.apply_mlp(dense, self.bot_l)
        ly = self.emb_l(lS_o, lS_i, layout="btd")
        return self.dq.apply_mlp(torch.cat([x.unsqueeze(1), ly], dim=1).flatten(1), self.top_l)


def test_dp_hooks_leave_the_same_bits_on_a_fused_stack(dq):
    """The hook sequence of test_dp_hooks_update_package_quantlinear_layers (one DP iteration at
    world size 1) on a fused ReLU stack and on the same stack unfused."""
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients_parallel_comm as H

    rows, D, B, lr = [4, 300], 16, 96, 0.1
    lS_i = torch.from_numpy(G.pooling_one(rows, B, 20)).cuda()
    lS_o = torch.arange(B, device="cuda").repeat(len(rows), 1)
    torch.manual_seed(1)
    dense = torch.rand(B, 13, device="cuda")
    result = []
    for fused in (True, False):
        torch.manual_seed(0)
        model = FusedMLPDLRM(dq, rows, D, G.table_weights(rows, D, 12), fused)
        mlp = [l for l in list(model.bot_l) + list(model.top_l) if isinstance(l, dq.QuantLinear)]
        assert H._linear_layers(model, "bot_l") + H._linear_layers(model, "top_l") == mlp and len(mlp) == 4
        before = [l.weight.detach().cpu().clone() for l in mlp]
        H.clear_gradients(model)
        model(dense, lS_o, lS_i).pow(2).mean().backward()
        mlp_p = [(l.weight.detach().cpu().numpy().copy(), l.bias.detach().cpu().numpy().copy()) for l in mlp]
        mlp_g = [(l.weight.grad.cpu().numpy().copy(), l.bias.grad.cpu().numpy().copy()) for l in mlp]
        assert all(np.abs(gw).max() > 0 for gw, _ in mlp_g)
        H.grad_update_parallel_comm(model, 1, emb_grad_quantized=True, num_bits=8, mlp_layer_quantized=True)
        H.weight_update_parallel_comm(model, lr, emb_grad_quantized=True, num_gpus=1, mlp_layer_quantized=True)
        O.dense_dp_step(mlp_p, [mlp_g], lr, bits=8, quantized=True)  # updates mlp_p in place
        for l, (W, b), W0 in zip(mlp, mlp_p, before):
            assert not torch.equal(l.weight.detach().cpu(), W0)
            np.testing.assert_array_equal(l.weight.detach().cpu().numpy(), W)
            np.testing.assert_array_equal(l.bias.detach().cpu().numpy(), b)
        result.append([t.detach().cpu() for l in mlp for t in (l.weight, l.bias, l.weight.grad,
                                                                 l.weight_scaling_factor, l.bias_scaling_factor)])
    for a, w in zip(*result):
        _eq(a, w, "fused against unfused after the hooks")
