"""GPU: QuantLinear (linear.py over csrc/dqrm_linear.hip) against a CPU restatement of the
reference's arithmetic (tests/cpu_linear.py: quant_modules_not_quantize_grad.py:105-211,
quant_utils.py:75-101, :196-220, :316-363).

Shapes (B, in, out): K below one k-step and odd (7, 13, 5); a single output column
(64, 415, 1); a long K loop with several tiles (33, 512, 256); ragged M, N and K edges with
several tiles in every dimension (130, 70, 66). One larger shape (1040, 1030, 1050) puts all
three products on the 64 x 64 workgroup tile, which the kernels choose from the shape."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import cpu_linear as R
import gen_inputs as G
import oracle as O

pytestmark = pytest.mark.gpu

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


def _layer(dq, W, b, bits, per_channel, full_precision=False):
    lin = nn.Linear(W.shape[1], W.shape[0])
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    q = dq.QuantLinear(weight_bit=bits, bias_bit=bits, full_precision_flag=full_precision, per_channel=per_channel)
    q.set_param(lin.cuda())
    return q


def _module_step(layer, x, dy, x_grad=True):
    """y, x.grad, weight.grad, bias.grad of one forward + backward through the module."""
    xg = x.cuda().requires_grad_(x_grad)
    layer.weight.grad = layer.bias.grad = None
    y, prev = layer(xg)
    assert prev is None
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

    def fwd(self, x, quantized=1):
        x = x.cuda().contiguous()
        y = torch.empty(x.shape[0], self.O, device="cuda")
        self.L.check(self.lib.dqrm_linear_fwd(C.byref(self.c), quantized, x.data_ptr(), x.shape[0], y.data_ptr(),
                                              self.st), "fwd")
        return y.cpu()

    def bwd(self, x, dy, quantized=1, want_dx=True):
        x, dy = x.cuda().contiguous(), dy.cuda().contiguous()
        dx = torch.empty_like(x) if want_dx else None
        dw, db = torch.empty_like(self.W), torch.empty_like(self.b)
        self.L.check(self.lib.dqrm_linear_bwd(C.byref(self.c), quantized, x.data_ptr(), dy.data_ptr(), x.shape[0],
                                              dx.data_ptr() if want_dx else None, dw.data_ptr(), db.data_ptr(),
                                              self.st), "bwd")
        return (dx.cpu() if want_dx else None), dw.cpu(), db.cpu()


def _eq(got, want, what):
    np.testing.assert_array_equal(got.numpy(), want.numpy(), err_msg=what)


# ------------------------------------------------------------------ 1. wquant, bit-exact
@pytest.mark.parametrize("shape,bits,per_channel", CASES, ids=IDS)
def test_wquant_bit_exact(dq, shape, bits, per_channel):
    B, K, O_ = shape
    W, b, x, _ = R.random_case(B, K, O_, seed=100 + K)
    s, wi, bi = R.quantize(W, b, bits, per_channel)
    n = R.qmax(bits)
    if per_channel:  # the all-zero row takes the 1e-8 clamp
        assert float(s[O_ // 2]) == float(np.float32(1e-8) / np.float32(n))
    if O_ >= 5:      # some biases saturate
        assert bool(((bi == n) | (bi == -n - 1)).any())
    c = CLayer(dq, W, b, bits, per_channel)
    c.wquant()
    _eq(c.s.cpu(), s, "scale")
    _eq(c.wi.cpu(), wi, "weight_integer")
    _eq(c.bi.cpu(), bi, "bias_integer")
    # and what the module holds after a quantized forward
    layer = _layer(dq, W, b, bits, per_channel)
    layer(x.cuda())
    _eq(layer.fc_scaling_factor.cpu(), s, "fc_scaling_factor")
    _eq(layer.weight_integer.cpu(), wi, "module weight_integer")
    _eq(layer.bias_integer.cpu(), bi, "module bias_integer")


# ------------------------------------------------------------------ 2. exact data
@pytest.mark.parametrize("shape,bits,per_channel", EXACT_CASES, ids=EXACT_IDS)
def test_exact_data_forward_backward_bit_exact(dq, shape, bits, per_channel):
    B, K, O_ = shape
    W, b, x, dy = R.exact_case(B, K, O_, bits, per_channel, seed=7 + B)
    y_r, dx_r, dw_r, db_r = R.forward_backward(x, W, b, dy, bits, per_channel)
    # the construction: a float64 evaluation of the forward gives the same values
    s, wi, bi = R.quantize(W, b, bits, per_channel)
    y64 = (x.double() @ wi.double().T + bi.double()) * s.double().view(1, -1)
    assert torch.equal(y64, y_r.double())
    assert float(wi.abs().max()) == R.qmax(bits)
    # through the module with autograd
    layer = _layer(dq, W, b, bits, per_channel)
    y, dx, dw, db = _module_step(layer, x, dy)
    _eq(y, y_r, "module y")
    _eq(dx, dx_r, "module x.grad")
    _eq(dw, dw_r, "module weight.grad")
    _eq(db, db_r, "module bias.grad")
    # through the bare C calls
    c = CLayer(dq, W, b, bits, per_channel)
    c.wquant()
    _eq(c.fwd(x), y_r, "C y")
    dx, dw, db = c.bwd(x, dy)
    _eq(dx, dx_r, "C dx")
    _eq(dw, dw_r, "C dw")
    _eq(db, db_r, "C db")
    # with dx = NULL
    _, dw, db = c.bwd(x, dy, want_dx=False)
    _eq(dw, dw_r, "C dw (dx NULL)")
    _eq(db, db_r, "C db (dx NULL)")
    y, dx, dw, db = _module_step(layer, x, dy, x_grad=False)
    assert dx is None
    _eq(dw, dw_r, "module weight.grad (input needs no gradient)")
    _eq(db, db_r, "module bias.grad (input needs no gradient)")


# ------------------------------------------------------------------ 3. random data, derived bound
def _check_bound(got, want64, bound, what):
    err = (got.double() - want64).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("full_precision", [False, True], ids=["quant", "fp32"])
@pytest.mark.parametrize("shape,bits,per_channel", CASES, ids=IDS)
def test_random_data_within_chain_bound(dq, shape, bits, per_channel, full_precision):
    """|result - float64 evaluation| <= gamma(m) * (sum of |products|), m the operation count of
    the chain: K+2 forward, B+2 for dw / db, out+1 for dx."""
    B, K, O_ = shape
    W, b, x, dy = R.random_case(B, K, O_, seed=100 + K)
    if full_precision:
        wi, bi, s = W.double(), b.double(), torch.ones(O_, dtype=torch.float64)
    else:
        s, wi, bi = (t.double() for t in R.quantize(W, b, bits, per_channel))
        s = s.expand(O_)
    x64, dy64 = x.double(), dy.double()
    layer = _layer(dq, W, b, bits, per_channel, full_precision)
    y, dx, dw, db = _module_step(layer, x, dy)
    y64 = (x64 @ wi.T + bi) * s
    _check_bound(y, y64, R.gamma(K + 2) * (x64.abs() @ wi.abs().T + bi.abs()) * s, "y")
    g64 = dy64 * s
    _check_bound(dx, g64 @ wi, R.gamma(O_ + 1) * (g64.abs() @ wi.abs()), "dx")
    _check_bound(dw, (g64.T @ x64) / s.view(-1, 1), R.gamma(B + 2) * (g64.abs().T @ x64.abs()) / s.view(-1, 1), "dw")
    _check_bound(db, g64.sum(0) / s, R.gamma(B + 2) * g64.abs().sum(0) / s, "db")


# ------------------------------------------------------------------ 4. determinism, batch invariance
def test_deterministic_and_batch_invariant(dq):
    B, K, O_ = 130, 70, 66
    W, b, x, dy = R.random_case(B, K, O_, seed=5)
    layer = _layer(dq, W, b, 4, True)
    first = _module_step(layer, x, dy)
    second = _module_step(layer, x, dy)
    for a, c, what in zip(first, second, ("y", "dx", "dw", "db")):
        _eq(a, c, what + " run to run")
    y7 = layer(x[:7].contiguous().cuda())[0].detach().cpu()
    _eq(y7, first[0][:7], "rows 0..6 alone against rows 0..6 of the batch of 130")


# ------------------------------------------------------------------ 5. hooks end to end
class QuantMLPDLRM(nn.Module):
    """emb_l / bot_l / top_l as DLRM_Net exposes them, the MLPs made of package QuantLinear
    layers applied as the reference's apply_mlp does (x, prev = layer(x, prev))."""

    def __init__(self, dq, rows, D, Ws):
        super().__init__()
        self.emb_l = dq.QuantEmbeddingBagCollection(rows, D, weights=[torch.from_numpy(w) for w in Ws],
                                                    grad_mode="dp")

        def ql(i, o):
            q = dq.QuantLinear(weight_bit=4, bias_bit=4, per_channel=True)
            q.set_param(nn.Linear(i, o).cuda())
            return q

        Z = D * (len(rows) + 1)
        self.bot_l = nn.ModuleList([ql(13, 24), nn.ReLU(), ql(24, D), nn.ReLU()])
        self.top_l = nn.ModuleList([ql(Z, 20), nn.ReLU(), ql(20, 1)])

    @staticmethod
    def _mlp(x, layers):
        prev = None
        for l in layers:
            if type(l).__name__ == "QuantLinear":
                x, prev = l(x, prev)
            else:
                x = l(x)
        return x

    def forward(self, dense, lS_o, lS_i):
        x = self._mlp(dense, self.bot_l)
        ly = self.emb_l(lS_o, lS_i, layout="btd")
        return self._mlp(torch.cat([x.unsqueeze(1), ly], dim=1).flatten(1), self.top_l)


def test_dp_hooks_update_package_quantlinear_layers(dq):
    """One DP iteration at world size 1 without set_mlp_plain_linear: the hooks select the
    package's QuantLinear layers by name and apply the dense path's documented update,
    W += (-lr * q) * s_avg, to the gradients autograd produced."""
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients_parallel_comm as H

    rows, D, B, lr = [4, 300], 16, 96, 0.1
    torch.manual_seed(0)
    model = QuantMLPDLRM(dq, rows, D, G.table_weights(rows, D, 12))
    mlp = [l for l in list(model.bot_l) + list(model.top_l) if isinstance(l, dq.QuantLinear)]
    assert H._linear_layers(model, "bot_l") + H._linear_layers(model, "top_l") == mlp and len(mlp) == 4
    lS_i = torch.from_numpy(G.pooling_one(rows, B, 20)).cuda()
    lS_o = torch.arange(B, device="cuda").repeat(len(rows), 1)
    dense = torch.rand(B, 13, device="cuda")
    H.clear_gradients(model)
    model(dense, lS_o, lS_i).pow(2).mean().backward()
    mlp_p = [(l.weight.detach().cpu().numpy().copy(), l.bias.detach().cpu().numpy().copy()) for l in mlp]
    mlp_g = [(l.weight.grad.cpu().numpy().copy(), l.bias.grad.cpu().numpy().copy()) for l in mlp]
    before = [w.copy() for w, _ in mlp_p]
    assert all(np.abs(gw).max() > 0 for gw, _ in mlp_g)
    H.grad_update_parallel_comm(model, 1, emb_grad_quantized=True, num_bits=8, mlp_layer_quantized=True)
    H.weight_update_parallel_comm(model, lr, emb_grad_quantized=True, num_gpus=1, mlp_layer_quantized=True)
    g_o, s_o = O.dense_dp_step(mlp_p, [mlp_g], lr, bits=8, quantized=True)
    for l, (W, b), (gw, gb), (sw, sb), W0 in zip(mlp, mlp_p, g_o, s_o, before):
        got = l.weight.detach().cpu().numpy()
        assert not np.array_equal(got, W0)
        np.testing.assert_array_equal(got, W)
        np.testing.assert_array_equal(l.bias.detach().cpu().numpy(), b)
        np.testing.assert_array_equal(l.weight.grad.cpu().numpy(), gw)
        np.testing.assert_array_equal(l.weight_scaling_factor.cpu().numpy(), sw)
        assert float(l.bias_scaling_factor) == float(sb[0])
