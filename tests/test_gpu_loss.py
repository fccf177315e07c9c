"""DLRMLoss on the GPU (csrc/dqrm_loss.hip) against the CPU restatement (tests/cpu_loss.py): what
has no transcendental in it (MSE, every gradient, the sum) bit for bit, the BCE terms within the
derived bound of the float64 form, and torch's own clamp + loss + backward on the same GPU within
bounds that follow from the two operation orders."""
import numpy as np
import pytest
import torch
from torch import nn

import cpu_loss as CL

pytestmark = pytest.mark.gpu

# 1: a single element; 63 / 64 / 65: around one wave; 255 / 256 / 257: the slot boundary and the
# first chain of length 2; 513: ragged chains; 2051: a realistic size with a tail (and a second
# batch of loads in the kernel's first slots)
SIZES = [1, 63, 64, 65, 255, 256, 257, 513, 2051]
TH = 0.1
WS = [0.3, 1.7]
KINDS = ["bce", "mse", "wbce"]


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _head(dq, kind, th):
    return dq.DLRMLoss(kind, WS if kind == "wbce" else None, th).cuda()


def _run(dq, kind, th, p, t, want_g=True):
    """dqrm_loss_fwd with every output: numpy loss (0-dim), g, z, terms."""
    m = _head(dq, kind, th)
    P, T = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    loss = torch.full((), -7.0, device="cuda")  # the kernel overwrites it: no memset, no accumulate
    g, z, terms = (torch.empty_like(P) for _ in range(3))
    m._run(P, T, loss, g if want_g else None, z, terms)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), g.cpu().numpy(), z.cpu().numpy(), terms.cpu().numpy()


def _bwd(dq, g, go):
    G, GO = torch.from_numpy(g).cuda(), torch.tensor(go, dtype=torch.float32, device="cuda")
    dp = torch.empty_like(G)
    L = dq._lib
    L.check(L.load().dqrm_loss_bwd(G.data_ptr(), GO.data_ptr(), G.numel(), dp.data_ptr(), None), "dqrm_loss_bwd")
    torch.cuda.synchronize()
    return dp.cpu().numpy()


def _bits(a, b, what):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


def _random(B, seed, lo=0.0, hi=1.0):
    rs = np.random.RandomState(seed)
    p = rs.uniform(lo, hi, B).astype(np.float32)
    if lo == 0.0:  # (0, 1): open at both ends
        p = np.clip(p, np.float32(2.0 ** -20), np.float32(1.0 - 2.0 ** -20))
    return p, rs.randint(0, 2, B).astype(np.float32)


def _edges(th):
    """p in {0, 1, lo, hi, nextafter(lo, 0), nextafter(hi, 1), 2^-130, 0.5} x t in {0, 1}."""
    _, lo, hi = CL.clamp_bounds(th if th else TH)
    ps = np.float32([0.0, 1.0, lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1)), 2.0 ** -130,
                     0.5])
    return np.repeat(ps, 2), np.tile(np.float32([0.0, 1.0]), len(ps))


# ------------------------------------------------------------------ MSE: everything bit for bit
@pytest.mark.parametrize("B", SIZES)
def test_mse_bit_exact(dq, B):
    for th in (0.0, TH):
        p, t = _random(B, 100 + B, -0.3, 1.3)  # both sides of the clamp are cut
        if B >= 63:
            _, lo, hi = CL.clamp_bounds(TH)
            p[:4] = [lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(1))]
        r = CL.forward(p, t, "mse", th)
        loss, g, z, terms = _run(dq, "mse", th, p, t)
        _bits(z, r["z"], f"z B={B} th={th}")
        _bits(terms, r["terms"], f"terms B={B} th={th}")
        _bits(g, r["g"], f"g B={B} th={th}")
        _bits(loss, r["loss"], f"loss B={B} th={th}")
        if th and B >= 63:
            assert (g == 0).any() and g[0] != 0 and g[1] != 0 and g[2] == 0 and g[3] == 0
        for go in (1.0, 0.37):
            _bits(_bwd(dq, g, go), CL.backward(r["g"], go), f"dp B={B} th={th} go={go}")


# ------------------------------------------------------------------ BCE / wbce
def _check_bce(dq, kind, th, p, t, what):
    """g bit for bit; terms within term_bound of the float64 form, exact at the saturated values;
    loss == the stated order over the GPU's own terms."""
    B = p.size
    r = CL.forward(p, t, kind, th, WS)
    loss, g, z, terms = _run(dq, kind, th, p, t)
    _bits(z, r["z"], f"z {what}")
    _bits(g, r["g"], f"g {what}")
    for go in (1.0, 0.37):
        _bits(_bwd(dq, g, go), CL.backward(r["g"], go), f"dp {what} go={go}")
    w32 = np.ones(B, dtype=np.float32) if kind == "bce" else CL.class_weights(t, WS)
    z64, t64, w64 = z.astype(np.float64), t.astype(np.float64), w32.astype(np.float64)
    want = w64 * CL.bce_terms(z64, t64)
    bound = CL.term_bound(z64, t64, w64)
    err = np.abs(terms.astype(np.float64) - want)
    print(f"{what}: terms max err {err.max():.3e}, max err/bound {(err / bound).max():.3f}")
    assert np.all(err <= bound), what
    wrong = ((z == 0) & (t == 1)) | ((z == 1) & (t == 0))
    _bits(terms[wrong], np.float32(100.0) * w32[wrong], f"the -100 floor {what}")
    ref = nn.BCELoss(reduction="none")(torch.from_numpy(z), torch.from_numpy(t)).numpy()  # torch on the CPU
    assert np.all(terms[ref == 0] == 0), what
    assert np.array_equal(ref == 0, ((z == 0) & (t == 0)) | ((z == 1) & (t == 1)))
    _bits(loss, CL.ordered_sum(terms) / np.float32(B), f"sum order {what}")
    return g, terms


@pytest.mark.parametrize("kind", ["bce", "wbce"])
@pytest.mark.parametrize("B", SIZES)
def test_bce_gradient_bit_exact_terms_within_bound_sum_in_order(dq, kind, B):
    for th in (0.0, TH):
        p, t = _random(B, 200 + B)
        _check_bce(dq, kind, th, p, t, f"{kind} B={B} th={th}")


@pytest.mark.parametrize("kind", ["bce", "wbce"])
def test_bce_edge_set(dq, kind):
    p, t = _edges(TH)
    w = np.ones(16, dtype=np.float32) if kind == "bce" else CL.class_weights(t, WS)
    # no clamp: the saturated values
    g, terms = _check_bce(dq, kind, 0.0, p, t, f"{kind} edges th=0")
    B, floor = np.float32(16), np.float32(1e-12)
    assert terms[1] == 100 * w[1] and terms[2] == 100 * w[2] and terms[0] == 0 and terms[3] == 0
    # the 1e-12 floor: p = 0, t = 1 -> w * (-1 / 1e-12f) / B; p = 1, t = 0 -> w * (1 / 1e-12f) / B
    _bits(g[1], w[1] * (np.float32(-1.0) / floor) / B, "g at p=0 t=1")
    _bits(g[2], w[2] * (np.float32(1.0) / floor) / B, "g at p=1 t=0")
    assert abs(g[1]) > 1e10 and g[0] == 0 and g[3] == 0
    assert g[13] == w[13] * (np.float32(2.0 ** -130 - 1.0) / floor) / B  # 2^-130, t = 1: the floor again
    # the clamp: p == lo and p == hi pass the gradient, one ulp outside (and 0, 1, 2^-130) does not
    g, terms = _check_bce(dq, kind, TH, p, t, f"{kind} edges th={TH}")
    assert np.all(g[[0, 1, 2, 3, 8, 9, 10, 11, 12, 13]] == 0) and np.all(g[[4, 5, 6, 7, 14, 15]] != 0)


@pytest.mark.parametrize("kind", KINDS)
def test_sum_order_on_mse_too_and_inference_only_call(dq, kind):
    """loss == ordered_sum(the GPU's terms) / B for every kind and size; g = NULL changes nothing."""
    for B in SIZES:
        p, t = _random(B, 300 + B)
        loss, _, _, terms = _run(dq, kind, TH, p, t)
        _bits(loss, CL.ordered_sum(terms) / np.float32(B), f"sum order {kind} B={B}")
        loss2, _, _, terms2 = _run(dq, kind, TH, p, t, want_g=False)
        _bits(loss2, loss, f"g=NULL loss {kind} B={B}")
        _bits(terms2, terms, f"g=NULL terms {kind} B={B}")


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("kind", KINDS)
def test_repeated_and_side_stream_calls_give_identical_bits(dq, kind):
    for B in (257, 2051):
        p, t = _random(B, 400 + B)
        m = _head(dq, kind, TH)
        P, T = torch.from_numpy(p).cuda().view(-1, 1).requires_grad_(True), torch.from_numpy(t).cuda().view(-1, 1)

        def step():
            P.grad = None
            E, Z = m(P, T, return_clamped=True)
            E.backward()
            return E.detach().clone(), Z.clone(), P.grad.clone()

        first = step()
        again = step()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = step()
        side.synchronize()
        torch.cuda.synchronize()
        for a, b, c in zip(first, again, other):
            assert torch.equal(a, b) and torch.equal(a, c)
            _bits(a.cpu().numpy(), b.cpu().numpy(), "repeat")
            _bits(a.cpu().numpy(), c.cpu().numpy(), "side stream")


# ------------------------------------------------------------------ wbce: a class with no weight
def test_wbce_out_of_range_class_is_nan_and_reads_nothing(dq):
    B = 300
    p, t = _random(B, 7)
    _, g_ok, _, terms_ok = _run(dq, "wbce", TH, p, t)
    bad = t.copy()
    bad[[5, 290]] = [2.0, -1.0]  # two weights: classes 0 and 1 only; .long() of -1 is no class here either
    loss, g, z, terms = _run(dq, "wbce", TH, p, bad)
    torch.cuda.synchronize()  # the run ends clean
    assert np.isnan(loss) and np.isnan(g[[5, 290]]).all() and np.isnan(terms[[5, 290]]).all()
    keep = np.ones(B, dtype=bool)
    keep[[5, 290]] = False
    _bits(g[keep], g_ok[keep], "the other samples' g")
    _bits(terms[keep], terms_ok[keep], "the other samples' terms")
    r = CL.forward(p, bad, "wbce", TH, WS)
    assert np.isnan(r["loss"]) and np.array_equal(np.isnan(r["g"]), np.isnan(g))


# ------------------------------------------------------------------ autograd
def _nodes(fn, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return seen
    seen.add(fn)
    for nxt, _ in fn.next_functions:
        _nodes(nxt, seen)
    return seen


@pytest.mark.parametrize("kind", KINDS)
def test_autograd_behind_the_top_mlp(dq, kind, monkeypatch):
    np.random.seed(11)
    top = dq.create_mlp([64, 415, 1], 1).cuda()  # the fused Sigmoid ends the stack
    x = torch.from_numpy(np.random.RandomState(3).standard_normal((37, 64)).astype(np.float32)).cuda()
    T = torch.from_numpy(np.random.RandomState(4).randint(0, 2, (37, 1)).astype(np.float32)).cuda()
    m = _head(dq, kind, TH)
    p = dq.apply_mlp(x, top)
    E, Z = m(p, T, return_clamped=True)
    assert E.shape == () and E.dtype == torch.float32 and Z.shape == p.shape
    assert not Z.requires_grad and Z.grad_fn is None
    names = {type(n).__name__ for n in _nodes(E.grad_fn)}
    assert any("_LossFn" in n for n in names), names
    for banned in ("ClampBackward", "BinaryCrossEntropyBackward", "MseLossBackward", "MeanBackward"):
        assert not any(n.startswith(banned) for n in names), names
    E.backward()
    for layer in top:
        if isinstance(layer, dq.QuantLinear):
            assert layer.weight.grad is not None and bool(layer.weight.grad.abs().sum() > 0)
            assert bool(torch.isfinite(layer.weight.grad).all()) and layer.bias.grad is not None
    _bits(Z.cpu().numpy().ravel(), CL.clamp(p.detach().cpu().numpy().ravel(), TH), "Z")
    assert torch.equal(dq.loss_fn_wrap(Z, T, kind, WS if kind == "wbce" else None), m(Z, T))  # way 1 == way 2
    assert torch.equal(m(p.detach(), T), E.detach())

    # p needs no gradient: no graph, no backward launch
    calls = []
    lib = dq._lib.load()
    real = lib.dqrm_loss_bwd

    class Counting:
        def __getattr__(self, name):
            if name == "dqrm_loss_bwd":
                return lambda *a: calls.append(a) or real(*a)
            return getattr(lib, name)

    monkeypatch.setattr(dq._lib, "_lib", Counting())
    E2 = m(p.detach(), T)
    assert E2.grad_fn is None and not E2.requires_grad
    T2 = T.clone().requires_grad_(True)  # a target that asks for a gradient gets none, and launches none
    E3 = m(p.detach(), T2)
    if E3.requires_grad:
        E3.backward()
    assert T2.grad is None and not calls
    P = p.detach().clone().requires_grad_(True)
    m(P, T).backward()
    assert len(calls) == 1 and P.grad is not None


# ------------------------------------------------------------------ torch's own ops on the same GPU
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 257, 2051])
def test_agreement_with_torch_on_the_same_gpu(dq, kind, B):
    """Loss: both sides hold terms within term_bound of the float64 form (the same z; MSE's two
    roundings give 2u per term) and sum them in some order; the allowance is the term bound summed
    plus the ordered-sum bound gamma_B * sum|w l|, over B.
    Gradient, u = 2^-24, go = 1 (loss.backward()), every step correctly rounded; torch divides by
    the batch size as a multiplication by r = fl(1 / B) (its scalar-divisor kernel):
      bce   here ((z - t) / den) / B                    torch ((z - t) / den) * r          u vs 2u
      mse   here (2 (z - t)) / B                         torch (fl(2 / B) * (z - t))        u vs 2u
      wbce  here (w * ((z - t) / den)) / B               torch ((r * w) * (z - t)) / den    3u vs 4u
    with z - t and den the same bits on both sides. The two results are within 3u (7u for wbce)
    of each other, relative; 1.01 for the second-order terms, 2^-148 where a result is subnormal.
    Where the clamp cuts, both are exactly 0."""
    p, t = _random(B, 500 + B, -0.2, 1.2)
    m = _head(dq, kind, TH)
    P = torch.from_numpy(p).cuda().view(-1, 1).requires_grad_(True)
    T = torch.from_numpy(t).cuda().view(-1, 1)
    E = m(P, T)
    E.backward()
    mine_g, mine_E = P.grad.cpu().numpy().ravel().astype(np.float64), float(E.detach().cpu())

    P2 = torch.from_numpy(p).cuda().view(-1, 1).requires_grad_(True)
    Z = torch.clamp(P2, min=TH, max=1.0 - TH)
    if kind == "mse":
        E2 = nn.MSELoss(reduction="mean")(Z, T)
    elif kind == "bce":
        E2 = nn.BCELoss(reduction="mean")(Z, T)
    else:
        loss_ws = torch.tensor(WS, dtype=torch.float32, device="cuda")
        E2 = (loss_ws[T.data.view(-1).long()].view_as(T) * nn.BCELoss(reduction="none")(Z, T)).mean()
    E2.backward()
    torch_g, torch_E = P2.grad.cpu().numpy().ravel().astype(np.float64), float(E2.detach().cpu())

    z64, t64 = CL.clamp(p, TH).astype(np.float64), t.astype(np.float64)
    if kind == "mse":
        exact = (z64 - t64) ** 2
        tb = 1.01 * 2 * CL.U * exact + 2.0 ** -148
    else:
        w64 = np.ones(B) if kind == "bce" else CL.class_weights(t, WS).astype(np.float64)
        exact = w64 * CL.bce_terms(z64, t64)
        tb = CL.term_bound(z64, t64, w64)
    allow = (tb.sum() + CL.gamma(B) * np.abs(exact).sum()) / B
    print(f"{kind} B={B}: loss {mine_E!r} torch {torch_E!r} diff {abs(mine_E - torch_E):.3e} allowed {allow:.3e}")
    assert abs(mine_E - torch_E) <= allow
    k = 7.0 if kind == "wbce" else 3.0
    gb = 1.01 * k * CL.U * np.abs(mine_g) + 2.0 ** -148
    gerr = np.abs(mine_g - torch_g)
    print(f"{kind} B={B}: grad max diff/bound {(gerr / gb).max():.3f}")
    assert np.all(gerr <= gb)
    cut = ~CL.clamp_mask(p, TH)
    assert np.all(mine_g[cut] == 0) and np.all(torch_g[cut] == 0) and (cut.any() or B == 1)
