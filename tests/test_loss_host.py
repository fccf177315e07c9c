"""Host-side checks of DLRMLoss: exports, the struct, constructor and argument validation, the
weight-string parse, the C calls' error returns (no device needed), and the float64 form of the
CPU restatement (tests/cpu_loss.py) against torch's own clamp / BCELoss / MSELoss / wbce."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import cpu_loss as CL
import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _build
from deep_quantized_recommendation_model_dqrm_amd import _lib as L
from deep_quantized_recommendation_model_dqrm_amd import loss as loss_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 0.1  # the clamp of the cases below: lo = 0.1, hi = 0.9


# ------------------------------------------------------------------ exports and the C ABI
def test_package_exports_and_signatures():
    assert dq.DLRMLoss is loss_mod.DLRMLoss and dq.loss_fn_wrap is loss_mod.loss_fn_wrap
    assert "DLRMLoss" in dq.__all__ and "loss_fn_wrap" in dq.__all__
    sig = inspect.signature(dq.DLRMLoss.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("loss_function", "bce"), ("loss_weights", None), ("loss_threshold", 0.0)]
    fsig = inspect.signature(dq.DLRMLoss.forward)
    assert [(n, p.default) for n, p in list(fsig.parameters.items())[1:]] == [
        ("p", inspect.Parameter.empty), ("T", inspect.Parameter.empty), ("return_clamped", False)]
    wsig = inspect.signature(dq.loss_fn_wrap)
    assert [(n, p.default) for n, p in wsig.parameters.items()] == [
        ("Z", inspect.Parameter.empty), ("T", inspect.Parameter.empty), ("loss_function", "bce"),
        ("loss_ws", None), ("loss_threshold", 0.0)]


def test_header_library_and_binding_carry_the_loss_abi():
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert re.search(r"enum\s*\{\s*DQRM_LOSS_BCE = 0, DQRM_LOSS_MSE = 1, DQRM_LOSS_WBCE = 2\s*\}", src)
    assert "typedef struct dqrm_loss {" in src and "} dqrm_loss;" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int dqrm_loss_fwd\(const dqrm_loss\* cfg, const float\* p, const float\* t, int64_t B,\s*"
                     r"float\* loss\s*, float\* g\s*,\s*float\* z\s*, float\* terms\s*,\s*void\* stream\);", code)
    assert "int dqrm_loss_bwd(const float* g, const float* go, int64_t B, float* dp, void* stream);" in code
    assert (L.DQRM_LOSS_BCE, L.DQRM_LOSS_MSE, L.DQRM_LOSS_WBCE) == (0, 1, 2)
    assert L.DQRM_ABI_VERSION == 12
    dq.build(verbose=False)
    lib = L.load()
    assert lib.dqrm_abi_version() == 12
    for name in ("dqrm_loss_fwd", "dqrm_loss_bwd"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    # dqrm_loss: 2 x i32 + 2 x f32 + i32 (+ 4 bytes of padding) + a pointer
    assert C.sizeof(L.Loss) == 32 and L.Loss.weights.offset == 24 and L.Loss.num_weights.offset == 16
    assert any(s.endswith("dqrm_loss.hip") for s in _build.SOURCES)


def test_a_library_built_before_the_loss_exports_says_rebuild_it(monkeypatch):
    """load() on a libdqrm.so of ABI 12 built before dqrm_loss_* were added: the "rebuild it"
    DQRMError, not an AttributeError."""
    dq.build(verbose=False)
    real = L.load()

    class Stale:
        def __getattr__(self, name):
            if name.startswith("dqrm_loss_"):
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(C, "CDLL", lambda path, mode=0: Stale())
    with pytest.raises(L.DQRMError, match=r"does not export dqrm_loss_fwd: rebuild it"):
        L.load()
    assert L._lib is None


def test_c_calls_reject_bad_arguments_without_device():
    dq.build(verbose=False)
    lib = L.load()
    P, T_, E, G = 0x100, 0x200, 0x300, 0x400
    assert lib.dqrm_loss_fwd(None, P, T_, 4, E, G, None, None, None) == L.DQRM_E_INVALID
    assert b"null dqrm_loss" in lib.dqrm_last_error()
    c = L.Loss()
    for kind in (-1, 3, 7):
        c.kind = kind
        assert lib.dqrm_loss_fwd(C.byref(c), P, T_, 4, E, G, None, None, None) == L.DQRM_E_INVALID
        assert b"unknown kind" in lib.dqrm_last_error()
    c.kind = L.DQRM_LOSS_WBCE
    for nw, ptr in ((2, None), (0, 0x500), (-1, 0x500)):
        c.num_weights, c.weights = nw, ptr
        assert lib.dqrm_loss_fwd(C.byref(c), P, T_, 4, E, G, None, None, None) == L.DQRM_E_INVALID
        assert b"needs weights" in lib.dqrm_last_error()
    c.num_weights, c.weights = 2, 0x500
    for kind in (L.DQRM_LOSS_BCE, L.DQRM_LOSS_MSE, L.DQRM_LOSS_WBCE):
        c.kind = kind
        for B in (0, -1, (1 << 20) + 1, 1 << 40):
            assert lib.dqrm_loss_fwd(C.byref(c), P, T_, B, E, G, None, None, None) == L.DQRM_E_INVALID
            assert b"B must be 1..1048576" in lib.dqrm_last_error()
        for args in ((None, T_, 4, E), (P, None, 4, E), (P, T_, 4, None)):
            assert lib.dqrm_loss_fwd(C.byref(c), *args, G, None, None, None) == L.DQRM_E_INVALID
            assert b"null p / t / loss" in lib.dqrm_last_error()
    for B in (0, -3, (1 << 20) + 1):
        assert lib.dqrm_loss_bwd(G, E, B, P, None) == L.DQRM_E_INVALID
        assert b"B must be" in lib.dqrm_last_error()
    for args in ((None, E, 4, P), (G, None, 4, P), (G, E, 4, None)):
        assert lib.dqrm_loss_bwd(*args, None) == L.DQRM_E_INVALID
        assert b"null g / go / dp" in lib.dqrm_last_error()


# ------------------------------------------------------------------ constructor and arguments
def test_constructor_validation_and_buffer():
    with pytest.raises(ValueError, match="unknown loss_function"):
        dq.DLRMLoss("hinge")
    with pytest.raises(ValueError, match="needs loss_weights"):
        dq.DLRMLoss("wbce")
    for bad in ("1.0-x", "", "1.0--2.0", [[1.0, 2.0]], [], torch.ones(2, 2)):
        with pytest.raises(ValueError):
            dq.DLRMLoss("wbce", bad)
    m = dq.DLRMLoss("wbce", "1.0-2.5", 0.05)
    assert m.loss_ws.dtype == torch.float32 and m.loss_ws.tolist() == [1.0, 2.5]
    assert [n for n, _ in m.named_buffers()] == ["loss_ws"] and not m.state_dict() and not list(m.parameters())
    assert m.double().loss_threshold == 0.05  # nn.Module's machinery works on it
    assert dq.DLRMLoss().loss_ws is None and not dq.DLRMLoss().state_dict()
    assert "bce" in repr(dq.DLRMLoss())
    c = m.float()._config()
    assert (c.kind, c.clamp, c.num_weights) == (L.DQRM_LOSS_WBCE, 1, 2)
    assert c.lo == float(np.float32(0.05)) and c.hi == float(np.float32(1.0 - 0.05))
    d = dq.DLRMLoss("bce", None, 0.357595)._config()  # a threshold where the subtraction's precision shows
    assert d.hi == float(np.float32(1.0 - 0.357595)) != float(np.float32(1.0) - np.float32(0.357595))
    for th in (0.0, 1.0, -0.1, 1.5):
        assert dq.DLRMLoss("bce", None, th)._config().clamp == 0
    assert dq.DLRMLoss("mse", None, 0.5)._config().kind == L.DQRM_LOSS_MSE


def test_weight_parse_matches_the_reference_parse():
    for s in ("1.0-1.0", "0.25-4", "1-2.5-0.125", "3"):
        want = np.fromstring(s, dtype=float, sep="-")  # the reference's parse
        got = loss_mod.parse_loss_weights(s)
        assert got.dtype == torch.float32 and got.tolist() == want.astype(np.float32).tolist()
    w64 = torch.tensor([0.1, 0.7], dtype=torch.float64)
    assert torch.equal(loss_mod.parse_loss_weights(w64), w64.float())       # cast to f32 once
    assert torch.equal(loss_mod.parse_loss_weights([0.1, 0.7]), w64.float())
    assert torch.equal(loss_mod.parse_loss_weights(np.array([0.1, 0.7])), w64.float())
    assert torch.equal(loss_mod.parse_loss_weights((1, 2)), torch.tensor([1.0, 2.0]))


def test_forward_argument_errors():
    m = dq.DLRMLoss("bce", None, TH)
    p, t = torch.rand(6, 1), torch.ones(6, 1)
    with pytest.raises(L.DQRMError, match="no CPU path"):
        m(p, t)
    with pytest.raises(L.DQRMError):
        dq.loss_fn_wrap(p, t)
    with pytest.raises(L.DQRMError):
        dq.DLRMLoss("wbce", [1.0, 2.0])(p, t, return_clamped=True)
    with pytest.raises(L.DQRMError):
        m(p.view(-1), t.view(-1))
    with pytest.raises(ValueError, match="float32"):
        m(p.double(), t)
    with pytest.raises(ValueError, match="float32"):
        m(p, t.long())
    with pytest.raises(ValueError, match="contiguous"):
        m(torch.rand(6, 2)[:, :1], t)
    with pytest.raises(ValueError, match="contiguous"):
        m(p, torch.ones(6, 2)[:, :1])
    with pytest.raises(ValueError, match=r"\[B, 1\] or \[B\]"):
        m(torch.rand(3, 2), torch.ones(3, 2))
    with pytest.raises(ValueError, match=r"\[B, 1\] or \[B\]"):
        m(torch.rand(()), torch.ones(()))
    with pytest.raises(ValueError, match="elements"):
        m(p, torch.ones(5, 1))
    with pytest.raises(ValueError, match="samples"):
        m(torch.rand(0, 1), torch.ones(0, 1))
    with pytest.raises(TypeError):
        m(p, [1.0] * 6)
    with pytest.raises(ValueError, match="unknown loss_function"):
        dq.loss_fn_wrap(p, t, "hinge")
    with pytest.raises(ValueError, match="needs loss_ws"):
        dq.loss_fn_wrap(p, t, "wbce")


# ------------------------------------------------------------------ the restatement against torch
def _cases():
    """p, t in float64: random interior values, then p exactly 0 and 1, equal to lo and to hi and
    just outside each bound (both as doubles and as the f32 bounds), crossed with t in {0, 1}."""
    rs = np.random.RandomState(5)
    lo32, hi32 = float(np.float32(TH)), float(np.float32(1.0 - TH))
    edge = [0.0, 1.0, TH, 1.0 - TH, np.nextafter(TH, 0.0), np.nextafter(1.0 - TH, 1.0), np.nextafter(TH, 1.0),
            np.nextafter(1.0 - TH, 0.0), lo32, hi32, float(np.nextafter(np.float32(TH), np.float32(0))),
            float(np.nextafter(np.float32(1.0 - TH), np.float32(1))), 2.0 ** -130, 0.5, 0.05, 0.95, 1e-10]
    p = np.concatenate([rs.uniform(0.0, 1.0, 300), np.repeat(edge, 2)])
    t = np.concatenate([rs.randint(0, 2, 300).astype(np.float64), np.tile([0.0, 1.0], len(edge))])
    return p, t


WS = [0.25, 1.5]  # exact in f32: the restatement's single f32 cast changes nothing


def _torch_reference(p, t, kind, th):
    """The reference's head in float64 with autograd: forward's clamp, then loss_fn_wrap."""
    P = torch.from_numpy(p).view(-1, 1).clone().requires_grad_(True)
    T = torch.from_numpy(t).view(-1, 1)
    Z = torch.clamp(P, min=th, max=1.0 - th) if 0.0 < th < 1.0 else P
    if kind == "mse":
        terms = nn.MSELoss(reduction="none")(Z, T)
        E = nn.MSELoss(reduction="mean")(Z, T)
    elif kind == "bce":
        terms = nn.BCELoss(reduction="none")(Z, T)
        E = nn.BCELoss(reduction="mean")(Z, T)
    else:
        loss_ws = torch.tensor(WS, dtype=torch.float64)
        terms = loss_ws[T.data.view(-1).long()].view_as(T) * nn.BCELoss(reduction="none")(Z, T)
        E = terms.mean()
    E.backward()
    return Z.detach().numpy().ravel(), terms.detach().numpy().ravel(), float(E.detach()), P.grad.numpy().ravel()


@pytest.mark.parametrize("kind", ["bce", "mse", "wbce"])
@pytest.mark.parametrize("th", [0.0, TH])
def test_float64_restatement_agrees_with_torch(kind, th):
    p, t = _cases()
    z, terms, E, grad = _torch_reference(p, t, kind, th)
    r = CL.forward(p, t, kind, th, WS, dtype=np.float64)
    assert np.array_equal(r["z"], z)
    eps = 2.0 ** -52
    # the same operations in the same order: at most an ulp or two where torch's vectorised log /
    # log1p and numpy's differ in the last bit
    assert np.all(np.abs(r["terms"] - terms) <= 4 * eps * np.abs(terms) + 1e-300)
    assert np.all(np.abs(r["g"] - grad) <= 4 * eps * np.abs(grad) + 1e-300)
    assert np.array_equal(r["g"] == 0, grad == 0)  # the clamp's mask, bounds inclusive
    B = p.size
    assert abs(float(r["loss"]) - E) <= (B * eps) * np.abs(terms).sum() / B + 4 * eps * abs(E)
    if th:
        cut = (p < th) | (p > 1.0 - th)
        assert cut.any() and np.all(r["g"][cut] == 0) and np.all(r["g"][~cut & (p != t)] != 0)
        assert np.all(r["g"][(p == th) | (p == 1.0 - th)] != 0)
    elif kind != "mse":  # the saturated values: the log's floor and the 1e-12 floor of the gradient
        assert np.array_equal(r["terms"][(p == 0) & (t == 1)], [100.0 * (WS[1] if kind == "wbce" else 1.0)])
        assert np.array_equal(r["terms"][(p == 1) & (t == 0)], [100.0 * (WS[0] if kind == "wbce" else 1.0)])
        assert np.all(r["terms"][(p == 0) & (t == 0)] == 0) and np.all(r["terms"][(p == 1) & (t == 1)] == 0)
        w1 = WS[1] if kind == "wbce" else 1.0
        assert np.array_equal(r["g"][(p == 0) & (t == 1)], [w1 * (-1.0 / float(np.float32(1e-12))) / B])


def test_checked_facts_of_torchs_formula():
    """What the kernel's formula rests on: log1p (not log(1 - z)), the -100 floor, the inclusive
    clamp bounds."""
    f = nn.BCELoss(reduction="none")
    assert float(f(torch.tensor([1e-10]), torch.tensor([0.0]))) == float(np.float32(1e-10))
    assert float(f(torch.tensor([1.0]), torch.tensor([0.0]))) == 100.0
    x = torch.tensor([0.1, 0.95], requires_grad=True)
    torch.clamp(x, min=0.1, max=0.9).sum().backward()
    assert x.grad.tolist() == [1.0, 0.0]
    r = CL.forward(np.float32([1e-10, 1.0]), np.float32([0, 0]), "bce")
    assert r["terms"].tolist() == [float(np.float32(1e-10)), 100.0]


# ------------------------------------------------------------------ the restatement's own invariants
def test_ordered_sum_is_the_stated_order():
    rs = np.random.RandomState(2)
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 2051):
        x = (rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4, n)).astype(np.float32)
        slot = [np.float32(0.0)] * 256
        for i in range(n):  # the definition, element by element
            slot[i % 256] = np.float32(slot[i % 256] + x[i])
        stride = 128
        while stride:
            for s in range(stride):
                slot[s] = np.float32(slot[s] + slot[s + stride])
            stride //= 2
        got = CL.ordered_sum(x)
        assert got.dtype == np.float32 and got.tobytes() == slot[0].tobytes()
    # the order shows: slots 1 and 129 meet at stride 128 (1 + 1) before slot 0's 2^24 takes them in;
    # added to 2^24 one at a time, each 1 would be rounded away
    x = np.float32([2.0 ** 24, 1.0] + [0.0] * 127 + [1.0])
    assert float(CL.ordered_sum(x)) == 2.0 ** 24 + 2.0
    assert float(np.float32(np.float32(x[0] + x[1]) + x[129])) == 2.0 ** 24


def test_f32_restatement_steps_and_class_weights():
    r = CL.forward(np.float32([0.05, 0.5, 0.95, 0.1, 0.9]), np.float32([1, 0, 1, 0, 1]), "mse", TH)
    lo, hi = np.float32(TH), np.float32(1.0 - TH)
    assert r["z"].tolist() == [float(lo), 0.5, float(hi), float(lo), float(hi)]
    assert r["g"][0] == 0 and r["g"][2] == 0 and r["g"][3] != 0 and r["g"][4] != 0
    assert r["g"][1] == np.float32(np.float32(2.0) * np.float32(0.5)) / np.float32(5.0)
    assert r["loss"].dtype == np.float32
    w = CL.class_weights(np.float32([0, 1, 1.9, -0.5, 2, -1, np.nan, 1e30]), [3.0, 5.0])
    assert w[:4].tolist() == [3.0, 5.0, 5.0, 3.0] and np.isnan(w[4:]).all()
    nanp = CL.forward(np.float32([np.nan, 0.5]), np.float32([1, 1]), "bce", TH)
    assert np.isnan(nanp["z"][0]) and np.isnan(nanp["g"][0]) and np.isnan(nanp["loss"]) and nanp["g"][1] != 0


def test_term_bound_holds_for_a_correctly_rounded_f32_evaluation():
    """The bound against a model of the kernel whose logs are correctly rounded (half an ulp, inside
    the 1 ulp the bound allows): float64 logs rounded to f32, then the f32 steps."""
    p, t = _cases()
    z = CL.clamp(p.astype(np.float32), 0.0)
    t32 = t.astype(np.float32)
    w = CL.class_weights(t32, [0.3, 1.7])
    with np.errstate(divide="ignore"):
        a = np.maximum(np.log1p(-z.astype(np.float64)), -100.0).astype(np.float32)
        b = np.maximum(np.log(z.astype(np.float64)), -100.0).astype(np.float32)
    terms32 = w * ((t32 - np.float32(1.0)) * a - t32 * b)
    assert terms32.dtype == np.float32
    z64, t64, w64 = z.astype(np.float64), t32.astype(np.float64), w.astype(np.float64)
    terms64 = w64 * CL.bce_terms(z64, t64)
    bound = CL.term_bound(z64, t64, w64)
    assert np.all(np.abs(terms32.astype(np.float64) - terms64) <= bound)
    assert np.all(bound <= 8.1 * 2.0 ** -24 * np.abs(terms64) + 2.0 ** -146)  # a few ulp, never loose
