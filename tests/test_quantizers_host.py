"""CPU checks of the LSQ and PACT embedding quantizers: the tests' CPU restatement
(cpu_quantizers) against torch autograd over a composition written from the contracts' formulas,
the s_eff != s case, the new exports' argument checks without a device, and the modules'
reference-named surface."""
import ctypes as C
import inspect
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_quantizers as CQ
import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _build, _lib as L

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


# ------------------------------------------------------------------ 1. the yardstick checks itself
def test_fma32_is_the_single_rounding():
    rs = np.random.RandomState(1)
    a = (rs.standard_normal(3000) * 10.0 ** rs.uniform(-6, 6, 3000)).astype(F32)
    b = (rs.standard_normal(3000) * 10.0 ** rs.uniform(-6, 6, 3000)).astype(F32)
    c = -(a.astype(np.float64) * b).astype(F32)  # cancelling: the product's low bits decide
    c[::3] = (rs.standard_normal(1000) * 10.0 ** rs.uniform(-6, 6, 1000)).astype(F32)
    got = CQ.fma32(a, b, c)

    def rn32(fr):  # round a Fraction to the nearest f32, ties to even
        if fr == 0:
            return F32(0)
        f = float(fr)  # correctly rounded to f64: a starting point two ulps wide
        cands = sorted({F32(f), np.nextafter(F32(f), F32(np.inf)), np.nextafter(F32(f), F32(-np.inf))},
                       key=lambda v: (abs(Fraction(float(v)) - fr), int(v.view(np.uint32)) & 1))
        return cands[0]

    for i in range(a.size):
        want = rn32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


def _lsq_case(B=33, D=16, seed=5):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, D)).astype(F32)
    dy = (rs.standard_normal((B, D)) * 0.1).astype(F32)
    # |x| / s > 8 clamps about a quarter of a standard normal's values at s = 1 / 7: P(|z| > 1.15) = 0.25
    s = F32(1.15 / 7.5)
    return x, dy, s


def test_lsq_restatement_equals_autograd():
    x, dy, s = _lsq_case()
    lo, hi, g = CQ.lsq_consts(4, x.size)
    st = torch.tensor([s], requires_grad=True)
    xt = torch.from_numpy(x).requires_grad_(True)
    sg = st * float(g)
    s_scale = (st - sg).detach() + sg
    q = xt / s_scale
    c = torch.clamp(q, float(lo), float(hi))
    r = (c.round() - c).detach() + c
    y = r * s_scale
    y.backward(torch.from_numpy(dy))
    clamped = float(((q < float(lo)) | (q > float(hi))).float().mean())
    assert 0.15 < clamped < 0.35, clamped
    np.testing.assert_array_equal(CQ.lsq_forward(x, s), y.detach().numpy())
    dx, ds = CQ.lsq_backward(x, dy, s)
    np.testing.assert_array_equal(dx, xt.grad.numpy())
    _, rr, gq, qs, _ = CQ.lsq_terms(x, dy, s)
    f8 = np.float64
    t1, t2 = dy.astype(f8) * rr.astype(f8), -gq.astype(f8) * qs.astype(f8)
    ds64 = (t1.sum() + t2.sum()) * f8(g)
    bound = (x.size + 4) * 2.0 ** -24 * f8(g) * (np.abs(t1).sum() + np.abs(t2).sum())
    print("ds", ds, "ds64", ds64, "autograd", float(st.grad[0]), "bound", bound)
    assert abs(f8(ds) - ds64) <= bound
    assert abs(f8(st.grad[0].item()) - ds64) <= bound


def test_chain_tree_sum_shape():
    """More than one element per chain, a ragged last sweep: the fmaf chains and the tree as
    written out by hand."""
    rs = np.random.RandomState(2)
    n = 2 * CQ.LSQ_CHAINS + 37
    a, b = rs.standard_normal(n).astype(F32), rs.standard_normal(n).astype(F32)
    acc = [F32(0)] * CQ.LSQ_CHAINS
    for e in range(n):
        c = e % CQ.LSQ_CHAINS
        acc[c] = CQ.fma32(a[e:e + 1], b[e:e + 1], np.array([acc[c]], F32))[0]
    while len(acc) > 1:
        acc = [F32(acc[i] + acc[i + 1]) for i in range(0, len(acc), 2)]
    assert CQ.chain_tree_sum(a, b) == acc[0]


@pytest.mark.parametrize("k", [2, 4, 8])
def test_pact_restatement_equals_the_torch_composition(k):
    rs = np.random.RandomState(7)
    n, D = 1000, 16
    W = rs.uniform(-np.sqrt(1 / n), np.sqrt(1 / n), (n, D)).astype(F32)
    Wt = torch.from_numpy(W)
    sc = 2 ** k - 1
    tanh = torch.tanh(Wt).float()
    want = (2 * (torch.round(sc * (tanh / (2 * torch.max(torch.abs(tanh))) + 0.5)) / sc) - 1).numpy()
    tmax = np.abs(W).max()
    got = CQ.pact_values(W, tmax, k)
    truth, near = CQ.pact_truth(W, tmax, k)
    assert near.mean() <= 0.002
    np.testing.assert_array_equal(got[~near], want[~near])
    np.testing.assert_array_equal(truth[~near], want[~near])
    print("k", k, "near-boundary share", near.mean(), "mismatches inside the band", int((got != want).sum()))


# ------------------------------------------------------------------ 2. s_eff != s
def test_restatement_uses_s_eff():
    s, B, D = CQ.find_s_eff_pair()
    g = CQ.lsq_consts(4, B * D)[2]
    se = CQ.lsq_s_eff(s, g)
    assert se != s
    x = np.full((B, D), se, F32)  # q = 1 exactly with s_eff
    x[0, 0] = F32(2.5) * se
    y = CQ.lsq_forward(x, s)
    np.testing.assert_array_equal(y[0, 1:], np.full(D - 1, se, F32))
    assert y[0, 0] == F32(2) * se  # 2.5 rounds to even
    assert np.any(y != np.rint(np.clip(x / s, -8, 7)) * s)  # the formula on s itself differs


# ------------------------------------------------------------------ 3. rejections without a device
def _fake_set(T=2, D=16):
    ts = L.TableSet()
    ts.num_tables, ts.dim = T, D
    for name, _ in L.TableSet._fields_[5:-1]:
        setattr(ts, name, 0x1000)
    return ts


def _fake_batch(B=8):
    return L.Batch(0x1000, 0x1000, 0x1000, B, B, 0, 0)


def test_exports_reject_bad_calls_without_device(lib):
    ts, ba = _fake_set(), _fake_batch()
    S, Bt, P = C.byref(ts), C.byref(ba), 0x1000
    inv = L.DQRM_E_INVALID
    # forward LSQ: set / batch / step / bits / out
    assert lib.dqrm_emb_fwd_lsq(None, Bt, P, 4, P, 128, 16, None, None) == inv
    assert lib.dqrm_emb_fwd_lsq(S, None, P, 4, P, 128, 16, None, None) == inv
    assert lib.dqrm_emb_fwd_lsq(S, Bt, None, 4, P, 128, 16, None, None) == inv
    assert b"step" in lib.dqrm_last_error()
    for bits in (1, 9):
        assert lib.dqrm_emb_fwd_lsq(S, Bt, P, bits, P, 128, 16, None, None) == inv
        assert b"bits" in lib.dqrm_last_error()
    assert lib.dqrm_emb_fwd_lsq(S, Bt, P, 4, None, 128, 16, None, None) == inv
    assert lib.dqrm_emb_fwd_lsq(S, Bt, P, 4, P + 4, 128, 16, None, None) == inv
    assert lib.dqrm_emb_fwd_lsq(S, Bt, P, 4, P, 130, 16, None, None) == inv
    bad = _fake_set(D=12)
    assert lib.dqrm_emb_fwd_lsq(C.byref(bad), Bt, P, 4, P, 128, 16, None, None) == inv
    assert b"dim" in lib.dqrm_last_error()
    # forward PACT
    assert lib.dqrm_emb_fwd_pact(None, Bt, 4, P, 128, 16, None) == inv
    assert lib.dqrm_emb_fwd_pact(S, None, 4, P, 128, 16, None) == inv
    assert lib.dqrm_emb_fwd_pact(S, Bt, 4, None, 128, 16, None) == inv
    for bits in (1, 9):
        assert lib.dqrm_emb_fwd_pact(S, Bt, bits, P, 128, 16, None) == inv
    # backward LSQ: the workspace
    need = lib.dqrm_emb_bwd_lsq_workspace_bytes(2, 8, 16)
    assert need > 0 and need % 16 == 0
    assert lib.dqrm_emb_bwd_lsq_workspace_bytes(0, 8, 16) == 0
    assert lib.dqrm_emb_bwd_lsq_workspace_bytes(2, 8, 12) == 0
    assert lib.dqrm_emb_bwd_lsq_workspace_bytes(2, -1, 16) == 0
    ok = [S, Bt, P, 128, 16, P, P, 4, P, P, P, need, None]

    def bwd(i, v):
        a = list(ok)
        a[i] = v
        return lib.dqrm_emb_bwd_lsq(*a)

    for i in (0, 1, 2, 5, 6, 8, 9, 10):  # set, batch, dy, pooled, step, dx, dstep, workspace
        assert bwd(i, None) == inv, i
    assert bwd(6, None) == inv and b"step" in lib.dqrm_last_error()
    assert bwd(7, 1) == inv and bwd(7, 9) == inv
    assert bwd(3, 126) == inv  # dy stride
    assert bwd(11, need - 1) == L.DQRM_E_WORKSPACE
    assert b"workspace" in lib.dqrm_last_error()
    # the launch queries validate the same set and batch
    for q in (lib.dqrm_emb_fwd_lsq_launches, lib.dqrm_emb_bwd_lsq_launches, lib.dqrm_emb_fwd_pact_launches):
        assert q(None, Bt) == inv and q(S, None) == inv
    assert lib.dqrm_emb_fwd_lsq_launches(S, Bt) == 1
    assert lib.dqrm_emb_bwd_lsq_launches(S, Bt) == 2
    assert lib.dqrm_emb_fwd_pact_launches(S, Bt) == 1
    empty = _fake_batch(0)
    assert lib.dqrm_emb_bwd_lsq_launches(S, C.byref(empty)) == 0


def test_python_rejects_what_is_not_built():
    from deep_quantized_recommendation_model_dqrm_amd import quant_learned_step_size_quan as QL
    from deep_quantized_recommendation_model_dqrm_amd import quant_pact_dorefa as QP

    for cls, args in ((QL.QuantEmbeddingBagLSQ, (10, 16)), (QP.QuantEmbeddingBagPACT, (10, 16, 4)),
                      (QL.LSQEmbeddingBagCollection, ([10, 20], 16)), (QP.PACTEmbeddingBagCollection, ([10, 20], 16, 4))):
        with pytest.raises(NotImplementedError, match="dp"):
            cls(*args, grad_mode="dp")
    for cls in (QL.QuantLinearLSQ, QL.QuantConv2dLSQ, QP.QuantLinearPACT, QP.QuantConv2dPACT):
        with pytest.raises(NotImplementedError, match="embedding tables"):
            cls(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError):
        QL.QuantEmbeddingBagLSQ(10, 16, bit=9)
    with pytest.raises(ValueError):
        QP.QuantEmbeddingBagPACT(10, 16, 1)


# ------------------------------------------------------------------ 4. the reference's names
class _HostSet:
    """Stands in for EmbeddingTableSet where no device exists: the rows and nothing else."""

    def __init__(self, rows, dim, device="cpu", init=None, seed=0, weights=None):
        self.num_rows, self.D, self.device = list(rows), dim, torch.device("cpu")
        self.W = torch.cat([w.to(torch.float32) for w in weights])
        self.R = self.W.shape[0]

    def table_weight(self, t):
        b = sum(self.num_rows[:t])
        return self.W[b: b + self.num_rows[t]]


def test_state_dict_keys_and_signatures(monkeypatch):
    from deep_quantized_recommendation_model_dqrm_amd import _baselines
    from deep_quantized_recommendation_model_dqrm_amd import quant_learned_step_size_quan as QL
    from deep_quantized_recommendation_model_dqrm_amd import quant_pact_dorefa as QP

    def names(fn, kind):
        return [p.name for p in inspect.signature(fn).parameters.values() if p.kind == kind and p.name != "self"]

    pos, kwo = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert names(QL.QuantEmbeddingBagLSQ.__init__, pos) == ["num_embeddings", "embedding_dim", "full_precision_flag",
                                                            "embedding_id", "quan_w_fn", "quan_a_fn"]
    assert names(QL.QuantEmbeddingBagLSQ.forward, pos) == ["input", "offsets", "full_precision_flag",
                                                           "per_sample_weights", "test_mode"]
    assert names(QP.QuantEmbeddingBagPACT.__init__, pos) == ["num_embeddings", "embedding_dim", "bitwidth",
                                                             "full_precision_flag", "embedding_id"]
    assert inspect.signature(QP.QuantEmbeddingBagPACT.__init__).parameters["bitwidth"].default == 8
    assert names(QP.QuantEmbeddingBagPACT.forward, pos) == ["input", "offsets", "per_sample_weights",
                                                            "full_precision_flag", "test_mode"]
    assert names(QL.LsqQuan.__init__, pos) == ["bit", "all_positive", "symmetric", "per_channel"]
    for cls in (QL.QuantEmbeddingBagLSQ, QP.QuantEmbeddingBagPACT):
        assert set(names(cls.__init__, kwo)) >= {"device", "weight", "init", "grad_mode", "lr"}
    for fwd in (QL.LSQEmbeddingBagCollection.forward, QP.PACTEmbeddingBagCollection.forward):
        assert names(fwd, pos) == ["lS_o", "lS_i", "full_precision_flag", "test_mode", "layout"]
    for name in ("LsqQuan", "QuantEmbeddingBagLSQ", "LSQEmbeddingBagCollection", "QuantEmbeddingBagPACT",
                 "PACTEmbeddingBagCollection"):
        assert name in dq.__all__ and hasattr(dq, name)
    assert any(s.endswith("dqrm_quantizers.hip") for s in _build.SOURCES)

    monkeypatch.setattr(_baselines, "EmbeddingTableSet", _HostSet)
    np.random.seed(3)
    m = QL.QuantEmbeddingBagLSQ(37, 16, 4, embedding_id=0, device="cpu")  # the driver's call: 4 is ignored
    assert list(m.state_dict()) == ["embedding_bag.weight", "quan_w_fn.s", "quan_a_fn.s"]
    assert m.bit == 4 and (m.quan_w_fn.thd_neg, m.quan_w_fn.thd_pos) == (-8, 7)
    assert tuple(m.quan_w_fn.s.shape) == (1,) and tuple(m.quan_a_fn.s.shape) == (1,)
    W = m.embedding_bag.weight.detach().numpy()
    assert np.abs(W).max() <= np.sqrt(1 / 37)
    assert m.quan_w_fn.s.detach().numpy()[0] == CQ.lsq_init_step(W)
    sd = m.state_dict()
    sd["quan_w_fn.s"] = torch.tensor(0.25)  # the reference's 0-d step loads
    m._tset.refresh_absmax = lambda: None
    m.load_state_dict(sd)
    assert m.quan_w_fn.s.detach().numpy().tolist() == [0.25]
    c = QL.LSQEmbeddingBagCollection([3, 37], 16, device="cpu")
    assert list(c.state_dict()) == ["embedding_bag.weight", "quan_w_fn.s"]
    for t in range(2):
        assert c.quan_w_fn.s.detach().numpy()[t] == CQ.lsq_init_step(c.table_weight(t).numpy())
    p = QP.QuantEmbeddingBagPACT(37, 16, 4, embedding_id=0, device="cpu")
    assert list(p.state_dict()) == ["embedding_bag.weight"]
    assert "bitwidth = 4" in repr(p)
    p.fix()
    assert p.fix_flag
    p.unfix()
    assert not p.fix_flag
    q = QL.LsqQuan(3, all_positive=True, per_channel=True)
    assert (q.thd_neg, q.thd_pos) == (0, 7)
    q.init_from(torch.ones(5, 2, 2))
    assert tuple(q.s.shape) == (5, 1, 1)
