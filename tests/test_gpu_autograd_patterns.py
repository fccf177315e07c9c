"""GPU: the embedding modules under the autograd and optimizer call patterns that real training
code uses beyond zero_grad / forward / backward / step: one module called twice in one graph,
opt.step(closure), gradient accumulation, zero_grad(set_to_none=False), retain_graph, two steps on
one backward, a second backward in grad_mode "dp", fused_sgd called twice in one graph.

QuantEmbeddingBagTwo, QuantEmbeddingBagLSQ and QuantEmbeddingBagPACT (tables of 37 and of 300
rows) and their T = 2 collections, D = 16, 4 bits, lr 0.1, B = 7 hand-written lookups a call.

Reference for W: torch's own semantics in float64 on the CPU (cpu_sparse_hook): W0 - lr * the sum,
over every lookup of every call whose gradient reached .grad, of that lookup's row gradient -- dy
for PACT and for QuantEmbeddingBagTwo (whose (dy * s) / s is dy to an ulp), cpu_quantizers' masked
dx for LSQ. Where the optimizer adds the COO: rtol 1e-5, atol 1e-6, the suite's tolerance for that
path; where the fused per-lookup step runs (a single call reaching a plain SGD step), the
oracle's emb_bwd_sgd bit for bit as well.

Every case is planned on the CPU first (the plan_* functions: inputs, references and the
precondition that the defect looked for -- a call dropped, a gradient applied once more or once
less, a stale table maximum -- moves the reference by at least 1e-3, a thousand tolerances);
test_sparse_hook_host runs the plans of every parametrisation without a device."""
import numpy as np
import pytest
import torch

import cpu_quantizers as CQ
import cpu_sparse_hook as R
import oracle as O

F32, F64 = np.float32, np.float64
D, B, BITS, LR = 16, 7, 4, 0.1
KINDS = ["two", "lsq", "pact"]
TABLES = {"n37": [37], "n300": [300], "T2": [37, 300]}
OFF = np.arange(B, dtype=np.int64)
IDX1 = np.arange(0, 7, dtype=np.int64)
IDX3 = np.array([0, 1, 2, 7, 8, 20, 21], np.int64)  # the forward after the step


def idx2_of(n, shared):
    """Disjoint from IDX1 with the table's last row, or sharing row 3 with it and row 9 twice."""
    return np.array([7, 8, 3, 9, 9, n - 1, 12] if shared else [7, 8, 9, 10, 11, 12, n - 1], np.int64)


def weights(rows, seed):
    rs = np.random.RandomState(seed)
    return [rs.uniform(-np.sqrt(1 / n), np.sqrt(1 / n), (n, D)).astype(F32) for n in rows]


def lsq_step(W):
    return F32(CQ.lsq_init_step(W, BITS) * F32(0.35))  # small enough for the clamp's mask to matter


class Ref:
    """The tables in float64, and the row gradients each kind hands to the optimizer."""

    def __init__(self, kind, Ws):
        self.kind = kind
        self.W = [np.array(W, F64) for W in Ws]
        self.s = [lsq_step(W) for W in Ws]

    def grads(self, idxs, dys):
        """One row gradient per lookup, per table, at the current W."""
        if self.kind != "lsq":
            return [np.array(dy, F64) for dy in dys]
        out = []
        for W, s, idx, dy in zip(self.W, self.s, idxs, dys):
            x = W.astype(F32)[idx]
            lo, hi, g = CQ.lsq_consts(BITS, x.size)
            q = x / CQ.lsq_s_eff(s, g)
            # the device's W differs from this one in its last bits: no element may sit on the mask's edge
            assert min(np.abs(q - lo).min(), np.abs(q - hi).min()) > 1e-5
            out.append(np.array(CQ.lsq_terms(x, dy, s, BITS)[0], F64))
        return out

    def after(self, calls, opt="sgd"):
        """The tables after one optimizer step on the summed gradient of calls = [(idxs, gs)]."""
        fn = R.sgd if opt == "sgd" else R.adagrad_first
        return [fn(W, [(idxs[t], gs[t]) for idxs, gs in calls], LR) for t, W in enumerate(self.W)]


def dys_of(seed, T):
    return [R.normal(seed + t, (B, D)) for t in range(T)]


class Plan(dict):
    __getattr__ = dict.__getitem__


# ------------------------------------------------------------------ the plans (CPU only)
def plan_two_calls(kind, rows, shared, seed=100):
    """a / g: y1 = m(idx1), y2 = m(idx2), one backward."""
    T, Ws = len(rows), weights(rows, seed)
    ref = Ref(kind, Ws)
    idx1, idx2 = [IDX1] * T, [idx2_of(n, shared) for n in rows]
    dy1, dy2 = dys_of(seed + 10, T), dys_of(seed + 20, T)
    c1, c2 = (idx1, ref.grads(idx1, dy1)), (idx2, ref.grads(idx2, dy2))
    good, no1, no2 = ref.after([c1, c2]), ref.after([c2]), ref.after([c1])
    for t in range(T):
        R.assert_visible(good[t], no1[t], idx1[t], "first call dropped")
        R.assert_visible(good[t], no2[t], idx2[t], "second call dropped")
    return Plan(Ws=Ws, idx1=idx1, idx2=idx2, dy1=dy1, dy2=dy2, good=good, ref=ref)


def plan_steps(kind, rows, seed=200):
    """b / d: three steps of one call each; refs[k] = the tables after k updates."""
    T, Ws = len(rows), weights(rows, seed)
    ref = Ref(kind, Ws)
    idx = [[IDX1] * T, [idx2_of(n, True) for n in rows], [IDX1] * T]
    dy = [dys_of(seed + 10 * (k + 1), T) for k in range(3)]
    refs = [ref.W]
    for k in range(3):
        call = (idx[k], ref.grads(idx[k], dy[k]))
        ref.W = ref.after([call])
        refs.append(ref.W)
        again = ref.after([call])
        for t in range(T):
            R.assert_visible(refs[k + 1][t], refs[k][t], idx[k][t], f"gradient {k} dropped")
            R.assert_visible(refs[k + 1][t], again[t], idx[k][t], f"gradient {k} applied twice")
    return Plan(Ws=Ws, idx=idx, dy=dy, refs=refs, steps=ref.s)


def _moving_maximum(rows, seed, first2=7):
    """Tables and micro-batch 1's dy for case c: W[0, 0] small, micro-batch 2's rows (first2 and the
    six after it) scaled down so that no step can carry the maximum into them, and dy1[0, 0] such
    that plain SGD leaves W[0, 0] at twice the old table maximum."""
    Ws = weights(rows, seed)
    dy1 = dys_of(seed + 10, len(rows))
    for W, dy in zip(Ws, dy1):
        W[0, 0] = 0.01
        W[first2:first2 + 7] *= F32(0.1)
        dy[0, 0] = F32((F64(W[0, 0]) - 2.0 * F64(np.abs(W).max())) / LR)
    return Ws, dy1


def _assert_maximum_moved(Ws, good, only1, opt, kind):
    """On the references: the new table maximum lies in a row that only micro-batch 1 touched, and a
    |W| hierarchy that missed those rows would be off by at least 1e-3."""
    for W0, W1 in zip(Ws, good):
        stale = np.abs(W1)
        stale[only1] = np.abs(W0[only1])
        row = int(np.abs(W1).max(axis=1).argmax())
        assert row in set(only1.tolist()), row
        assert np.abs(W1).max() - stale.max() >= R.VISIBLE
        if opt == "sgd":
            assert abs(W1[0, 0] - 2.0 * np.abs(W0).max()) < 1e-6


def plan_accumulate(kind, rows, opt, first2=7, seed=300):
    """c: forward 1, backward 1, forward 2, backward 2, step, forward 3. Micro-batch 1 looks up rows
    0..6, micro-batch 2 rows first2..first2 + 6: 7..13, or 290..296 of a 300-row table (its second
    256-row block). Any sync of a table of at most 256 rows rebuilds its whole |W| hierarchy from W
    (finalize_table's narrow tables), so the 37-row table alone cannot show a forgotten row: the
    300-row tables, on their own and as the collections' second table, can."""
    T = len(rows)
    Ws, dy1 = _moving_maximum(rows, seed, first2)
    ref = Ref(kind, Ws)
    idx1, idx2 = [IDX1] * T, [np.arange(first2, first2 + 7, dtype=np.int64)] * T
    dy2 = dys_of(seed + 20, T)
    c1, c2 = (idx1, ref.grads(idx1, dy1)), (idx2, ref.grads(idx2, dy2))
    good, no1 = ref.after([c1, c2], opt), ref.after([c2], opt)
    for t in range(T):
        R.assert_visible(good[t], no1[t], idx1[t], "micro-batch 1 dropped")
    _assert_maximum_moved(Ws, good, IDX1, opt, kind)
    return Plan(Ws=Ws, idx1=idx1, idx2=idx2, dy1=dy1, dy2=dy2, good=good)


def plan_eval_between(kind, rows, seed=400):
    """c, second form: forward, backward, an eval forward, an Adagrad step, forward."""
    T = len(rows)
    Ws, dy1 = _moving_maximum(rows, seed)
    ref = Ref(kind, Ws)
    idx1 = [IDX1] * T
    good = ref.after([(idx1, ref.grads(idx1, dy1))], "adagrad")
    _assert_maximum_moved(Ws, good, IDX1, "adagrad", kind)
    return Plan(Ws=Ws, idx1=idx1, idx2=[np.arange(7, 14, dtype=np.int64)] * T, dy1=dy1, good=good)


def plan_one_call(kind, rows, seed=500):
    """d (retain_graph) / e: one call; the tables after its gradient once and twice."""
    T, Ws = len(rows), weights(rows, seed)
    ref = Ref(kind, Ws)
    idx, dy = [idx2_of(n, True) for n in rows], dys_of(seed + 10, T)
    c = (idx, ref.grads(idx, dy))
    once, twice = ref.after([c]), ref.after([c, c])
    for t in range(T):
        R.assert_visible(once[t], twice[t], idx[t], "once or twice")
    return Plan(Ws=Ws, idx=idx, dy=dy, once=once, twice=twice, steps=ref.s)


# ------------------------------------------------------------------ the device side
pytestmark = pytest.mark.gpu  # the tests; the plans above are plain functions


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Dev:
    """One module (one table) or one collection (T tables) of a kind, called with per-table lookups."""

    def __init__(self, dq, kind, rows, Ws, grad_mode="sparse", lr=None, packed=False):
        from deep_quantized_recommendation_model_dqrm_amd import quant_modules_not_quantize_grad as Q

        tw = [torch.from_numpy(W.copy()) for W in Ws]
        self.kind, self.T, self.coll = kind, len(rows), len(rows) > 1
        kw = dict(grad_mode=grad_mode, lr=lr)
        if kind == "two" and self.coll:
            m = Q.QuantEmbeddingBagCollection(rows, D, BITS, weights=tw, **kw)
        elif kind == "two":
            m = Q.QuantEmbeddingBagTwo(rows[0], D, BITS, embedding_id=0, weight=tw[0], use_packed_int4=packed, **kw)
        elif kind == "lsq" and self.coll:
            m = dq.LSQEmbeddingBagCollection(rows, D, bit=BITS, weights=tw, **kw)
        elif kind == "lsq":
            m = dq.QuantEmbeddingBagLSQ(rows[0], D, BITS, embedding_id=0, weight=tw[0], bit=BITS, **kw)
        elif self.coll:
            m = dq.PACTEmbeddingBagCollection(rows, D, BITS, weights=tw, **kw)
        else:
            m = dq.QuantEmbeddingBagPACT(rows[0], D, BITS, embedding_id=0, weight=tw[0], **kw)
        if kind == "lsq":
            with torch.no_grad():
                m.quan_w_fn.s.copy_(_cuda(np.array([lsq_step(W) for W in Ws], F32)))
        self.m, self.weight, self.off = m, m.embedding_bag.weight, _cuda(OFF)

    def fwd(self, idxs, **kw):
        if self.coll:
            return self.m([self.off] * self.T, [_cuda(i) for i in idxs], **kw)
        return [self.m(_cuda(idxs[0]), self.off, **kw)]

    def fwd_bwd(self, idxs, dys, **kw):
        torch.autograd.backward(self.fwd(idxs), [_cuda(dy) for dy in dys], **kw)

    def tables(self):
        ts = self.m._tset
        return [ts.table_weight(t).detach().cpu().numpy() for t in range(ts.T)]

    def assert_tables(self, want, what):
        for t, W in enumerate(self.tables()):
            R.assert_weights(W, want[t], f"{what}, table {t}")

    def assert_refreshing_forward(self, idxs, what):
        """A training forward now sees the table as it is: QuantEmbeddingBagTwo's scale is
        oracle.table_scale of the weights read back, exactly, and its output the oracle's on them;
        PACT's output passes the quantizers' check with the read-back maximum. (LSQ: no scale.)"""
        from test_gpu_quantizers import _pact_check

        ys = [y.detach().cpu().numpy() for y in self.fwd(idxs)]
        Wd = self.tables()
        if self.kind == "two":
            got = self.m.eb_scaling_factor.detach().cpu().numpy().reshape(-1)
            for t in range(self.T):
                s = O.table_scale(Wd[t], BITS)
                assert got[t] == s, (what, t, got[t], s)
                np.testing.assert_array_equal(ys[t], O.emb_fwd(Wd[t], idxs[t], OFF, s)[0], err_msg=f"{what}, y {t}")
        elif self.kind == "pact":
            for t in range(self.T):
                _pact_check(ys[t], Wd[t], idxs[t], OFF, BITS, f"{what}, table {t}")
        assert self.m._tset.read_errors() == 0


def _oracle_sgd(kind, Wo, idx, dy, step):
    """torch's sparse SGD per lookup in lookup order on one f32 table, in place: what the fused
    optimizer step and grad_mode "fused_sgd" compute, bit for bit."""
    if kind == "two":
        assert O.emb_bwd_sgd(Wo, idx, OFF, dy, O.table_scale(Wo, BITS), LR) == 0
        return
    g = CQ.lsq_backward(Wo[idx], dy, step, BITS)[0] if kind == "lsq" else dy
    assert O.emb_bwd_sgd(Wo, idx, OFF, np.ascontiguousarray(g, dtype=F32), F32(1), LR, ste=False) == 0


def _sgd(dev):
    return torch.optim.SGD([dev.weight], lr=LR)


# ------------------------------------------------------------------ a
@pytest.mark.parametrize("shared", [False, True], ids=["disjoint", "shared_row"])
@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("kind", KINDS)
def test_a_two_calls_in_one_graph(dq, kind, tables, shared):
    rows = TABLES[tables]
    p = plan_two_calls(kind, rows, shared)
    dev = Dev(dq, kind, rows, p.Ws)
    opt = _sgd(dev)
    y1, y2 = dev.fwd(p.idx1), dev.fwd(p.idx2)
    torch.autograd.backward(y1 + y2, [_cuda(g) for g in p.dy1 + p.dy2])
    opt.step()
    dev.assert_tables(p.good, "W after two calls, one backward, one step")
    assert dev.m._sgd_pend is None
    dev.assert_refreshing_forward([IDX3] * len(rows), "the forward after it")


# ------------------------------------------------------------------ b
@pytest.mark.parametrize("tables", ["n37", "n300"])
@pytest.mark.parametrize("kind", KINDS)
def test_b_closure(dq, kind, tables):
    rows = TABLES[tables]
    p = plan_steps(kind, rows)
    dev = Dev(dq, kind, rows, p.Ws)
    opt = _sgd(dev)
    for k in range(3):
        def closure():
            opt.zero_grad()
            dev.fwd_bwd(p.idx[k], p.dy[k])

        opt.step(closure)
        dev.assert_tables(p.refs[k + 1], f"W after {k + 1} closure steps")
    assert dev.m._tset.read_errors() == 0


# ------------------------------------------------------------------ c
ACCUMULATE = ([(k, t, f, False) for k in KINDS for t, f in (("n37", 7), ("T2", 7), ("n300", 290))]
              + [("two", "n37", 7, True), ("two", "n300", 290, True)])  # (kind, tables, micro-batch 2's first row, packed)


@pytest.mark.parametrize("opt_kind", ["sgd", "adagrad"])
@pytest.mark.parametrize("kind,tables,first2,packed", ACCUMULATE,
                         ids=["-".join([k, t, f"rows{f}"] + ["packed_int4"] * p) for k, t, f, p in ACCUMULATE])
def test_c_accumulation_with_a_maximum_that_moves(dq, kind, tables, first2, packed, opt_kind):
    """Micro-batch 1 carries the table maximum into row 0, which micro-batch 2 does not touch; the
    forward between them runs before the optimizer has moved anything. The forward after the step
    must see the new maximum (and, with use_packed_int4, micro-batch 1's rows repacked)."""
    rows = TABLES[tables]
    p = plan_accumulate(kind, rows, opt_kind, first2)
    dev = Dev(dq, kind, rows, p.Ws, packed=packed)
    opt = _sgd(dev) if opt_kind == "sgd" else torch.optim.Adagrad([dev.weight], lr=LR)
    dev.fwd_bwd(p.idx1, p.dy1)
    dev.fwd_bwd(p.idx2, p.dy2)
    opt.step()
    dev.assert_tables(p.good, "W after the accumulated step")
    dev.assert_refreshing_forward([IDX3] * len(rows), "forward 3")


@pytest.mark.parametrize("tables", ["n37", "T2"])
@pytest.mark.parametrize("kind", KINDS)
def test_c_eval_forward_between_backward_and_step(dq, kind, tables):
    rows = TABLES[tables]
    p = plan_eval_between(kind, rows)
    dev = Dev(dq, kind, rows, p.Ws)
    opt = torch.optim.Adagrad([dev.weight], lr=LR)
    dev.fwd_bwd(p.idx1, p.dy1)
    with torch.no_grad():
        dev.fwd(p.idx2, test_mode=True)
    opt.step()
    dev.assert_tables(p.good, "W after the Adagrad step")
    dev.assert_refreshing_forward([IDX3] * len(rows), "the forward after the step")


# ------------------------------------------------------------------ d
@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("kind", KINDS)
def test_d_zero_grad_keeping_the_tensors(dq, kind, tables):
    """Three steps under zero_grad(set_to_none=False). Each is a single call reaching a plain SGD
    step with .grad None (the fused step cleared it), so W is the oracle's to the bit as well."""
    rows = TABLES[tables]
    p = plan_steps(kind, rows)
    dev = Dev(dq, kind, rows, p.Ws)
    opt = _sgd(dev)
    Wo = [W.copy() for W in p.Ws]
    for k in range(3):
        opt.zero_grad(set_to_none=False)
        dev.fwd_bwd(p.idx[k], p.dy[k])
        opt.step()
        dev.assert_tables(p.refs[k + 1], f"W after step {k}")
        for t in range(len(rows)):
            _oracle_sgd(kind, Wo[t], p.idx[k][t], p.dy[k][t], p.steps[t])
            np.testing.assert_array_equal(dev.tables()[t], Wo[t], err_msg=f"step {k} table {t}: not the fused step's bits")
    dev.assert_refreshing_forward([IDX3] * len(rows), "the forward after three steps")


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("kind", KINDS)
def test_d_retain_graph_two_backwards_one_step(dq, kind, tables):
    rows = TABLES[tables]
    p = plan_one_call(kind, rows)
    dev = Dev(dq, kind, rows, p.Ws)
    opt = _sgd(dev)
    ys, gs = dev.fwd(p.idx), [_cuda(dy) for dy in p.dy]
    torch.autograd.backward(ys, gs, retain_graph=True)
    torch.autograd.backward(ys, gs)
    opt.step()
    dev.assert_tables(p.twice, "W after two backwards of one graph")
    assert dev.m._sgd_pend is None
    dev.assert_refreshing_forward([IDX3] * len(rows), "the forward after it")


# ------------------------------------------------------------------ e
@pytest.mark.parametrize("tables", ["n37", "n300"])
@pytest.mark.parametrize("kind", KINDS)
def test_e_two_steps_on_one_backward(dq, kind, tables):
    """opt.step(); opt.step() with no backward between. The fused step applies the update and
    clears .grad, so the second step finds no gradient: it is a documented no-op, the gradient is
    applied ONCE (torch alone, keeping .grad, would add it again; with the fused step switched off
    it does -- test_sparse_hook_host pins both)."""
    rows = TABLES[tables]
    p = plan_one_call(kind, rows)
    dev = Dev(dq, kind, rows, p.Ws)
    opt = _sgd(dev)
    dev.fwd_bwd(p.idx, p.dy)
    opt.step()
    Wo = p.Ws[0].copy()
    _oracle_sgd(kind, Wo, p.idx[0], p.dy[0], p.steps[0])
    np.testing.assert_array_equal(dev.tables()[0], Wo)  # the fused per-lookup step, bit for bit
    dev.assert_tables(p.once, "W after the first step")
    assert dev.weight.grad is None
    opt.step()
    np.testing.assert_array_equal(dev.tables()[0], Wo)
    assert dev.m._tset.read_errors() == 0


# ------------------------------------------------------------------ f
def test_f_dp_second_backward_raises(dq):
    """grad_mode "dp" keeps ONE gradient for the hooks: a second backward while it waits raises
    instead of overwriting it; after clear_gradients, or the hooks' update, it does not."""
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients_parallel_comm as H

    rows = [37]
    p = plan_one_call("two", rows)
    dev = Dev(dq, "two", rows, p.Ws, grad_mode="dp")
    model = torch.nn.Module()
    model.emb_l = torch.nn.ModuleList([dev.m])
    model.bot_l, model.top_l = torch.nn.Sequential(), torch.nn.Sequential()
    dev.fwd_bwd(p.idx, p.dy)
    first = dev.m._pending
    with pytest.raises(RuntimeError, match=r"QuantEmbeddingBagTwo \(embedding_id=0\).*grad_update_parallel_comm"):
        dev.fwd_bwd([IDX1], p.dy)
    assert dev.m._pending is first
    H.clear_gradients(model)
    dev.fwd_bwd(p.idx, p.dy)
    H.grad_update_parallel_comm(model, 1, emb_grad_quantized=False)
    H.weight_update_parallel_comm(model, LR, emb_grad_quantized=False, num_gpus=1)
    dev.fwd_bwd(p.idx, p.dy)  # the hooks consumed the gradient: no raise
    dev.assert_tables(p.once, "W after the one update the hooks applied")
    assert dev.m._tset.read_errors() == 0


# ------------------------------------------------------------------ g
@pytest.mark.parametrize("tables", ["n37", "T2"])
@pytest.mark.parametrize("kind", KINDS)
def test_g_fused_sgd_called_twice_in_one_graph(dq, kind, tables):
    rows = TABLES[tables]
    p = plan_two_calls(kind, rows, True)

    def run():
        dev = Dev(dq, kind, rows, p.Ws, grad_mode="fused_sgd", lr=LR)
        y1, y2 = dev.fwd(p.idx1), dev.fwd(p.idx2)
        torch.autograd.backward(y1 + y2, [_cuda(g) for g in p.dy1 + p.dy2])
        assert dev.m._tset.read_errors() == 0
        return dev

    a, b = run(), run()
    a.assert_tables(p.good, "W after two fused_sgd calls in one graph")
    for x, y in zip(a.tables(), b.tables()):
        np.testing.assert_array_equal(x, y)


PLANS = ([(plan_two_calls, (k, TABLES[t], s)) for k in KINDS for t in TABLES for s in (False, True)]
         + [(plan_steps, (k, TABLES[t])) for k in KINDS for t in TABLES]
         + [(plan_accumulate, (k, TABLES[t], o, f)) for k, t, f, p in ACCUMULATE if not p for o in ("sgd", "adagrad")]
         + [(plan_eval_between, (k, TABLES[t])) for k in KINDS for t in ("n37", "T2")]
         + [(plan_one_call, (k, TABLES[t])) for k in KINDS for t in TABLES])
