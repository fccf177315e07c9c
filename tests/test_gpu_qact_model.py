"""GPU: DQRMNet(quantize_activation=True): train_step / predict / evaluate (dqrm_model_step_qact /
dqrm_model_fwd_qact) against a twin model built from the same numpy seed that runs the composed
modules: ``forward`` under autograd (quant_input, the bottom stack, the tables, the interaction,
quant_feature_outputs, the top stack), ``loss.backward()``, ``tables.backward_sgd`` and the stacks'
``sgd_step``. The library calls the same exports in the same order, so every comparison is bit for
bit (np.testing.assert_array_equal takes NaNs at the same positions as equal).

The model is tests/test_gpu_model.py's: T = 3 tables of 7, 300 and 1000 rows, D = 8, ln_bot =
[5, 16, 8], ln_top = [14, 16, 1] (18 with the diagonal). B = 33, and B = 3300, where the
interaction's output crosses 16384 elements and quant_feature_outputs takes its three-launch path
(3300 * 14 = 46200) while quant_input (3300 * 5 = 16500) crosses it too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LN_EMB, D, LN_BOT = [7, 300, 1000], 8, [5, 16, 8]
LR = 0.1
FRESH, REQUANT, NO_UPDATE, EMB_READY = 1, 2, 4, 8


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _model(dq, seed=11, qbits=None, itself=False, loss="bce", th=0.0, fp=False, weight_bit=4):
    np.random.seed(seed)
    return dq.DQRMNet(LN_EMB, D, LN_BOT, [18 if itself else 14, 16, 1], arch_interaction_itself=itself,
                      quantize_bits=qbits, weight_bit=weight_bit, per_channel=False, full_precision_flag=fp,
                      quantize_activation=True, loss_function=loss, loss_threshold=th, device="cuda")


def _lins(m):
    return m.bot_stack.layers + m.top_stack.layers


def _data(dq, step, bags=False, B=33):
    rs = np.random.RandomState(100 + step)
    x = torch.from_numpy((rs.standard_normal((B, LN_BOT[0])) * (1 + step % 3)).astype(np.float32)).cuda()
    t = torch.from_numpy(rs.randint(0, 2, B).astype(np.float32)).cuda()
    if not bags:
        idx = np.stack([rs.randint(0, n, B) for n in LN_EMB]).astype(np.int64)
        return x, dq.LookupBatch.pooling_one(torch.from_numpy(idx).cuda()), t
    idx, off = [], []
    for n in LN_EMB:
        sizes = rs.randint(0, 4, B)
        off.append(torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)))
        idx.append(torch.from_numpy(rs.randint(0, n, int(sizes.sum())).astype(np.int64)))
    return x, dq.LookupBatch(idx, off, device="cuda"), t


def _np(t):
    return t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _eq(got, want, what):
    np.testing.assert_array_equal(_np(got), _np(want), err_msg=what)


def _state(m):
    """Everything a step may write: the tables with their scale and |W| maxima, both QuantActs'
    range and scale, every layer's parameters, integers, scale and correct_output_scale."""
    s = {"W": m.tables.W, "emb scale": m.tables.scale, "rowmax": m.tables.rowmax, "tmax": m.tables.tmax}
    for name, q in (("quant_input", m.quant_input), ("quant_feature_outputs", m.quant_feature_outputs)):
        s[name + " x_min"], s[name + " x_max"] = q.x_min, q.x_max
        s[name + " act_scaling_factor"] = q.act_scaling_factor
    for i, l in enumerate(_lins(m)):
        s[f"layer {i} weight"], s[f"layer {i} bias"] = l.weight, l.bias
        if not l.full_precision_flag:
            s[f"layer {i} fc_scaling_factor"] = l.fc_scaling_factor
            s[f"layer {i} weight_integer"], s[f"layer {i} bias_integer"] = l.weight_integer, l.bias_integer
            s[f"layer {i} correct_output_scale"] = l.correct_output_scale.reshape(-1)
    return {k: _np(v) for k, v in s.items()}


def _same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _grads(m):
    return [(_np(l.weight.grad), _np(l.bias.grad)) for l in _lins(m)]


def _same_grads(a, b, what):
    for i, ((dw, db), (tw, tb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(dw, tw, err_msg=f"{what}: layer {i} dw")
        np.testing.assert_array_equal(db, tb, err_msg=f"{what}: layer {i} db")


def _twin_backward(tw, x, batch, t):
    for p in tw.parameters():
        p.grad = None
    E, Z = tw.loss(tw(x, batch), t, return_clamped=True)
    E.backward()
    return _np(E), _np(Z), _grads(tw), _np(tw.emb_out.grad)


def _twin_update(tw, batch, lr=LR):
    tw.tables.backward_sgd(batch, tw.emb_out.grad, lr, ste=True, layout="btd")
    tw.bot_stack.sgd_step(lr)
    tw.top_stack.sgd_step(lr)


def _step_and_compare(m, tw, data, what, **kw):
    x, batch, t = data
    E = m.train_step(x, batch, t, LR, **kw)
    tE, tZ, tg, tdemb = _twin_backward(tw, x, batch, t)
    _twin_update(tw, batch)
    _eq(E, tE, f"{what}: loss")
    _eq(m.z, tZ, f"{what}: z")
    _same_grads(_grads(m), tg, what)
    _eq(m.emb_grad, tdemb, f"{what}: emb_grad")
    _same_state(_state(m), _state(tw), what)
    assert np.isfinite(tE) and float(np.abs(tdemb).max()) > 0 and all(float(np.abs(g[0]).max()) > 0 for g in tg)


CASES = {
    "plain-bce": dict(),
    "plain-itself-mse": dict(itself=True, loss="mse"),
    "q16-bce-threshold": dict(qbits=16, th=0.45),
    "q16-itself-mse": dict(qbits=16, itself=True, loss="mse"),
    "w8-plain-bce": dict(weight_bit=8),
    "act-only-bce": dict(fp=True),
    "act-only-q16-itself-mse": dict(fp=True, qbits=16, itself=True, loss="mse"),
}
RUNS = [(c, 33) for c in CASES] + [("plain-bce", 3300), ("q16-itself-mse", 3300), ("act-only-bce", 3300)]


# ------------------------------------------------------------------ 1. four steps, twice
@pytest.mark.parametrize("case,B", RUNS, ids=[f"{c}-B{B}" for c, B in RUNS])
def test_four_steps_equal_the_composition_and_repeat(dq, case, B):
    kw = CASES[case]
    finals = []
    for run in range(2):
        m, tw = _model(dq, **kw), _model(dq, **kw)
        assert m.quantize_activation and m.bot_stack._qact == (not kw.get("fp", False))
        _same_state(_state(m), _state(tw), "two models of one seed")
        flags = []
        for step in range(1, 5):
            data = _data(dq, step, bags=step % 2 == 0, B=B)
            _step_and_compare(m, tw, data, f"{case} B={B} run {run} step {step}")
            flags.append(m._last_flags)
            assert m.bot_stack.is_fresh() and m.top_stack.is_fresh()
        assert flags == [REQUANT] + [FRESH | REQUANT] * 3  # stale -> fresh -> fresh
        finals.append(_state(m))
        # the ranges followed the data: the running min / max of what the modules saw
        assert float(m.quant_input.x_min) < 0 < float(m.quant_input.x_max)
        assert float(m.quant_feature_outputs.act_scaling_factor) > 0
        # what the step is expected to launch: 3L + a_in + a_feat + 9 for fresh per-tensor stacks
        a = lambda n: 2 if n <= 16384 else 3  # noqa: E731
        base = 3 * 4 + a(B * 5) + a(B * (18 if kw.get("itself") else 14)) + 9 + (1 if kw.get("qbits") else 0)
        if kw.get("fp"):  # act-only: no prepare launches, one update launch
            base -= 3
        assert m.step_launches(data[1], fresh=True) == base
        if not kw.get("fp"):
            assert m.step_launches(data[1], fresh=False) == base - 2 + 2 * 4
    _same_state(finals[0], finals[1], "two runs of the same four steps")


# ------------------------------------------------------------------ 2. fixed QuantActs
@pytest.mark.parametrize("B", [33, 3300])
def test_fixed_quantacts(dq, B):
    m, tw = _model(dq, qbits=16), _model(dq, qbits=16)
    _step_and_compare(m, tw, _data(dq, 1, B=B), "step 1 (running)")
    for mm in (m, tw):
        mm.quant_input.fix()
        mm.quant_feature_outputs.fix()
    rng = [_np(t) for t in (m.quant_input.x_min, m.quant_input.x_max, m.quant_feature_outputs.x_min,
                            m.quant_feature_outputs.x_max)]
    for step in (2, 3):  # wider data than step 1's: a running range would move
        _step_and_compare(m, tw, _data(dq, step, bags=step == 2, B=B), f"step {step} (fixed)")
    for got, want in zip((m.quant_input.x_min, m.quant_input.x_max, m.quant_feature_outputs.x_min,
                          m.quant_feature_outputs.x_max), rng):
        _eq(got, want, "a fixed range does not move")
    data = _data(dq, 4, B=B)
    assert m.step_launches(data[1], fresh=True) == 3 * 4 + 1 + 1 + 9 + 1
    m.quant_input.unfix()
    tw.quant_input.unfix()
    _step_and_compare(m, tw, data, "step 4 (quant_input running again)")


# ------------------------------------------------------------------ 3. update=False
@pytest.mark.parametrize("fp", [False, True], ids=["integer", "act-only"])
def test_update_false_leaves_the_gradients_and_writes_no_parameter(dq, fp):
    m, tw = _model(dq, qbits=16, fp=fp), _model(dq, qbits=16, fp=fp)
    _step_and_compare(m, tw, _data(dq, 1), "step 1")
    x, batch, t = _data(dq, 2, bags=True)
    before = _state(m)
    E = m.train_step(x, batch, t, LR, update=False)
    assert m._last_flags == FRESH | NO_UPDATE
    tE, tZ, tg, tdemb = _twin_backward(tw, x, batch, t)
    _eq(E, tE, "loss")
    _eq(m.z, tZ, "z")
    _same_grads(_grads(m), tg, "update=False")
    _eq(m.emb_grad, tdemb, "emb_grad")
    after = _state(m)
    for k in before:  # the forward's own writes aside, nothing moved
        if k.startswith("layer") and ("weight" in k or k.endswith("bias") or "fc_scaling" in k) or k in ("W", "rowmax",
                                                                                                         "tmax"):
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    _same_state(after, _state(tw), "update=False: what the forward writes")
    assert m.bot_stack.is_fresh() and m.top_stack.is_fresh()
    # the manual update from those gradients lands where the composition's does
    m.tables.backward_sgd(batch, m.emb_grad, LR, ste=True, layout="btd")
    m.bot_stack.sgd_step(LR)
    m.top_stack.sgd_step(LR)
    _twin_update(tw, batch)
    _same_state(_state(m), _state(tw), "the manual update after update=False")
    _step_and_compare(m, tw, _data(dq, 3), "the step after")


# ------------------------------------------------------------------ 4. the next batch's forward
@pytest.mark.parametrize("B,bags", [(33, False), (33, True), (128, False)])
def test_prefetched_steps_equal_plain_steps(dq, B, bags):
    m, plain = _model(dq), _model(dq)
    data = [_data(dq, s, bags=bags, B=B) for s in range(1, 6)]
    for s in range(4):
        x, batch, t = data[s]
        E = m.train_step(x, batch, t, LR, next_batch=data[s + 1][1])
        pE = plain.train_step(x, batch, t, LR)
        assert bool(m._last_flags & EMB_READY) == (s > 0), s
        assert not plain._last_flags & EMB_READY
        _eq(E, pE, f"step {s + 1}: loss")
        _eq(m.z, plain.z, f"step {s + 1}: z")
        _same_grads(_grads(m), _grads(plain), f"step {s + 1}")
        _eq(m.emb_grad, plain.emb_grad, f"step {s + 1}: emb_grad")
        # the prefetching model has already run the next batch's forward on the updated tables
        want = plain.tables.forward(data[s + 1][1], bits=4, refresh_scale=True, layout="btd")
        _eq(m._view(m._ws[0], m._cm[1], B, batch.max_lookups, "slab"), want, f"step {s + 1}: the prefetched slab")
        _same_state(_state(m), _state(plain), f"step {s + 1}")
    one = m.tables.sgd_fwd_is_one_launch(data[0][1], data[1][1])
    assert m.step_launches(data[1][1], next_batch=data[2][1], prefetched=True, fresh=True) == \
        3 * 4 + 2 + 2 + 9 - 1 + (0 if one else 1)


# ------------------------------------------------------------------ 5. predict and evaluate
@pytest.mark.parametrize("fp", [False, True], ids=["integer", "act-only"])
@pytest.mark.parametrize("B", [33, 3300])
def test_predict_with_and_without_labels(dq, B, fp):
    m, tw = _model(dq, qbits=16, th=0.45, fp=fp), _model(dq, qbits=16, th=0.45, fp=fp)
    _step_and_compare(m, tw, _data(dq, 1, B=B), "step 1")
    for step, labels in ((2, False), (3, True), (4, False)):
        x, batch, t = _data(dq, step, bags=step == 3, B=B)
        with torch.no_grad():
            p = tw(x, batch)
            E, Z = tw.loss(p, t, return_clamped=True)
        if labels:
            gE, gZ = m.predict(x, batch, t)
            _eq(gE, E, "predict: loss")
            _eq(gZ, Z, "predict: z")
        else:
            got = m.predict(x, batch)
            assert tuple(got.shape) == (B, 1)
            _eq(got, p, "predict without labels")
        _same_state(_state(m), _state(tw), f"after predict {step}")  # the ranges follow the test data too
        assert m.bot_stack.is_fresh() and m.top_stack.is_fresh()
    # not fresh: the per-layer quantization in the forward's place
    for mm in (m, tw):
        mm.invalidate()
    x, batch, t = _data(dq, 5, B=B)
    with torch.no_grad():
        p = tw(x, batch)
    _eq(m.predict(x, batch), p, "predict, not fresh")
    _same_state(_state(m), _state(tw), "after the predict that was not fresh")


def test_evaluate_equals_the_composed_test_loop(dq):
    m, tw = _model(dq, th=0.45), _model(dq, th=0.45)
    for step in (1, 2):
        _step_and_compare(m, tw, _data(dq, step), f"step {step}")
    batches = [_data(dq, s, bags=s % 2 == 0) for s in range(3, 8)]
    got = m.evaluate(batches)
    ref = dq.DLRMMetrics(len(batches) * 33, device="cuda")
    with torch.no_grad():
        for x, batch, t in batches:
            _, Z = tw.loss(tw(x, batch), t, return_clamped=True)
            ref.update(Z, t)
    want = ref.compute()
    assert got.keys() == want.keys() and got["n"] == 5 * 33
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])
    _same_state(_state(m), _state(tw), "after evaluate")


# ------------------------------------------------------------------ 6. what the mode refuses
def test_out_of_scope_calls_raise(dq):
    m = _model(dq)
    x, batch, t = _data(dq, 1)
    with pytest.raises(NotImplementedError, match="quantize_activation"):
        m.micro_step(x, batch, t, 2)
    with pytest.raises(NotImplementedError, match="quantize_activation"):
        m.apply_micro_steps(LR, 2)
    with pytest.raises(NotImplementedError, match="quantize_activation"):
        m.quantize_embedding(4)
    np.random.seed(0)
    with pytest.raises(ValueError, match="per tensor"):
        dq.DQRMNet(LN_EMB, D, LN_BOT, [14, 16, 1], per_channel=True, quantize_activation=True, device="cuda")
    keys = list(m.state_dict().keys())
    for k in ("quant_input.x_min", "quant_input.x_max", "quant_input.act_scaling_factor",
              "quant_feature_outputs.x_min", "quant_feature_outputs.act_scaling_factor"):
        assert k in keys, k
    assert m.quant_input.activation_bit == 8 and m.quant_feature_outputs.fixed_point_quantization
    assert m.quant_input.act_range_momentum == -1
