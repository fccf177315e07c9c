"""GPU: DLRMMetrics (dqrm_metrics_update / _finish, metrics.py) and DQRMNet.evaluate against the
CPU restatement (tests/cpu_metrics.py). The device is held to integers: n_pos, n_neg, n_correct,
twice_u and the sorted keys are compared with assert_array_equal; roc_auc is one float64 division of
those integers on either side, so it is compared for equality too.

Shapes: batches of 1, 63, 64, 65, 255, 257 and 2051 samples (wave and workgroup tails of the update),
smaller classes of tile - 1, tile, tile + 1 and 3 * tile + 5 keys (tile = DQRM_METRICS_SORT_TILE:
one tile, its edge, more than one), 2^18 + 3 samples (many tiles, grid-stride in the search), and
66 000 x 66 003 pairs (a sum above 2^32)."""
import warnings

import numpy as np
import pytest
import torch

import cpu_metrics as CM

pytestmark = pytest.mark.gpu

F32 = np.float32
INTS = ("n_pos", "n_neg", "n_correct", "twice_u", "flags")


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _feed(m, z, t, sizes=None):
    z, t = np.asarray(z, dtype=F32), np.asarray(t, dtype=F32)
    sizes = [z.size] if sizes is None else sizes
    assert sum(sizes) == z.size
    at = 0
    for s in sizes:
        m.update(_cuda(z[at:at + s]), _cuda(t[at:at + s]))
        at += s


def _ints(d):
    return np.array([d[k] for k in INTS], dtype=np.uint64)


def _check(dq, z, t, sizes=None, capacity=None, keys=True):
    """Feed (z, t), compute, compare every integer (and the keys' regions) with the oracle."""
    z, t = np.asarray(z, dtype=F32), np.asarray(t, dtype=F32)
    want = CM.compute(z, t)
    m = dq.DLRMMetrics(capacity or z.size)
    _feed(m, z, t, sizes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = m.compute()
    np.testing.assert_array_equal(_ints(m.raw), _ints(want))
    assert got["n"] == z.size and got["n_pos"] == want["n_pos"] and got["n_correct"] == want["n_correct"]
    assert got["test_acc"] == want["n_correct"] / z.size
    if want["n_pos"] and want["n_neg"]:
        assert got["roc_auc"] == want["roc_auc"]
    else:
        assert np.isnan(got["roc_auc"])
    if keys:
        _check_keys(m, want)
    return m, got, want


def _check_keys(m, want):
    """The smaller class's region is np.sort of its keys, byte for byte; the other region holds its
    keys as a multiset."""
    k = m.keys.cpu().numpy().view(np.uint32)
    P, N = want["n_pos"], want["n_neg"]
    kp, kn = k[:P], k[m.capacity - N:]
    if want["sorted"] == "pos":
        np.testing.assert_array_equal(kp, np.sort(want["keys_pos"]))
        np.testing.assert_array_equal(np.sort(kn), np.sort(want["keys_neg"]))
    else:
        np.testing.assert_array_equal(kn, np.sort(want["keys_neg"]))
        np.testing.assert_array_equal(np.sort(kp), np.sort(want["keys_pos"]))


def _scores(rs, n, p=0.4):
    t = (rs.rand(n) < p).astype(F32)
    z = (1.0 / (1.0 + np.exp(-(rs.standard_normal(n) + t - 0.5)))).astype(F32)
    return z, t


# ------------------------------------------------------------------ two samples
@pytest.mark.parametrize("z,t,twice_u", [([0.9, 0.1], [1, 0], 2), ([0.3, 0.3], [1, 0], 1), ([0.1, 0.9], [1, 0], 0),
                                         ([0.1, 0.9], [0, 1], 2)])
def test_two_samples(dq, z, t, twice_u):
    m, got, want = _check(dq, z, t)
    assert m.raw["twice_u"] == twice_u and got["roc_auc"] == twice_u / 2


@pytest.mark.parametrize("z,t,correct", [([0.7], [1], 1), ([0.7], [0], 0), ([0.7, 0.2, 0.6], [1, 1, 1], 2),
                                         ([0.7, 0.2, 0.6], [0, 0, 0], 1)])
def test_one_class_gives_nan_with_a_warning(dq, z, t, correct):
    m = dq.DLRMMetrics(8)
    _feed(m, z, t)
    with pytest.warns(RuntimeWarning, match="one class"):
        got = m.compute()
    assert np.isnan(got["roc_auc"]) and got["n_correct"] == correct and got["n"] == len(z)
    assert got["test_acc"] == correct / len(z) and m.raw["twice_u"] == 0


# ------------------------------------------------------------------ update tails, the multiset claim
def test_update_tails_and_batch_order(dq):
    sizes = [1, 63, 64, 65, 255, 257, 2051]
    rs = np.random.RandomState(3)
    z, t = _scores(rs, sum(sizes))
    assert z.size == 2756
    m1, got1, want = _check(dq, z, t, sizes)
    m2, got2, _ = _check(dq, z, t)                      # one batch of all 2756 samples
    rz = np.concatenate([z[a:a + s] for a, s in reversed(list(zip(np.cumsum([0] + sizes[:-1]), sizes)))])
    rt = np.concatenate([t[a:a + s] for a, s in reversed(list(zip(np.cumsum([0] + sizes[:-1]), sizes)))])
    m3, got3, _ = _check(dq, rz, rt, sizes[::-1])       # those batches in reverse order
    m4, got4, _ = _check(dq, z, t, sizes)               # a second run
    assert got1 == got2 == got3 == got4
    assert m1.raw == m2.raw == m3.raw == m4.raw
    assert 0 < want["n_pos"] < want["n_neg"]


# ------------------------------------------------------------------ sort tiles
def test_sort_tile_edges(dq):
    tile = dq._lib.DQRM_METRICS_SORT_TILE
    rs = np.random.RandomState(4)
    for k, small in enumerate((tile - 1, tile, tile + 1, 3 * tile + 5)):
        big = small + 9
        z = rs.rand(small + big).astype(F32)
        t = np.zeros(small + big, dtype=F32)
        t[rs.permutation(small + big)[:(small if k % 2 == 0 else big)]] = 1  # either class is the smaller one
        m, got, want = _check(dq, z, t, capacity=small + big + 3)
        assert min(want["n_pos"], want["n_neg"]) == small


def test_many_tiles(dq):
    rs = np.random.RandomState(5)
    n = (1 << 18) + 3
    z, t = _scores(rs, n, p=0.45)
    _check(dq, z, t, sizes=[100000, 100000, n - 200000])


# ------------------------------------------------------------------ digits
def test_digit_patterns(dq):
    rs = np.random.RandomState(6)
    n = 9000
    t = (rs.rand(n) < 0.5).astype(F32)
    # keys that differ only in the top byte: powers of 4 (an odd biased exponent, no mantissa)
    top = (F32(4.0) ** rs.randint(-30, 30, n).astype(F32)).astype(F32)
    assert np.unique(CM.keys_of(top) & np.uint32(0x00FFFFFF)).size == 1 and np.unique(CM.keys_of(top)).size > 50
    _check(dq, top, t)
    # keys that differ only in the low byte
    low = (np.uint32(0x3F000000) + rs.randint(0, 256, n).astype(np.uint32)).view(F32)
    assert np.unique(CM.keys_of(low) >> np.uint32(8)).size == 1
    _check(dq, low, t)
    # all scores identical: twice_u = P * N, AUC exactly 0.5, one bucket in every pass
    m, got, want = _check(dq, np.full(n, 0.25, dtype=F32), t)
    assert m.raw["twice_u"] == want["n_pos"] * want["n_neg"] and got["roc_auc"] == 0.5
    # seven values: heavy ties
    _check(dq, F32([0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95])[rs.randint(0, 7, n)], t)


# ------------------------------------------------------------------ both branches
@pytest.mark.parametrize("P,N", [(700, 1900), (1900, 700), (1300, 1300)])
def test_both_branches(dq, P, N):
    rs = np.random.RandomState(7)
    z = np.round(rs.rand(P + N), 2).astype(F32)  # ties between the classes
    t = np.zeros(P + N, dtype=F32)
    t[rs.permutation(P + N)[:P]] = 1
    m, got, want = _check(dq, z, t, sizes=[1000, P + N - 1000])
    assert want["sorted"] == ("pos" if P <= N else "neg")
    assert want["twice_u"] == CM.compute(z, t, "pos")["twice_u"] == CM.compute(z, t, "neg")["twice_u"]


# ------------------------------------------------------------------ the order transform
def test_order_transform(dq):
    d = F32(2.0 ** -149)
    z = F32([-3.5, -1.0, -0.25, -d, -0.0, 0.0, d, 2 * d, 0.25, 1.0, 1.0000001, 2.5, 7.0, -0.0, 0.0])
    for shift in range(4):
        t = F32([(i + shift) % 2 for i in range(z.size)])
        _check(dq, z, t)
    m, got, _ = _check(dq, F32([-0.0, 0.0]), F32([1, 0]))  # -0 against +0: a tie
    assert m.raw["twice_u"] == 1 and got["roc_auc"] == 0.5
    m, got, _ = _check(dq, F32([-d, 0.0]), F32([1, 0]))
    assert m.raw["twice_u"] == 0
    m, got, _ = _check(dq, F32([-1.0, -2.0]), F32([1, 0]))
    assert m.raw["twice_u"] == 2


def test_rounding(dq):
    for z, t, correct in ((0.5, 0, 1), (0.5, 1, 0), (0.50000006, 1, 1), (1.5, 1, 0), (1.5, 2, None), (2.5, 0, 0)):
        m = dq.DLRMMetrics(4)
        _feed(m, [z, 0.25], [t, 1])  # the second sample is never correct; both classes when t == 0
        if correct is None:  # rint(1.5) == 2, but 2 is no label
            with pytest.raises(ValueError, match="DQRM_METRICS_F_LABEL"):
                m.compute()
            assert m.raw["n_correct"] == 1
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            assert m.compute()["n_correct"] == correct, (z, t)


# ------------------------------------------------------------------ 64-bit sums
def test_sums_above_two_to_the_32(dq):
    P, N = 66000, 66003
    rs = np.random.RandomState(8)
    z = np.concatenate([0.6 + 0.4 * rs.rand(P), 0.4 * rs.rand(N)]).astype(F32)
    t = np.concatenate([np.ones(P), np.zeros(N)]).astype(F32)
    perm = rs.permutation(P + N)
    m, got, want = _check(dq, z[perm], t[perm])
    assert m.raw["twice_u"] == 2 * P * N == 8_712_396_000 > 2 ** 32 and got["roc_auc"] == 1.0


# ------------------------------------------------------------------ flags
@pytest.mark.parametrize("bad_z,bad_t,flag", [(np.nan, 1, "NONFINITE"), (np.inf, 0, "NONFINITE"),
                                              (0.5, 0.5, "LABEL"), (0.5, 2.0, "LABEL")])
def test_flags_raise_and_a_reset_clears_them(dq, bad_z, bad_t, flag):
    rs = np.random.RandomState(9)
    z, t = _scores(rs, 300)
    zb, tb = z.copy(), t.copy()
    zb[137], tb[137] = bad_z, bad_t
    m = dq.DLRMMetrics(300)
    _feed(m, zb, tb, [100, 200])
    with pytest.raises(ValueError, match="DQRM_METRICS_F_" + flag):
        m.compute()
    assert m.raw["flags"] == CM.flags_of(zb, tb) and m.n == 300
    m.reset()
    _feed(m, z, t)
    want = CM.compute(z, t)
    assert m.compute()["roc_auc"] == want["roc_auc"]
    np.testing.assert_array_equal(_ints(m.raw), _ints(want))


def test_counters_that_contradict_seen_are_flagged_not_sorted(dq):
    """A finish told of fewer samples than the counters hold (its workspace is sized from `seen`)
    sets DQRM_METRICS_F_COUNT, sorts nothing and leaves the state as it was."""
    z, t = F32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6] * 2), F32([1] * 6 + [0] * 6)
    m = dq.DLRMMetrics(16)
    _feed(m, z, t)
    before = m.keys.cpu().numpy().copy()
    m.n = 4  # the smaller class may then have 2 keys; it has 6
    with pytest.raises(ValueError, match="DQRM_METRICS_F_COUNT"):
        m.compute()
    assert m.raw["flags"] == dq._lib.DQRM_METRICS_F_COUNT and m.raw["twice_u"] == 0
    assert (m.raw["n_pos"], m.raw["n_neg"]) == (6, 6)
    np.testing.assert_array_equal(m.keys.cpu().numpy()[[0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15]],
                                  before[[0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15]])
    m.n = 12
    m.compute()
    np.testing.assert_array_equal(_ints(m.raw), _ints(CM.compute(z, t)))


# ------------------------------------------------------------------ update after finish
def test_updates_after_a_finish(dq):
    rs = np.random.RandomState(10)
    z, t = _scores(rs, 5000, p=0.55)
    m = dq.DLRMMetrics(5000)
    _feed(m, z[:3000], t[:3000], [1500, 1500])
    first = m.compute()
    w1 = CM.compute(z[:3000], t[:3000])
    np.testing.assert_array_equal(_ints(m.raw), _ints(w1))
    assert first["roc_auc"] == w1["roc_auc"]
    assert m.compute() == first  # finish again: the state stayed valid
    _feed(m, z[3000:], t[3000:], [1200, 800])
    second = m.compute()
    w2 = CM.compute(z, t)
    np.testing.assert_array_equal(_ints(m.raw), _ints(w2))
    assert second["roc_auc"] == w2["roc_auc"] and second["n"] == 5000
    _check_keys(m, w2)


# ------------------------------------------------------------------ DQRMNet.evaluate
LN_EMB, D, LN_BOT, LN_TOP = [7, 300, 1000], 8, [5, 16, 8], [14, 16, 1]


def _model(dq, th, spread=None):
    np.random.seed(21)
    m = dq.DQRMNet(LN_EMB, D, LN_BOT, LN_TOP, per_channel=True, loss_threshold=th, device="cuda")
    # the last layer in full precision: an INT4 bias could not hold the centring bias below
    m.top_stack.layers[-1].full_precision_flag = True
    if spread is not None:  # the last layer widened and centred (the same two numbers for every twin)
        with torch.no_grad():
            m.top_stack.layers[-1].weight.mul_(spread[0])
            m.top_stack.layers[-1].bias.fill_(spread[1])
    return m


def _spread(dq, batches):
    """(k, b): a scale of the last layer's weight and a bias that put the median logit of these
    batches at 0 and its 10th / 90th percentiles at -3 / +3, so that a clamp at 0.1 / 0.9 (logits of
    +-2.2) cuts a tenth of the predictions at either end and leaves the middle. A freshly initialised
    model predicts 0.5 +- little, which no clamp touches."""
    probe = _model(dq, 0.0)
    p = np.concatenate([probe.predict(x, b).cpu().numpy().ravel() for x, b, _ in batches]).astype(np.float64)
    logit = np.log(p / (1.0 - p))
    b0 = float(probe.top_stack.layers[-1].bias.item())
    lo, mid, hi = np.percentile(logit, [10, 50, 90])
    k = 6.0 / (hi - lo)
    return float(k), float(-k * (mid - b0))


def _batches(dq):
    out = []
    for k, B in enumerate([50] * 5 + [17]):
        rs = np.random.RandomState(200 + k)
        x = torch.from_numpy(rs.standard_normal((B, LN_BOT[0])).astype(F32)).cuda()
        t = torch.from_numpy(rs.randint(0, 2, B).astype(F32)).cuda()
        idx = np.stack([rs.randint(0, n, B) for n in LN_EMB]).astype(np.int64)
        out.append((x, dq.LookupBatch.pooling_one(torch.from_numpy(idx).cuda()), t))
    return out


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    return out, [n for n in names if not n.lower().startswith(("memcpy", "memset"))]


@pytest.mark.parametrize("th", [0.0, 0.1])
def test_evaluate_equals_the_oracle_on_a_predict_loop(dq, th):
    batches = _batches(dq)
    spread = _spread(dq, batches)
    m, twin = _model(dq, th, spread), _model(dq, th, spread)
    Z = np.concatenate([twin.predict(x, b, t)[1].cpu().numpy().ravel() for x, b, t in batches])
    T = np.concatenate([t.cpu().numpy() for _, _, t in batches])
    want = CM.compute(Z, T)
    at_bounds = int(np.count_nonzero((Z == F32(th)) | (Z == F32(1.0 - th))))
    print("th", th, "scores at the clamp's bounds:", at_bounds, "distinct scores:", np.unique(Z).size)
    assert np.unique(Z).size > 100
    if th:  # the clamp makes ties, within a class and between the classes
        assert np.count_nonzero(Z == F32(th)) > 2 and np.count_nonzero(Z == F32(1.0 - th)) > 2
        assert 0 < want["twice_u"] < 2 * want["n_pos"] * want["n_neg"]
    assert not (m.bot_stack.is_fresh() and m.top_stack.is_fresh())  # evaluate requantizes once
    got = m.evaluate(batches)
    assert got == {"n": 267, "n_pos": want["n_pos"], "n_correct": want["n_correct"],
                   "test_acc": want["n_correct"] / 267, "roc_auc": want["roc_auc"]}
    assert m.bot_stack.is_fresh() and m.top_stack.is_fresh()
    # a given DLRMMetrics is reset and used; a generator then needs no len; max_batches cuts
    mine = dq.DLRMMetrics(400)
    mine.update(_cuda([0.5]), _cuda([1.0]))
    assert m.evaluate(iter(batches), metrics=mine) == got
    np.testing.assert_array_equal(_ints(mine.raw), _ints(want))
    w2 = CM.compute(Z[:100], T[:100])
    assert m.evaluate(batches, max_batches=2)["roc_auc"] == w2["roc_auc"]
    with pytest.raises(ValueError, match=r"no len\(\)"):
        m.evaluate(iter(batches))
    # the finish's launches as the profiler sees them
    _, kernels = _kernels(mine.compute)
    assert len(kernels) == mine.finish_launches() == dq._lib.load().dqrm_metrics_finish_launches(267), kernels
