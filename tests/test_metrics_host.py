"""Host-side checks of DLRMMetrics: the CPU restatement (tests/cpu_metrics.py) against what sklearn
and numpy said (tests/golden/metrics.npz), the exports, the structs, every rejection of the C calls
on made-up addresses (no device needed), and the argument errors of DLRMMetrics and
DQRMNet.evaluate."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cpu_metrics as CM
import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _build
from deep_quantized_recommendation_model_dqrm_amd import _lib as L
from deep_quantized_recommendation_model_dqrm_amd import metrics as metrics_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["uniform", "sigmoid", "ties7", "clamped", "separated", "negdenorm", "rounding"]
# measured on this fixture with Fraction: the largest |oracle's exact rational - sklearn's float64|
# is 1.071 * 2^-53 (case "sigmoid"); the bound is 4 x that, rounded up to a whole multiple of 2^-53
AUC_MEASURED = 1.071 * 2.0 ** -53
AUC_BOUND = Fraction(5, 2 ** 53)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


# ------------------------------------------------------------------ the oracle
def test_fixture_has_every_case(golden):
    assert str(golden["sklearn_version"]) == "1.7.2"
    for name in CASES:
        z, t = golden[name + "_z"], golden[name + "_t"]
        assert z.dtype == np.float32 and t.dtype == np.uint8 and z.shape == t.shape and set(np.unique(t)) == {0, 1}


@pytest.mark.parametrize("name", CASES)
def test_oracle_against_sklearn_and_numpy(golden, name):
    """The counts are equal; the oracle's exact AUC (a Fraction) is within 5 * 2^-53 of sklearn's
    float64. Measured on this fixture: at most 1.071 * 2^-53 (sklearn's trapezoid is an m-term
    float64 sum whose rounding moves with the data; the bound is 4 x the measurement rounded up to
    a multiple of 2^-53). The tolerance touches this link alone: the device is held to integers."""
    z, t = golden[name + "_z"], golden[name + "_t"].astype(np.float32)
    a, b = CM.compute(z, t, "neg"), CM.compute(z, t, "pos")
    assert a["twice_u"] == b["twice_u"] == CM.compute(z, t)["twice_u"]  # the two branches: one number
    assert a["flags"] == 0 and a["n"] == z.size and a["n_pos"] == int(t.sum())
    assert a["n_correct"] == int(golden[name + "_correct"])
    err = abs(a["roc_auc_exact"] - Fraction(float(golden[name + "_auc"])))
    print(name, "auc error in 2^-53:", float(err * 2 ** 53))
    assert err <= AUC_BOUND
    assert abs(Fraction(a["roc_auc"]) - a["roc_auc_exact"]) <= Fraction(1, 2 ** 54)  # one rounding
    assert AUC_MEASURED * 4 <= float(AUC_BOUND)


def test_oracle_keys_order_and_rounding():
    f = np.float32
    z = f([-np.inf, -3.0, -1.0, -2.0 ** -149, -0.0, 0.0, 2.0 ** -149, 0.5, 1.0, 1.5, np.inf])
    k = CM.keys_of(z)
    assert k.dtype == np.uint32 and k[4] == k[5] == 0x80000000  # -0 ties with +0
    assert np.all(np.diff(k.astype(np.int64))[[0, 1, 2, 3, 5, 6, 7, 8, 9]] > 0)
    # ties to even: 0.5 -> 0, 1.5 -> 2
    assert CM.n_correct(f([0.5, 0.5, 0.50000006, 1.5]), f([0, 1, 1, 1])) == 2
    assert CM.compute(f([0.9, 0.1]), f([1, 0]))["twice_u"] == 2
    assert CM.compute(f([0.3, 0.3]), f([1, 0]))["twice_u"] == 1
    assert CM.compute(f([0.1, 0.9]), f([1, 0]))["twice_u"] == 0
    assert CM.flags_of(f([np.nan]), f([1])) == CM.F_NONFINITE and CM.flags_of(f([0.5]), f([0.5])) == CM.F_LABEL
    one = CM.compute(f([0.7, 0.2]), f([1, 1]))
    assert np.isnan(one["roc_auc"]) and one["n_correct"] == 1


# ------------------------------------------------------------------ exports and the C ABI
def test_header_library_and_binding_carry_the_metrics_abi(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define DQRM_METRICS_MAX_SAMPLES \(1ll << 30\)", code)
    tile = int(re.search(r"#define DQRM_METRICS_SORT_TILE\s+(\d+)", code).group(1))
    assert tile == L.DQRM_METRICS_SORT_TILE and L.DQRM_METRICS_MAX_SAMPLES == 1 << 30
    for name, val in (("LABEL", L.DQRM_METRICS_F_LABEL), ("NONFINITE", L.DQRM_METRICS_F_NONFINITE)):
        assert int(re.search(r"#define DQRM_METRICS_F_%s\s+(\d+)u" % name, code).group(1)) == val
    assert "typedef struct dqrm_metrics {" in code and "} dqrm_metrics_result;" in code
    names = ("dqrm_metrics_reset", "dqrm_metrics_update", "dqrm_metrics_workspace_bytes", "dqrm_metrics_finish",
             "dqrm_metrics_finish_launches")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.dqrm_abi_version() == 12
    # dqrm_metrics: i64 + 2 pointers; dqrm_metrics_result: 5 x u64 (the 40-byte read-back)
    assert C.sizeof(L.Metrics) == 24 and L.Metrics.keys.offset == 8 and L.Metrics.counters.offset == 16
    assert C.sizeof(L.MetricsResult) == 40
    assert [f[0] for f in L.MetricsResult._fields_] == ["n_pos", "n_neg", "n_correct", "twice_u", "flags"]
    assert any(s.endswith("dqrm_metrics.hip") for s in _build.SOURCES)
    unit = open(os.path.join(ROOT, "deep_quantized_recommendation_model_dqrm_amd", "csrc", "dqrm_metrics.hip")).read()
    assert "using dqrm_internal::set_error;" in unit and '#include "dqrm_internal.h"' in unit
    assert '#include "dqrm_device.h"' in unit
    assert not re.search(r"rocprim|hipcub|thrust", unit, flags=re.I)  # libdqrm's kernels are its own


def test_workspace_bytes_and_launch_count(lib):
    assert lib.dqrm_metrics_workspace_bytes(0) == 0 and b"seen must be" in lib.dqrm_last_error()
    assert lib.dqrm_metrics_workspace_bytes(-5) == 0
    assert lib.dqrm_metrics_workspace_bytes((1 << 30) + 1) == 0
    prev = 0
    for seen in (1, 2, 3, 4095, 8192, 8194, 1 << 20, (1 << 24) + 7, 1 << 30):
        b = lib.dqrm_metrics_workspace_bytes(seen)
        # the smaller class: at most seen // 2 keys, and one 256-bin histogram per tile of them
        tiles = max(1, -(-(seen // 2) // L.DQRM_METRICS_SORT_TILE))
        assert b >= 4 * (seen // 2) + 4 * 256 * tiles + 4 * 4 * 256 + 8 and b % 16 == 0
        assert b <= 4 * (seen // 2) + 4 * 256 * tiles + 4 * 4 * 256 + 64
        assert b >= prev
        prev = b
    assert lib.dqrm_metrics_finish_launches(0) == L.DQRM_E_INVALID
    assert lib.dqrm_metrics_finish_launches(-1) == L.DQRM_E_INVALID
    n = lib.dqrm_metrics_finish_launches(1)
    assert n > 0 and all(lib.dqrm_metrics_finish_launches(s) == n for s in (2, 4097, 1 << 24, 1 << 30))


def test_c_calls_reject_bad_arguments_without_device(lib):
    Z, T_, K, CN, OUT, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x10000
    m = L.Metrics()
    m.capacity, m.keys, m.counters = 100, K, CN
    ok = C.byref(m)
    need = lib.dqrm_metrics_workspace_bytes(100)
    INV, WSE = L.DQRM_E_INVALID, L.DQRM_E_WORKSPACE
    # a null struct
    assert lib.dqrm_metrics_reset(None, None) == INV and b"null dqrm_metrics" in lib.dqrm_last_error()
    assert lib.dqrm_metrics_update(None, Z, T_, 4, 0, None) == INV
    assert lib.dqrm_metrics_finish(None, 4, OUT, WS, need, None) == INV
    # a null member, a capacity outside 1..DQRM_METRICS_MAX_SAMPLES
    for field, value, msg in (("keys", None, b"null keys / counters"), ("counters", None, b"null keys / counters"),
                              ("capacity", 0, b"capacity must be"), ("capacity", -1, b"capacity must be"),
                              ("capacity", (1 << 30) + 1, b"capacity must be")):
        b = L.Metrics()
        b.capacity, b.keys, b.counters = 100, K, CN
        setattr(b, field, value)
        for call in (lambda: lib.dqrm_metrics_reset(C.byref(b), None),
                     lambda: lib.dqrm_metrics_update(C.byref(b), Z, T_, 4, 0, None),
                     lambda: lib.dqrm_metrics_finish(C.byref(b), 4, OUT, WS, need, None)):
            assert call() == INV, (field, value)
            assert msg in lib.dqrm_last_error(), (field, lib.dqrm_last_error())
    # update: null z / t, n < 1, seen_before + n > capacity
    assert lib.dqrm_metrics_update(ok, None, T_, 4, 0, None) == INV and b"null z / t" in lib.dqrm_last_error()
    assert lib.dqrm_metrics_update(ok, Z, None, 4, 0, None) == INV
    for n in (0, -1):
        assert lib.dqrm_metrics_update(ok, Z, T_, n, 0, None) == INV and b"n must be" in lib.dqrm_last_error()
    for n, before in ((101, 0), (1, 100), (51, 50), (1, -1), (1 << 62, 1 << 62)):
        assert lib.dqrm_metrics_update(ok, Z, T_, n, before, None) == INV, (n, before)
        assert b"exceeds capacity" in lib.dqrm_last_error()
    # finish: seen < 1 (and beyond the capacity), null out, the workspace
    for seen in (0, -7, 101):
        assert lib.dqrm_metrics_finish(ok, seen, OUT, WS, need, None) == INV and b"seen must be" in lib.dqrm_last_error()
    assert lib.dqrm_metrics_finish(ok, 100, None, WS, need, None) == INV and b"null out_dev" in lib.dqrm_last_error()
    assert lib.dqrm_metrics_finish(ok, 100, OUT, None, need, None) == WSE
    assert lib.dqrm_metrics_finish(ok, 100, OUT, WS + 8, need, None) == WSE
    assert lib.dqrm_metrics_finish(ok, 100, OUT, WS, need - 1, None) == WSE
    assert b"workspace" in lib.dqrm_last_error()
    assert lib.dqrm_metrics_finish(ok, 100, OUT, WS, 0, None) == WSE


# ------------------------------------------------------------------ Python arguments
def test_package_exports_and_signatures():
    assert dq.DLRMMetrics is metrics_mod.DLRMMetrics and "DLRMMetrics" in dq.__all__
    sig = inspect.signature(dq.DLRMMetrics.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("capacity", inspect.Parameter.empty), ("device", "cuda")]
    for name in ("reset", "update", "compute"):
        assert callable(getattr(dq.DLRMMetrics, name))
    esig = inspect.signature(dq.DQRMNet.evaluate)
    assert [(n, p.default) for n, p in list(esig.parameters.items())[1:]] == [
        ("batches", inspect.Parameter.empty), ("metrics", None), ("max_batches", -1)]


def test_metrics_constructor_errors():
    with pytest.raises(L.DQRMError, match="no CPU path"):
        dq.DLRMMetrics(16, device="cpu")
    for bad in (0, -3, (1 << 30) + 1):
        with pytest.raises(ValueError, match="capacity must be"):
            dq.DLRMMetrics(bad, device="cpu")


def _host_metrics(capacity=10, n=0):
    """A DLRMMetrics whose argument checks can run without a device."""
    m = object.__new__(dq.DLRMMetrics)
    m.capacity, m.n, m.device = capacity, n, torch.device("cuda", 0)
    return m


def test_update_argument_errors():
    m = _host_metrics()
    z, t = torch.rand(6, 1), torch.ones(6, 1)
    with pytest.raises(TypeError):
        m.update(z, [1.0] * 6)
    with pytest.raises(ValueError, match="float32"):
        m.update(z.double(), t)
    with pytest.raises(ValueError, match="float32"):
        m.update(z, t.long())
    with pytest.raises(ValueError, match="contiguous"):
        m.update(torch.rand(6, 2)[:, :1], t)
    with pytest.raises(ValueError, match=r"\[B, 1\] or \[B\]"):
        m.update(torch.rand(3, 2), torch.ones(3, 2))
    with pytest.raises(ValueError, match="elements"):
        m.update(z, torch.ones(5, 1))
    with pytest.raises(ValueError, match="at least one sample"):
        m.update(torch.rand(0), torch.ones(0))
    with pytest.raises(L.DQRMError, match="no CPU path"):
        m.update(z, t)
    with pytest.raises(L.DQRMError, match="no CPU path"):
        m.update(z.view(-1), t.view(-1))
    with pytest.raises(ValueError, match="no sample seen"):
        m.compute()
    with pytest.raises(ValueError, match="capacity 10 exceeded: 5 samples seen, 6 more"):
        _host_metrics(10, 5).update(z, t)  # before any call: it grows nothing


def test_evaluate_argument_errors():
    np.random.seed(0)
    model = dq.DQRMNet([5, 7], 8, [4, 8], [8 + 3, 1], device="cpu")
    with pytest.raises(TypeError, match="DLRMMetrics"):
        model.evaluate([], metrics="auc")
    with pytest.raises(ValueError, match=r"no len\(\)"):
        model.evaluate(iter([]))
    with pytest.raises(L.DQRMError, match="no CPU path"):
        model.evaluate([])
    with pytest.raises(L.DQRMError, match="no CPU path"):
        model.evaluate(iter([]), metrics=_host_metrics())
