"""CPU checks of the row-wise model forward's host side: the dqrm_rowwise_set exports in the header
and the binding, their argument validation (all of it before any device call: every descriptor
here sits on made-up addresses), the forward-only workspace query, the launch count, and
DQRMNet.quantize_embedding's errors on a model without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _build
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dqrm_rowwise_set_fwd", "dqrm_model_fwd_rowwise", "dqrm_model_fwd_rowwise_workspace_bytes",
         "dqrm_model_fwd_rowwise_workspace_layout", "dqrm_model_fwd_rowwise_launches")
FRESH = 1


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


def _stack(widths, per_channel, acts, base):
    n = len(widths) - 1
    lin = (L.Linear * n)()
    for i in range(n):
        l = lin[i]
        l.in_features, l.out_features, l.weight_bit, l.bias_bit = widths[i], widths[i + 1], 4, 4
        l.per_channel = per_channel[i]
        b = base * (i + 1)
        l.weight, l.bias, l.weight_integer, l.bias_integer, l.scale = (b + 0x1000 * j for j in range(1, 6))
    c = L.MLP()
    c.num_layers = n
    keep = (lin, (C.c_int32 * n)(*([1] * n)), (C.c_int32 * n)(*acts))
    c.layers, c.quantized, c.act = keep
    return c, keep


class Fake:
    """A valid (dqrm_model without tables, dqrm_rowwise_set, dqrm_batch) on made-up addresses: T = 3
    tables of dim 8, bottom [5, 16, 8], top [14, 16, 1], B = 33 Criteo-form bags."""

    def __init__(self, T=3, D=8, bits=4, B=33, qbits=0, bot_pc=(1, 1), top_pc=(1, 1), pooling_one=True):
        self.B = B
        self.bot, self._kb = _stack((5, 16, D), bot_pc, (1, 1), 0x10000)
        self.top, self._kt = _stack((D + (T + 1) * T // 2, 16, 1), top_pc, (1, 2), 0x200000)
        self.loss = L.Loss()
        self.loss.kind = L.DQRM_LOSS_BCE
        self.m = L.Model()
        self.m.bottom, self.m.top, self.m.loss = C.pointer(self.bot), C.pointer(self.top), C.pointer(self.loss)
        self.m.interact.num_features, self.m.interact.dim, self.m.interact.quant_bits = T + 1, D, qbits
        self.m.embedding_bit = 99  # ignored by the row-wise forward
        self.rs = L.RowwiseSet(T, D, bits, 0, 1307, 0x1000000, 0x1100000, 0x1200000)
        self.batch = L.Batch(0x3000000, 0x3100000, 0x3200000, B, B, L.DQRM_BATCH_POOLING_ONE if pooling_one else 0, 0)
        self.L = 4


def _calls(lib, f, flags=FRESH, model=True, rset=True, batch=True, x=0x5000000, labels=0x5100000, loss=0x5200000,
           ws=0x6000000, ws_bytes=1 << 40, B=None):
    m = C.byref(f.m) if model else None
    r = C.byref(f.rs) if rset else None
    b = C.byref(f.batch) if batch else None
    lay = L.ModelLayout()
    return {
        "fwd": lambda: lib.dqrm_model_fwd_rowwise(m, r, b, flags, x, labels, loss, None, ws, ws_bytes, None),
        "launches": lambda: lib.dqrm_model_fwd_rowwise_launches(m, r, b, flags, 1),
        "layout": lambda: lib.dqrm_model_fwd_rowwise_workspace_layout(m, r, f.B if B is None else B, C.byref(lay)),
        "bytes": lambda: lib.dqrm_model_fwd_rowwise_workspace_bytes(m, r, f.B if B is None else B),
    }


ALL = ("fwd", "launches", "layout", "bytes")
CALLS = ("fwd", "launches")


def _rejected(lib, calls, msg, which=ALL, code=L.DQRM_E_INVALID):
    for name in which:
        rc = calls[name]()
        if name == "bytes":
            assert rc == 0, name
        else:
            assert rc == code, (name, rc, lib.dqrm_last_error())
        assert msg in lib.dqrm_last_error(), (name, lib.dqrm_last_error())


def _set_fwd(lib, f, out=0x7000000, st=8, sb=24, psw=None, rset=True, batch=True):
    return lib.dqrm_rowwise_set_fwd(C.byref(f.rs) if rset else None, C.byref(f.batch) if batch else None, psw, out,
                                    st, sb, None)


# ------------------------------------------------------------------ header, binding, structs
def test_header_binding_and_struct(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12 and lib.dqrm_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert re.search(r"typedef\s+struct\s+dqrm_rowwise_set\s*\{", code)
    # 4 x i32 (num_tables, dim, bits, reserved), i64 total_rows, 3 pointers
    assert C.sizeof(L.RowwiseSet) == 16 + 8 + 3 * 8
    assert L.RowwiseSet.total_rows.offset == 16 and L.RowwiseSet.packed.offset == 24
    # the structs the issue pins keep their sizes
    assert C.sizeof(L.Model) == 4 * 8 + 32 + 16 and C.sizeof(L.ModelLayout) == 7 * C.sizeof(C.c_size_t)
    assert C.sizeof(L.Batch) == 48
    assert "RowwiseTableSet" in dq.__all__ and dq.RowwiseTableSet is dq.rowwise.RowwiseTableSet
    assert any(s.endswith("dqrm_rowwise.hip") for s in _build.SOURCES)


# ------------------------------------------------------------------ the valid call, on the host
def test_valid_queries(lib):
    f = Fake()
    c = _calls(lib, f)
    # tables is NULL: the row-wise forward never reads it
    assert not f.m.tables
    assert c["launches"]() == f.L + 3  # emb + L layers + interact + loss
    assert lib.dqrm_model_fwd_rowwise_launches(C.byref(f.m), C.byref(f.rs), C.byref(f.batch), FRESH, 0) == f.L + 2
    need = c["bytes"]()
    al = lambda n: (n + 255) & ~255
    B, T, D = 33, 3, 8
    want = (al(4 * B * T * D) + al(4 * B * 16) + al(4 * B * 8) + al(4 * B * 14) + al(4 * B * 16) + al(4 * B)
            + al(4) + al(0))
    assert need == want
    lay = L.ModelLayout()
    assert lib.dqrm_model_fwd_rowwise_workspace_layout(C.byref(f.m), C.byref(f.rs), B, C.byref(lay)) == 0
    assert lay.slab == 0 and lay.total == need and lay.dr == lay.dx == lay.demb == 0
    assert lay.r == al(4 * B * T * D) + al(4 * B * 16) + al(4 * B * 8)
    assert lay.p == lay.r + al(4 * B * 14) + al(4 * B * 16)
    # grows with B
    assert lib.dqrm_model_fwd_rowwise_workspace_bytes(C.byref(f.m), C.byref(f.rs), 34) >= need


def test_launch_count_additions(lib):
    f = Fake(qbits=16)
    assert _calls(lib, f)["launches"]() == f.L + 4          # + the interaction's scale
    f = Fake()
    assert _calls(lib, f, flags=0)["launches"]() == f.L + 3 + 4   # + 1 per per-channel layer, not fresh
    f = Fake(bot_pc=(0, 1), top_pc=(1, 0))
    assert _calls(lib, f, flags=0)["launches"]() == f.L + 3 + 2 + 2 * 2  # + 2 per per-tensor layer
    assert _calls(lib, f, flags=FRESH)["launches"]() == f.L + 3


# ------------------------------------------------------------------ validation
def test_null_arguments_rejected(lib):
    f = Fake()
    _rejected(lib, _calls(lib, f, model=False), b"null model")
    _rejected(lib, _calls(lib, f, rset=False), b"null row-wise set")
    _rejected(lib, _calls(lib, f, batch=False), b"null batch", which=CALLS)
    for field in ("bottom", "top", "loss"):
        f = Fake()
        setattr(f.m, field, None)
        _rejected(lib, _calls(lib, f), b"null bottom / top / loss")
    for field in ("packed", "meta", "err"):
        f = Fake()
        setattr(f.rs, field, None)
        _rejected(lib, _calls(lib, f), b"null packed / meta / err")
        assert _set_fwd(lib, f) == L.DQRM_E_INVALID and b"null packed / meta / err" in lib.dqrm_last_error()
    f = Fake()
    assert lib.dqrm_model_fwd_rowwise_workspace_layout(C.byref(f.m), C.byref(f.rs), 33, None) == L.DQRM_E_INVALID
    assert b"null out" in lib.dqrm_last_error()
    _rejected(lib, _calls(lib, f, x=None), b"null x", which=("fwd",))
    _rejected(lib, _calls(lib, f, loss=None), b"labels need a loss", which=("fwd",))
    f = Fake()
    f.batch.idx = None
    _rejected(lib, _calls(lib, f), b"null batch idx", which=CALLS)
    f = Fake(pooling_one=False)
    f.batch.off = None
    _rejected(lib, _calls(lib, f), b"needs off and idx_base", which=CALLS)
    f = Fake()  # the Criteo form reads neither
    f.batch.off = f.batch.idx_base = None
    assert _calls(lib, f)["launches"]() == f.L + 3


def test_set_rules_rejected(lib):
    for bits in (0, 2, 5, 16):
        f = Fake(bits=bits)
        _rejected(lib, _calls(lib, f), b"bits must be 4 or 8")
        assert _set_fwd(lib, f) == L.DQRM_E_INVALID and b"bits must be 4 or 8" in lib.dqrm_last_error()
    for D in (4, 12, 24, 512):
        f = Fake()
        f.rs.dim = D
        _rejected(lib, _calls(lib, f), b"unsupported")
    f = Fake()
    f.rs.num_tables = 0
    _rejected(lib, _calls(lib, f), b"num_tables out of range")
    f = Fake()
    f.rs.total_rows = 0
    _rejected(lib, _calls(lib, f), b"total_rows")
    f = Fake()
    f.rs.packed = 0x1000002
    _rejected(lib, _calls(lib, f), b"packed must be 4-byte aligned")
    # the set against the model
    f = Fake()
    f.rs.dim = 16
    _rejected(lib, _calls(lib, f), b"num_features = tables + 1")
    f = Fake()
    f.rs.num_tables = 4
    _rejected(lib, _calls(lib, f), b"num_features = tables + 1")


def test_set_fwd_out_rules(lib):
    f = Fake()
    for kw in (dict(out=None), dict(out=0x7000008), dict(st=6), dict(sb=26)):
        assert _set_fwd(lib, f, **kw) == L.DQRM_E_INVALID, kw
        assert b"16-B aligned" in lib.dqrm_last_error()
    assert _set_fwd(lib, f, rset=False) == L.DQRM_E_INVALID and b"null row-wise set" in lib.dqrm_last_error()
    assert _set_fwd(lib, f, batch=False) == L.DQRM_E_INVALID and b"null batch" in lib.dqrm_last_error()
    f.batch.num_bags = -1
    assert _set_fwd(lib, f) == L.DQRM_E_INVALID and b"negative num_bags" in lib.dqrm_last_error()
    f.batch.num_bags = 0  # nothing to do, nothing launched
    assert _set_fwd(lib, f) == L.DQRM_OK


def test_stage_and_call_rules_rejected(lib):
    f = Fake()
    f._kb[0][1].in_features = 15
    _rejected(lib, _calls(lib, f), b"does not match")
    f = Fake()
    f._kt[2][1] = 3
    _rejected(lib, _calls(lib, f), b"act must be")
    f = Fake()
    f._kb[0][1].out_features = 16
    f._kt[0][0].in_features = 14
    _rejected(lib, _calls(lib, f), b"the bottom stack returns 16 features")
    f = Fake()
    f._kt[0][0].in_features = 15
    _rejected(lib, _calls(lib, f), b"the top stack takes 15 features")
    f = Fake()
    f.m.interact.quant_bits = 17
    _rejected(lib, _calls(lib, f), b"quant_bits must be 0 or 2..16")
    f = Fake()
    f.loss.kind = 3
    _rejected(lib, _calls(lib, f), b"unknown loss kind 3")
    # flags: DQRM_MODEL_MLP_FRESH only
    for flags in (2, 4, 8, 16):
        _rejected(lib, _calls(lib, Fake(), flags=flags), b"unknown flags", which=CALLS)
    # B: the loss's range
    for B in (0, (1 << 20) + 1):
        f = Fake(B=B)
        _rejected(lib, _calls(lib, f), b"B must be 1..")


def test_workspace_rejected(lib):
    f = Fake()
    need = _calls(lib, f)["bytes"]()
    for kw in (dict(ws=None), dict(ws=0x6000008), dict(ws_bytes=need - 1)):
        _rejected(lib, _calls(lib, f, **kw), b"workspace needs", which=("fwd",), code=L.DQRM_E_WORKSPACE)


def test_bytes_zero_on_bad_arguments(lib):
    f = Fake()
    assert lib.dqrm_model_fwd_rowwise_workspace_bytes(None, C.byref(f.rs), 33) == 0
    assert lib.dqrm_model_fwd_rowwise_workspace_bytes(C.byref(f.m), None, 33) == 0
    assert lib.dqrm_model_fwd_rowwise_workspace_bytes(C.byref(f.m), C.byref(f.rs), 0) == 0
    f.rs.bits = 5
    assert lib.dqrm_model_fwd_rowwise_workspace_bytes(C.byref(f.m), C.byref(f.rs), 33) == 0


# ------------------------------------------------------------------ DQRMNet without a GPU
def _cpu_model():
    return dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 1], device="cpu")


def test_cpu_model_quantize_embedding_raises():
    m = _cpu_model()
    assert m.quantize_emb is False and m.quantize_bits is None and m.emb_q is None
    with pytest.raises(L.DQRMError, match="no CPU path"):
        m.quantize_embedding(4)
    with pytest.raises(L.DQRMError, match="no CPU path"):
        m.quantize_embedding(8, keep_fp32=False)
    assert m.emb_q is None and "emb_weight" in m.state_dict()
    m.dequantize_embedding()  # nothing to drop


@pytest.mark.parametrize("bits", [5, 0, 16, 32, None, True, 4.5])
def test_quantize_embedding_bad_bits(bits):
    with pytest.raises(ValueError, match="bits must be 4 or 8"):
        _cpu_model().quantize_embedding(bits)


def test_rowwise_table_set_argument_errors():
    with pytest.raises(ValueError, match="bits must be 4 or 8"):
        dq.RowwiseTableSet.from_weights([torch.zeros(3, 8)], 5)
    with pytest.raises(ValueError, match="one D"):
        dq.RowwiseTableSet.from_weights([torch.zeros(3, 8), torch.zeros(3, 16)], 4)
