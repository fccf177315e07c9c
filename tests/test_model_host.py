"""CPU checks of DQRMNet's host side: the dqrm_model exports in the header and the binding, their
argument validation (all of it before any device call: every descriptor here sits on made-up
addresses), the workspace query, the launch count, dqrm_mlp_sgd_multi's layer total, and DQRMNet's
construction errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _build
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dqrm_mlp_sgd_multi_workspace_bytes", "dqrm_mlp_sgd_multi", "dqrm_model_workspace_bytes",
         "dqrm_model_workspace_layout", "dqrm_model_fwd", "dqrm_model_step", "dqrm_model_step_launches")
FRESH, REQUANT, NO_UPDATE, EMB_READY = 1, 2, 4, 8


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


class FakeStack:
    """A valid dqrm_mlp over made-up device addresses (tests/test_mlpstack_host.py's)."""

    def __init__(self, widths, per_channel=None, quantized=None, acts=None, base=0x10000):
        n = len(widths) - 1
        per_channel = [1] * n if per_channel is None else per_channel
        quantized = [1] * n if quantized is None else quantized
        acts = [1] * n if acts is None else acts
        self.lin = (L.Linear * n)()
        for i in range(n):
            l = self.lin[i]
            l.in_features, l.out_features, l.weight_bit, l.bias_bit = widths[i], widths[i + 1], 4, 4
            l.per_channel = per_channel[i]
            b = base * (i + 1)
            l.weight, l.bias, l.weight_integer, l.bias_integer, l.scale = (b + 0x1000 * j for j in range(1, 6))
        self.quantized = (C.c_int32 * n)(*quantized)
        self.act = (C.c_int32 * n)(*acts)
        self.c = L.MLP()
        self.c.num_layers = n
        self.c.layers, self.c.quantized, self.c.act = self.lin, self.quantized, self.act
        self.n = n


class FakeModel:
    """A valid dqrm_model on made-up addresses: T = 3 tables of dim 8, bottom [5, 16, 8],
    top [14, 16, 1] (F = 4 vectors, 6 pairs), a batch of B = 33 Criteo-form bags."""

    def __init__(self, T=3, D=8, bot=(5, 16, 8), top=(14, 16, 1), B=33, itself=0, qbits=0, bot_pc=None, top_pc=None,
                 pooling_one=True, max_lookups=None):
        self.T, self.D, self.B = T, D, B
        self.ts = L.TableSet()
        self.ts.num_tables, self.ts.dim, self.ts.total_rows, self.ts.total_blocks, self.ts.total_sblocks = T, D, 1307, 7, 3
        for k, (name, _) in enumerate(L.TableSet._fields_[5:19]):
            setattr(self.ts, name, 0x1000000 + 0x10000 * k)
        self.rows = (C.c_int64 * T)(*([7, 300, 1000] + [10] * T)[:T])
        self.ts.num_rows_host = C.addressof(self.rows)
        self.bot = FakeStack(bot, per_channel=bot_pc, base=0x10000)
        self.top = FakeStack(top, per_channel=top_pc, acts=[1] * (len(top) - 2) + [2], base=0x200000)
        self.loss = L.Loss()
        self.loss.kind = L.DQRM_LOSS_BCE
        self.m = L.Model()
        self.m.tables, self.m.bottom, self.m.top = C.pointer(self.ts), C.pointer(self.bot.c), C.pointer(self.top.c)
        self.m.loss = C.pointer(self.loss)
        self.m.interact.num_features, self.m.interact.dim = T + 1, D
        self.m.interact.self_interaction, self.m.interact.quant_bits = itself, qbits
        self.m.embedding_bit, self.m.emb_fwd_flags, self.m.ste, self.m.repack_bits = 4, L.DQRM_FWD_REFRESH_SCALE, 1, 0
        self.batch = self.make_batch(B, pooling_one, max_lookups)
        self.L = self.bot.n + self.top.n

    @staticmethod
    def make_batch(B, pooling_one=True, max_lookups=None):
        return L.Batch(0x3000000, 0x3100000, 0x3200000, B, B if max_lookups is None else max_lookups,
                       L.DQRM_BATCH_POOLING_ONE if pooling_one else 0, 0)

    def ptrs(self, first=0x4000000):
        return (C.c_void_p * self.L)(*[first + 0x1000 * i for i in range(self.L)])


def _calls(lib, f, flags=0, batch="own", nxt=None, x=0x5000000, labels=0x5100000, loss=0x5200000, g=0x5300000,
           dw="own", db="own", ws=0x6000000, ws_bytes=1 << 40, model=True):
    """The four calls on the model, with valid (made-up) arguments unless overridden."""
    m = C.byref(f.m) if model else None
    b = C.byref(f.batch) if batch == "own" else batch
    n = None if nxt is None else C.byref(nxt)
    dw = f.ptrs(0x4000000) if dw == "own" else dw
    db = f.ptrs(0x4100000) if db == "own" else db
    fwd_flags = flags & ~(REQUANT | NO_UPDATE)  # the update's flags are the step's alone
    return {
        "fwd": lambda: lib.dqrm_model_fwd(m, b, fwd_flags, x, labels, loss, None, ws, ws_bytes, None),
        "step": lambda: lib.dqrm_model_step(m, b, n, flags, x, labels, 0.1, loss, None, g, dw, db, ws, ws_bytes, None),
        "launches": lambda: lib.dqrm_model_step_launches(m, b, n, flags),
        "bytes": lambda: lib.dqrm_model_workspace_bytes(m, f.B, f.B),
    }


def _rejected(lib, calls, msg, which=("fwd", "step", "launches", "bytes"), code=L.DQRM_E_INVALID):
    for name in which:
        rc = calls[name]()
        if name == "bytes":
            assert rc == 0, name
        else:
            assert rc == code, (name, rc, lib.dqrm_last_error())
        assert msg in lib.dqrm_last_error(), (name, lib.dqrm_last_error())


NOT_BYTES = ("fwd", "step", "launches")


# ------------------------------------------------------------------ header, binding, structs
def test_header_binding_and_structs(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12 and lib.dqrm_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    for name, val in (("MLP_FRESH", 1), ("REQUANT", 2), ("NO_UPDATE", 4), ("EMB_READY", 8)):
        assert int(re.search(r"^#define\s+DQRM_MODEL_%s\s+(\d+)u" % name, src, flags=re.M).group(1)) == val
        assert getattr(L, "DQRM_MODEL_" + name) == val
    # dqrm_model: 4 pointers, dqrm_interact (4 x i32 + 2 x i64), 4 x 32 bits; the layout: 7 x size_t
    assert C.sizeof(L.Interact) == 32
    assert C.sizeof(L.Model) == 4 * 8 + 32 + 16
    assert C.sizeof(L.ModelLayout) == 7 * C.sizeof(C.c_size_t)
    assert "DQRMNet" in dq.__all__ and dq.DQRMNet is dq.model.DQRMNet
    assert any(s.endswith("dqrm_model.hip") for s in _build.SOURCES)


# ------------------------------------------------------------------ validation
def test_null_model_and_members_rejected(lib):
    f = FakeModel()
    _rejected(lib, _calls(lib, f, model=False), b"null model")
    for field in ("tables", "bottom", "top", "loss"):
        f = FakeModel()
        setattr(f.m, field, None)
        _rejected(lib, _calls(lib, f), b"null tables / bottom / top / loss")
    f = FakeModel()
    assert lib.dqrm_model_workspace_layout(C.byref(f.m), 33, 33, None) == L.DQRM_E_INVALID
    assert b"null out" in lib.dqrm_last_error()


def test_what_each_stage_rejects(lib):
    # the tables
    f = FakeModel()
    f.ts.W = None
    _rejected(lib, _calls(lib, f), b"null state pointer")
    f = FakeModel()
    f.ts.W = 0x1000008
    _rejected(lib, _calls(lib, f), b"16-byte aligned")
    f = FakeModel()
    f.m.embedding_bit = 17
    _rejected(lib, _calls(lib, f), b"embedding_bit 17 unsupported")
    f = FakeModel()
    f.m.emb_fwd_flags |= L.DQRM_FWD_USE_PACKED
    f.ts.packed = None
    _rejected(lib, _calls(lib, f), b"packed path needs packed rows")
    f = FakeModel()
    f.m.repack_bits = 8
    _rejected(lib, _calls(lib, f), b"repack needs packed rows")
    f = FakeModel()
    f.batch.idx = None
    _rejected(lib, _calls(lib, f), b"null batch pointer", which=NOT_BYTES)
    f = FakeModel(max_lookups=1 << 30)
    _rejected(lib, _calls(lib, f), b"max_lookups", which=("step", "launches"), code=L.DQRM_E_CAPACITY)
    # the stacks
    f = FakeModel()
    f.bot.lin[1].in_features = 15
    _rejected(lib, _calls(lib, f), b"does not match")
    f = FakeModel()
    f.top.lin[0].weight_bit = 1
    _rejected(lib, _calls(lib, f), b"layer 0: weight_bit")
    f = FakeModel()
    f.top.act[1] = 3
    _rejected(lib, _calls(lib, f), b"act must be")
    f = FakeModel()
    f.bot.lin[0].scale = None
    _rejected(lib, _calls(lib, f), b"null weight_integer / bias_integer / scale")
    # the interaction
    f = FakeModel()
    f.m.interact.quant_bits = 17
    _rejected(lib, _calls(lib, f), b"quant_bits must be 0 or 2..16")
    f = FakeModel()
    f.m.interact.num_features = 5
    _rejected(lib, _calls(lib, f), b"num_features = tables + 1")
    f = FakeModel()
    f.m.interact.dim = 16
    _rejected(lib, _calls(lib, f), b"num_features = tables + 1")
    # the loss
    f = FakeModel()
    f.loss.kind = 3
    _rejected(lib, _calls(lib, f), b"unknown loss kind 3")
    f = FakeModel()
    f.loss.kind = L.DQRM_LOSS_WBCE
    _rejected(lib, _calls(lib, f), b"DQRM_LOSS_WBCE needs weights")


def test_widths_between_the_stages_rejected(lib):
    f = FakeModel(bot=(5, 16, 4))
    _rejected(lib, _calls(lib, f), b"the bottom stack returns 4 features, the tables' dim is 8")
    f = FakeModel(top=(15, 16, 1))
    _rejected(lib, _calls(lib, f), b"the top stack takes 15 features, the interaction returns 14")
    f = FakeModel(top=(14, 16, 1), itself=1)  # with the diagonal: 8 + 6 + 4
    _rejected(lib, _calls(lib, f), b"the interaction returns 18")
    assert _calls(lib, FakeModel(top=(18, 16, 1), itself=1))["launches"]() > 0
    f = FakeModel(top=(14, 16, 2))
    _rejected(lib, _calls(lib, f), b"the top stack must return 1 feature (got 2)")
    f = FakeModel(bot=[5] + [8] * 9, top=[14] + [8] * 7 + [1])  # 9 + 8 layers
    _rejected(lib, _calls(lib, f), b"17 layers in all")
    ok = FakeModel(bot=[5] + [8] * 9, top=[14] + [8] * 6 + [1])  # 9 + 7: accepted
    assert _calls(lib, ok, flags=FRESH | REQUANT)["launches"]() == 3 * 16 + 5
    _rejected(lib, _calls(lib, ok, ws_bytes=16), b"workspace needs", which=("fwd", "step"), code=L.DQRM_E_WORKSPACE)


def test_batch_size_flags_tensors_next_and_workspace_rejected(lib):
    f = FakeModel()
    for B in (0, -1, (1 << 20) + 1):
        b = FakeModel.make_batch(B)
        _rejected(lib, _calls(lib, f, batch=C.byref(b)), b"B must be 1..1048576", which=NOT_BYTES)
        assert lib.dqrm_model_workspace_bytes(C.byref(f.m), B, 33) == 0
        assert b"B must be 1..1048576" in lib.dqrm_last_error()
    assert lib.dqrm_model_workspace_bytes(C.byref(f.m), 1 << 20, 1 << 20) > 0
    assert lib.dqrm_model_workspace_bytes(C.byref(f.m), 33, -1) == 0
    _rejected(lib, _calls(lib, f, batch=None), b"null batch", which=NOT_BYTES)
    _rejected(lib, _calls(lib, f, flags=16), b"unknown flags 0x10", which=NOT_BYTES)
    assert lib.dqrm_model_fwd(C.byref(f.m), C.byref(f.batch), REQUANT, 0x5000000, None, None, None, 0x6000000, 1 << 40,
                              None) == L.DQRM_E_INVALID  # an update flag on the inference call
    assert b"unknown flags 0x2" in lib.dqrm_last_error()
    _rejected(lib, _calls(lib, f, x=None), b"null x", which=("fwd", "step"))
    for kw in ({"labels": None}, {"loss": None}, {"g": None}):
        _rejected(lib, _calls(lib, f, **kw), b"null x / labels / loss / g", which=("step",))
    _rejected(lib, _calls(lib, f, loss=None), b"null loss", which=("fwd",))
    null = C.cast(None, C.POINTER(C.c_void_p))
    _rejected(lib, _calls(lib, f, dw=null), b"null dw / db array", which=("step",))
    _rejected(lib, _calls(lib, f, db=null), b"null dw / db array", which=("step",))
    hole = f.ptrs()
    hole[3] = None
    _rejected(lib, _calls(lib, f, dw=hole), b"null dw[3] / db[3]", which=("step",))
    _rejected(lib, _calls(lib, f, db=hole), b"null dw[3] / db[3]", which=("step",))
    # the next batch
    other = FakeModel.make_batch(34)
    _rejected(lib, _calls(lib, f, nxt=other), b"next has 34 bags, the slab holds 33", which=("step", "launches"))
    same = FakeModel.make_batch(33)
    _rejected(lib, _calls(lib, f, nxt=same, flags=NO_UPDATE), b"a next batch needs the update", which=("step", "launches"))
    bad = FakeModel.make_batch(33)
    bad.off = None
    _rejected(lib, _calls(lib, f, nxt=bad), b"null batch pointer", which=("step", "launches"))
    # the workspace
    need = lib.dqrm_model_workspace_bytes(C.byref(f.m), 33, 33)
    for kw in ({"ws_bytes": need - 1}, {"ws": None}, {"ws": 0x6000008}):
        _rejected(lib, _calls(lib, f, **kw), b"workspace needs %d bytes" % need, which=("fwd", "step"),
                  code=L.DQRM_E_WORKSPACE)


def test_mlp_sgd_multi_validation(lib):
    MS = C.POINTER(L.MLP) * 2

    def call(a, b, flags=1, dw=None, db=None, gs=None, ws=0x800000, ws_bytes=1 << 20, n=2):
        L_ = a.n + b.n
        arr = lambda first: (C.c_void_p * L_)(*[first + 0x1000 * i for i in range(L_)])  # noqa: E731
        return lib.dqrm_mlp_sgd_multi(MS(C.pointer(a.c), C.pointer(b.c)), n, flags, arr(0xA00000) if dw is None else dw,
                                      arr(0xB00000) if db is None else db, gs, 0.1, ws, ws_bytes, None)

    a, b = FakeStack([5] + [8] * 9), FakeStack([14] + [8] * 8)  # 9 + 8 = 17 layers
    assert call(a, b) == L.DQRM_E_INVALID and b"17 layers in all" in lib.dqrm_last_error()
    assert lib.dqrm_mlp_sgd_multi_workspace_bytes(MS(C.pointer(a.c), C.pointer(b.c)), 2) == 0
    # 9 + 7 = 16 pass the total: the call gets as far as the next bad argument
    a, b = FakeStack([5] + [8] * 9), FakeStack([14] + [8] * 7)
    hole = (C.c_void_p * 16)(*[0xA00000 + 0x1000 * i for i in range(16)])
    hole[15] = None
    assert call(a, b, dw=hole) == L.DQRM_E_INVALID and b"null dw[15]" in lib.dqrm_last_error()
    assert call(a, b, db=hole) == L.DQRM_E_INVALID and b"null db[15]" in lib.dqrm_last_error()
    assert call(a, b, gs=hole) == L.DQRM_E_INVALID and b"null gscale[15]" in lib.dqrm_last_error()
    assert call(a, b, flags=2) == L.DQRM_E_INVALID and b"unknown flags" in lib.dqrm_last_error()
    assert call(a, b, n=0) == L.DQRM_E_INVALID and b"num_stacks" in lib.dqrm_last_error()
    assert lib.dqrm_mlp_sgd_multi(None, 2, 1, hole, hole, None, 0.1, None, 0, None) == L.DQRM_E_INVALID
    assert b"null stacks array" in lib.dqrm_last_error()
    # each stack's own width chain
    a, b = FakeStack((5, 16, 8)), FakeStack((14, 16, 1))
    b.lin[1].in_features = 15
    assert call(a, b) == L.DQRM_E_INVALID and b"does not match" in lib.dqrm_last_error()
    # the second stack need not continue the first (8 -> 14 is no chain); a per-tensor layer in
    # either asks for the row maxima of both
    a, b = FakeStack((5, 16, 8)), FakeStack((14, 16, 1), per_channel=(1, 0))
    stacks = MS(C.pointer(a.c), C.pointer(b.c))
    need = lib.dqrm_mlp_sgd_multi_workspace_bytes(stacks, 2)
    assert need == (16 + 8 + 16 + 1) * 4
    assert call(a, b, ws_bytes=need - 1) == L.DQRM_E_INVALID and b"workspace" in lib.dqrm_last_error()
    assert call(a, b, ws=None) == L.DQRM_E_INVALID and b"workspace" in lib.dqrm_last_error()
    b = FakeStack((14, 16, 1))
    assert lib.dqrm_mlp_sgd_multi_workspace_bytes(MS(C.pointer(a.c), C.pointer(b.c)), 2) == 0


# ------------------------------------------------------------------ the workspace query
def test_workspace_bytes_monotone_and_covers_its_parts(lib):
    f = FakeModel(qbits=16, top_pc=(1, 0), pooling_one=False)
    prev = 0
    for B in (1, 2, 33, 128, 129, 2048, 5000):
        n = lib.dqrm_model_workspace_bytes(C.byref(f.m), B, B)
        assert n >= prev and n % 16 == 0
        prev = n
    T, D, R = 3, 8, 14
    for B, ml in ((33, 33), (33, 500), (5000, 20000)):
        n = lib.dqrm_model_workspace_bytes(C.byref(f.m), B, ml)
        assert n >= lib.dqrm_model_workspace_bytes(C.byref(f.m), B, 33 if ml > 33 else 1)
        outputs = B * 4 * (16 + 8 + 16 + 1)
        parts = (2 * B * T * D * 4 + 2 * B * R * 4 + B * D * 4 + outputs
                 + max(lib.dqrm_mlp_bwd_scratch_bytes(C.byref(f.bot.c), B), lib.dqrm_mlp_bwd_scratch_bytes(C.byref(f.top.c), B))
                 + lib.dqrm_bwd_workspace_bytes(T, ml) + 4 + (16 + 8 + 16 + 1) * 4)
        assert n >= parts, (B, ml, n, parts)
        lay = L.ModelLayout()
        assert lib.dqrm_model_workspace_layout(C.byref(f.m), B, ml, C.byref(lay)) == 0
        assert lay.total == n and lay.slab == 0
        offs = [lay.slab, lay.r, lay.p, lay.dr, lay.dx, lay.demb]
        assert offs == sorted(offs) and len(set(offs)) == 6 and all(o % 16 == 0 for o in offs)
        assert lay.r - lay.slab >= B * T * D * 4 and lay.dx - lay.dr >= B * R * 4 and lay.demb - lay.dx >= B * D * 4
        assert n - lay.demb >= B * T * D * 4


# ------------------------------------------------------------------ the launch count
def test_step_launches_formula_and_corrections(lib):
    f = FakeModel()
    Lr = f.L  # 4 layers
    base = 3 * Lr + 5
    count = lambda f, flags, nxt=None: _calls(lib, f, flags=flags, nxt=nxt)["launches"]()  # noqa: E731
    assert count(f, FRESH | REQUANT) == base
    assert count(f, FRESH) == base                       # an update without requantization
    assert count(f, FRESH | REQUANT | EMB_READY) == base - 1
    assert count(f, FRESH | NO_UPDATE) == base - 2       # no embedding update, no MLP update
    assert count(f, REQUANT) == base + Lr                # not fresh, per channel: one wquant per layer
    kaggle = FakeModel(T=26, D=16, bot=(13, 512, 256, 64, 16), top=(367, 512, 256, 1), B=128)
    assert count(kaggle, FRESH | REQUANT) == 26
    # per-tensor layers: two wquant launches each when not fresh, one more update launch with REQUANT
    pt = FakeModel(bot_pc=(1, 0), top_pc=(0, 1))
    assert count(pt, FRESH) == base
    assert count(pt, FRESH | REQUANT) == base + 1
    assert count(pt, REQUANT) == base + 1 + 2 * 2 + 2 * 1
    assert count(pt, NO_UPDATE) == base - 2 + 2 * 2 + 2 * 1
    # a full-precision layer has nothing to quantize
    fp = FakeModel()
    fp.top.quantized[0] = 0
    assert count(fp, REQUANT) == base + Lr - 1
    # the quantized interaction's scale
    q = FakeModel(qbits=16)
    assert count(q, FRESH | REQUANT) == base + 1
    # the next batch's forward: inside the update's launch for a small Criteo-form pair (where
    # dqrm_bwd_sgd_fwd_is_one_launch says so: it asks the device for the kernel's LDS use, and
    # without a device answers 0), a launch of its own otherwise (multi-lookup bags; a batch past
    # the small kernel's 512 lookups)
    nxt = FakeModel.make_batch(33)
    one = lib.dqrm_bwd_sgd_fwd_is_one_launch(C.byref(f.ts), C.byref(f.batch), C.byref(nxt), f.m.emb_fwd_flags)
    assert one in (0, 1)
    assert count(f, FRESH | REQUANT, nxt) == base + 1 - one
    assert count(f, FRESH | REQUANT | EMB_READY, nxt) == base - one
    bags = FakeModel.make_batch(33, pooling_one=False, max_lookups=90)
    assert lib.dqrm_bwd_sgd_fwd_is_one_launch(C.byref(f.ts), C.byref(f.batch), C.byref(bags), f.m.emb_fwd_flags) == 0
    assert count(f, FRESH | REQUANT, bags) == base + 1
    big = FakeModel(B=2048)
    nxt = FakeModel.make_batch(2048)
    assert lib.dqrm_bwd_sgd_fwd_is_one_launch(C.byref(big.ts), C.byref(big.batch), C.byref(nxt), big.m.emb_fwd_flags) == 0
    assert count(big, FRESH | REQUANT) == base
    assert count(big, FRESH | REQUANT, nxt) == base + 1


# ------------------------------------------------------------------ DQRMNet's own errors
def test_dqrmnet_construction_errors():
    np.random.seed(0)
    with pytest.raises(ValueError, match=r"ln_bot\[-1\] = 4 does not match m_spa = 8"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 4], [14, 16, 1], device="cpu")
    with pytest.raises(ValueError, match=r"ln_top\[0\] = 15 does not match the interaction's 14"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [15, 16, 1], device="cpu")
    with pytest.raises(ValueError, match=r"ln_top\[0\] = 14 does not match the interaction's 18"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 1], arch_interaction_itself=True, device="cpu")
    with pytest.raises(ValueError, match=r"ln_top\[-1\] must be 1"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 2], device="cpu")
    with pytest.raises(NotImplementedError, match="quantize_activation"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 1], quantize_activation=True, device="cpu")
    with pytest.raises(ValueError, match="wbce"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 1], loss_function="wbce", device="cpu")
    with pytest.raises(ValueError, match="16"):
        dq.DQRMNet([7], 8, [5] + [8] * 9, [9] + [8] * 7 + [1], device="cpu")


def test_dqrmnet_description_and_cpu_calls_raise_dqrm_error():
    np.random.seed(0)
    m = dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 1], device="cpu")
    keys = list(m.state_dict().keys())
    assert keys[0] == "emb_weight" and "bot_l.0.weight" in keys and "bot_l.2.bias" in keys and "top_l.2.weight" in keys
    assert tuple(m.emb_weight.shape) == (1307, 8)
    assert [l.activation for l in m.top_stack.layers] == ["relu", "sigmoid"]
    assert [l.activation for l in m.bot_stack.layers] == ["relu", "relu"]
    # the draw order is the reference's: tables, bottom, top
    np.random.seed(0)
    w0 = np.random.uniform(low=-np.sqrt(1 / 7), high=np.sqrt(1 / 7), size=(7, 8)).astype(np.float32)
    np.testing.assert_array_equal(m.emb_weight[:7].numpy(), w0)
    x, t = torch.zeros(33, 5), torch.zeros(33)
    for call in (lambda: m.train_step(x, None, t, 0.1), lambda: m.predict(x, None), lambda: m(x, None),
                 lambda: m.requantize(), lambda: m.step_launches(None)):
        with pytest.raises(L.DQRMError, match="no CPU path"):
            call()
