"""CPU checks of the quantize_activation calls' host side: dqrm_mlp_qact_prepare / _fwd_qact /
_bwd_qact and the dqrm_model_*_qact exports in the header and the binding, their argument
validation (all of it before any device call: every descriptor sits on made-up addresses), the
workspace query, the launch count, and the Python layers' construction errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L
from test_model_host import FakeModel, FakeStack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dqrm_mlp_qact_prepare", "dqrm_mlp_fwd_qact", "dqrm_mlp_bwd_qact", "dqrm_model_fwd_qact",
         "dqrm_model_step_qact", "dqrm_model_qact_workspace_bytes", "dqrm_model_qact_workspace_layout",
         "dqrm_model_qact_step_launches")
FRESH, REQUANT, NO_UPDATE, EMB_READY = 1, 2, 4, 8
PREV = 0xC00000
NULLPP = C.cast(None, C.POINTER(C.c_void_p))


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


def tensor_stack(widths=(6, 4, 3), per_channel=None, **kw):
    n = len(widths) - 1
    return FakeStack(widths, per_channel=[0] * n if per_channel is None else per_channel, **kw)


def arr(n, first):
    return (C.c_void_p * n)(*[first + 0x1000 * i for i in range(n)])


def stack_calls(lib, s, B=5, x=0x500000, dy=0x600000, prev=PREV, out_scale="own", y="own", dw="own", db="own",
                scratch=0x700000, scratch_bytes=1 << 20, flags=1, stack=True):
    """The three stack exports with valid (made-up) arguments unless overridden."""
    os_ = arr(s.n, 0xD00000) if out_scale == "own" else out_scale
    y = arr(s.n, 0x900000) if y == "own" else y
    dw = arr(s.n, 0xA00000) if dw == "own" else dw
    db = arr(s.n, 0xB00000) if db == "own" else db
    c = C.byref(s.c) if stack else None
    return {
        "prepare": lambda: lib.dqrm_mlp_qact_prepare(c, prev, os_, None),
        "fwd": lambda: lib.dqrm_mlp_fwd_qact(c, flags, x, prev, os_, B, y, None),
        "bwd": lambda: lib.dqrm_mlp_bwd_qact(c, x, y, dy, prev, os_, B, None, dw, db, scratch, scratch_bytes, None),
    }


ALL3 = ("prepare", "fwd", "bwd")


def rejected(lib, calls, msg, which, code=L.DQRM_E_INVALID):
    for name in which:
        rc = calls[name]()
        if name == "bytes":
            assert rc == 0, name
        else:
            assert rc == code, (name, rc, lib.dqrm_last_error())
        assert msg in lib.dqrm_last_error(), (name, lib.dqrm_last_error())


# ------------------------------------------------------------------ header, binding, structs
def test_header_binding_and_abi(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12 and lib.dqrm_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"\}\s*dqrm_model_qact\s*;", code)
    # the structs the existing calls take are what they were; the new one is three pointers
    assert C.sizeof(L.Linear) == 6 * 4 + 5 * 8 and C.sizeof(L.MLP) == 8 + 3 * 8
    assert C.sizeof(L.Model) == 4 * 8 + 32 + 16 and C.sizeof(L.ActQuant) == 16 + 3 * 8
    assert C.sizeof(L.ModelQAct) == 3 * 8
    assert "no integer-activation" not in src


# ------------------------------------------------------------------ the stack exports
def test_stack_everything_check_mlp_rejects(lib):
    s = tensor_stack()
    rejected(lib, stack_calls(lib, s, stack=False), b"null stack", ALL3)
    for field in ("layers", "quantized", "act"):
        s = tensor_stack()
        setattr(s.c, field, None)
        rejected(lib, stack_calls(lib, s), b"null layers / quantized / act", ALL3)
    for n in (0, 17):
        s = tensor_stack()
        s.c.num_layers = n
        rejected(lib, stack_calls(lib, s), b"num_layers", ALL3)
    s = tensor_stack()
    s.lin[1].in_features = 5
    rejected(lib, stack_calls(lib, s), b"does not match", ALL3)
    s = tensor_stack(acts=(1, 3))
    rejected(lib, stack_calls(lib, s), b"act must be", ALL3)
    s = tensor_stack()
    s.lin[1].bias_bit = 33
    rejected(lib, stack_calls(lib, s), b"weight_bit / bias_bit", ALL3)
    s = tensor_stack()
    s.lin[0].bias_integer = None
    rejected(lib, stack_calls(lib, s), b"null weight_integer", ALL3)
    s = tensor_stack()
    s.lin[0].bias = None
    rejected(lib, stack_calls(lib, s), b"null weight / bias", ALL3)


def test_stack_full_precision_layer_and_inner_per_channel_rejected(lib):
    for quantized in ((0, 1), (1, 0), (0, 0)):
        s = tensor_stack(quantized=quantized)
        rejected(lib, stack_calls(lib, s), b"is full precision", ALL3)
    s = tensor_stack(per_channel=(1, 0))
    rejected(lib, stack_calls(lib, s), b"layer 0 is per_channel", ALL3)
    s = tensor_stack(widths=(6, 4, 3, 2), per_channel=(0, 1, 1))
    rejected(lib, stack_calls(lib, s), b"layer 1 is per_channel", ALL3)
    # per channel on the last layer passes: the calls stop at the next bad argument
    s = tensor_stack(per_channel=(0, 1))
    rejected(lib, stack_calls(lib, s, prev=None), b"null prev", ALL3)
    one = tensor_stack(widths=(9, 65), per_channel=(1,))
    rejected(lib, stack_calls(lib, one, prev=None), b"null prev", ALL3)


def test_stack_null_prev_arrays_and_entries_rejected(lib):
    s = tensor_stack()
    rejected(lib, stack_calls(lib, s, prev=None), b"null prev", ALL3)
    rejected(lib, stack_calls(lib, s, out_scale=NULLPP), b"null out_scale array", ALL3)
    hole = arr(s.n, 0xD00000)
    hole[1] = None
    rejected(lib, stack_calls(lib, s, out_scale=hole), b"null out_scale[1]", ALL3)
    rejected(lib, stack_calls(lib, s, x=None), b"null x", ("fwd", "bwd"))
    rejected(lib, stack_calls(lib, s, dy=None), b"null x / dy", ("bwd",))
    rejected(lib, stack_calls(lib, s, y=NULLPP), b"null y array", ("fwd", "bwd"))
    rejected(lib, stack_calls(lib, s, y=hole), b"null y[1]", ("fwd", "bwd"))
    rejected(lib, stack_calls(lib, s, dw=hole), b"null dw[1]", ("bwd",))
    rejected(lib, stack_calls(lib, s, db=hole), b"null db[1]", ("bwd",))
    rejected(lib, stack_calls(lib, s, dw=NULLPP), b"null dw array", ("bwd",))


def test_stack_flags_batch_size_and_scratch_rejected(lib):
    s = tensor_stack()
    rejected(lib, stack_calls(lib, s, flags=2), b"unknown flags", ("fwd",))
    rejected(lib, stack_calls(lib, s, B=-1), b"bad batch size", ("fwd", "bwd"))
    rejected(lib, stack_calls(lib, s, B=0), b"bad batch size", ("bwd",))
    rejected(lib, stack_calls(lib, s, B=1 << 31), b"bad batch size", ("fwd", "bwd"))
    need = lib.dqrm_mlp_bwd_scratch_bytes(C.byref(s.c), 5)
    assert need == 2 * 5 * 4 * 4
    rejected(lib, stack_calls(lib, s, scratch_bytes=need - 1), b"scratch", ("bwd",))
    rejected(lib, stack_calls(lib, s, scratch=None), b"scratch", ("bwd",))


# ------------------------------------------------------------------ the model exports
class FakeQAct:
    """A valid dqrm_model_qact on made-up addresses beside a FakeModel."""

    def __init__(self, f, running_stat=(1, 1)):
        self.q = []
        for k in range(2):
            q = L.ActQuant()
            q.activation_bit, q.running_stat, q.momentum, q.one_minus_momentum = 8, running_stat[k], -1.0, 2.0
            q.x_min, q.x_max, q.scale = (0x7000000 + 0x10000 * k + 0x1000 * j for j in range(3))
            self.q.append(q)
        self.os = arr(f.L, 0x7100000)
        self.c = L.ModelQAct()
        self.c.quant_input, self.c.quant_features = C.pointer(self.q[0]), C.pointer(self.q[1])
        self.c.out_scale = self.os


def qa_model(**kw):
    """FakeModel with per-tensor stacks (what a quantize_activation model has) unless overridden."""
    bot, top = kw.get("bot", (5, 16, 8)), kw.get("top", (14, 16, 1))
    kw.setdefault("bot_pc", [0] * (len(bot) - 1))
    kw.setdefault("top_pc", [0] * (len(top) - 1))
    return FakeModel(**kw)


def model_calls(lib, f, qa, flags=0, batch="own", nxt=None, x=0x5000000, labels=0x5100000, loss=0x5200000,
                g=0x5300000, ws=0x6000000, ws_bytes=1 << 40, model=True, qact=True):
    m = C.byref(f.m) if model else None
    a = C.byref(qa.c) if qact else None
    b = C.byref(f.batch) if batch == "own" else batch
    n = None if nxt is None else C.byref(nxt)
    dw, db = f.ptrs(0x4000000), f.ptrs(0x4100000)
    lay = L.ModelLayout()
    fwd_flags = flags & ~(REQUANT | NO_UPDATE)
    return {
        "fwd": lambda: lib.dqrm_model_fwd_qact(m, a, b, fwd_flags, x, labels, loss, None, ws, ws_bytes, None),
        "step": lambda: lib.dqrm_model_step_qact(m, a, b, n, flags, x, labels, 0.1, loss, None, g, dw, db, ws, ws_bytes,
                                                 None),
        "launches": lambda: lib.dqrm_model_qact_step_launches(m, a, b, n, flags),
        "bytes": lambda: lib.dqrm_model_qact_workspace_bytes(m, a, f.B, f.B),
        "layout": lambda: lib.dqrm_model_qact_workspace_layout(m, a, f.B, f.B, C.byref(lay)),
    }


ALL5 = ("fwd", "step", "launches", "bytes", "layout")
CALLS3 = ("fwd", "step", "launches")


def test_model_what_the_plain_calls_reject(lib):
    f = qa_model()
    qa = FakeQAct(f)
    rejected(lib, model_calls(lib, f, qa, model=False), b"null model", ALL5)
    f.m.top = None
    rejected(lib, model_calls(lib, f, qa), b"null tables / bottom / top / loss", ALL5)
    f = qa_model()
    f.bot.lin[1].in_features = 15
    rejected(lib, model_calls(lib, f, FakeQAct(f)), b"does not match", ALL5)
    f = qa_model(top=(15, 16, 1))
    rejected(lib, model_calls(lib, f, FakeQAct(f)), b"the top stack takes 15 features", ALL5)
    f = qa_model()
    qa = FakeQAct(f)
    rejected(lib, model_calls(lib, f, qa, batch=None), b"null batch", CALLS3)
    rejected(lib, model_calls(lib, f, qa, flags=16), b"unknown flags 0x10", CALLS3)
    rejected(lib, model_calls(lib, f, qa, x=None), b"null x", ("fwd", "step"))
    rejected(lib, model_calls(lib, f, qa, g=None), b"null x / labels / loss / g", ("step",))
    b0 = FakeModel.make_batch(0)
    rejected(lib, model_calls(lib, f, qa, batch=C.byref(b0)), b"B must be 1..1048576", CALLS3)
    assert lib.dqrm_model_qact_workspace_bytes(C.byref(f.m), C.byref(qa.c), 0, 33) == 0
    assert lib.dqrm_model_qact_workspace_bytes(C.byref(f.m), C.byref(qa.c), 33, -1) == 0
    assert lib.dqrm_model_qact_workspace_layout(C.byref(f.m), C.byref(qa.c), 33, 33, None) == L.DQRM_E_INVALID
    other = FakeModel.make_batch(34)
    rejected(lib, model_calls(lib, f, qa, nxt=other), b"next has 34 bags", ("step", "launches"))
    same = FakeModel.make_batch(33)
    rejected(lib, model_calls(lib, f, qa, nxt=same, flags=NO_UPDATE), b"a next batch needs the update",
             ("step", "launches"))


def test_model_qact_set_rejected(lib):
    f = qa_model()
    qa = FakeQAct(f)
    rejected(lib, model_calls(lib, f, qa, qact=False), b"null dqrm_model_qact", ALL5)
    for field in ("quant_input", "quant_features"):
        qa = FakeQAct(f)
        setattr(qa.c, field, None)
        rejected(lib, model_calls(lib, f, qa), b"null dqrm_act_quant", ALL5)
    for k in (0, 1):
        for bits in (1, 33):
            qa = FakeQAct(f)
            qa.q[k].activation_bit = bits
            rejected(lib, model_calls(lib, f, qa), b"activation_bit must be 2..32", ALL5)
        for field in ("x_min", "x_max", "scale"):
            qa = FakeQAct(f)
            setattr(qa.q[k], field, None)
            rejected(lib, model_calls(lib, f, qa), b"null x_min / x_max / scale", ALL5)
    qa = FakeQAct(f)
    qa.c.out_scale = NULLPP
    rejected(lib, model_calls(lib, f, qa), b"null out_scale array", ALL5)
    for hole, name in ((1, b"null out_scale[1]"), (3, b"null out_scale[1]")):  # bottom's second, top's second
        qa = FakeQAct(f)
        qa.os[hole] = None
        rejected(lib, model_calls(lib, f, qa), name, ALL5)


def test_model_per_channel_mixture_and_act_only(lib):
    f = qa_model(bot_pc=(1, 0))
    rejected(lib, model_calls(lib, f, FakeQAct(f)), b"layer 0 is per_channel", ALL5)
    f = qa_model(top_pc=(1, 0))
    rejected(lib, model_calls(lib, f, FakeQAct(f)), b"layer 0 is per_channel", ALL5)
    f = qa_model(bot_pc=(0, 1), top_pc=(0, 1))  # each stack's last layer may be
    assert model_calls(lib, f, FakeQAct(f))["launches"]() > 0
    # a mixture of quantized and full-precision layers
    for stack, i in (("bot", 0), ("bot", 1), ("top", 0), ("top", 1)):
        f = qa_model()
        getattr(f, stack).quantized[i] = 0
        rejected(lib, model_calls(lib, f, FakeQAct(f)), b"mixed", ALL5)
    f = qa_model()
    for i in range(2):
        f.bot.quantized[i] = 0
    rejected(lib, model_calls(lib, f, FakeQAct(f)), b"mixed", ALL5)
    # act-only: every layer full precision; out_scale is not read
    f = qa_model()
    for s in (f.bot, f.top):
        for i in range(2):
            s.quantized[i] = 0
    qa = FakeQAct(f)
    qa.c.out_scale = NULLPP
    calls = model_calls(lib, f, qa, flags=REQUANT)
    assert calls["launches"]() == 3 * 4 + 5 + 2 + 2 + 1
    assert calls["bytes"]() > 0


def test_model_workspace(lib):
    f = qa_model(qbits=16)
    qa = FakeQAct(f)
    T, D, R, X = 3, 8, 14, 5
    for B, ml in ((33, 33), (33, 500), (3300, 3300)):
        plain = lib.dqrm_model_workspace_bytes(C.byref(f.m), B, ml)
        need = lib.dqrm_model_qact_workspace_bytes(C.byref(f.m), C.byref(qa.c), B, ml)
        extra = 4 * B * (X + 2 * R) + lib.dqrm_act_quant_workspace_bytes(B * X) + lib.dqrm_act_quant_workspace_bytes(B * R)
        assert need >= plain + extra and need % 16 == 0
        a, b = L.ModelLayout(), L.ModelLayout()
        assert lib.dqrm_model_workspace_layout(C.byref(f.m), B, ml, C.byref(a)) == 0
        assert lib.dqrm_model_qact_workspace_layout(C.byref(f.m), C.byref(qa.c), B, ml, C.byref(b)) == 0
        # the existing cut first, at unchanged offsets
        for name in ("slab", "r", "p", "dr", "dx", "demb"):
            assert getattr(a, name) == getattr(b, name), name
        assert a.total == plain and b.total == need
    need = lib.dqrm_model_qact_workspace_bytes(C.byref(f.m), C.byref(qa.c), 33, 33)
    plain = lib.dqrm_model_workspace_bytes(C.byref(f.m), 33, 33)
    # short (the plain call's size is short here), null and misaligned
    for kw in ({"ws_bytes": need - 1}, {"ws_bytes": plain}, {"ws": None}, {"ws": 0x6000008}):
        rejected(lib, model_calls(lib, f, qa, **kw), b"workspace needs %d bytes" % need, ("fwd", "step"),
                 code=L.DQRM_E_WORKSPACE)


def test_model_step_launches_formula(lib):
    def count(f, flags, nxt=None, running_stat=(1, 1)):
        return model_calls(lib, f, FakeQAct(f, running_stat), flags=flags, nxt=nxt)["launches"]()

    def a(numel, running=1):  # a QuantAct forward's own launches
        return 1 if not running else (2 if numel <= 16384 else 3)

    f = qa_model()  # B = 33: x is 165 elements, r 462
    Lr = f.L
    base = 3 * Lr + a(33 * 5) + a(33 * 14) + 9
    assert base == 3 * 4 + 2 + 2 + 9
    assert count(f, FRESH | REQUANT) == base
    assert count(f, FRESH) == base - 1                   # an update without requantization: one launch
    assert count(f, FRESH | REQUANT | EMB_READY) == base - 1
    assert count(f, FRESH | NO_UPDATE) == base - 3       # no embedding update, no MLP update (two launches)
    # not fresh: two wquant launches per per-tensor layer in place of the two prepare launches
    assert count(f, REQUANT) == base - 2 + 2 * Lr
    assert count(f, NO_UPDATE) == base - 3 - 2 + 2 * Lr
    # fixed QuantActs: the elementwise pass alone
    assert count(f, FRESH | REQUANT, running_stat=(0, 0)) == 3 * Lr + 1 + 1 + 9
    assert count(f, FRESH | REQUANT, running_stat=(0, 1)) == 3 * Lr + 1 + 2 + 9
    # B on both sides of 16384 elements: r crosses it between B = 1170 and 1171, x between 3276 and 3277
    for B in (1170, 1171, 3276, 3277):
        g = qa_model(B=B)
        assert count(g, FRESH | REQUANT) == 3 * Lr + a(B * 5) + a(B * 14) + 9, B
    assert a(1170 * 14) == 2 and a(1171 * 14) == 3 and a(3276 * 5) == 2 and a(3277 * 5) == 3
    # the Kaggle stacks at B = 128
    kaggle = qa_model(T=26, D=16, bot=(13, 512, 256, 64, 16), top=(367, 512, 256, 1), B=128)
    assert count(kaggle, FRESH | REQUANT) == 35 == 3 * 7 + a(128 * 13) + a(128 * 367) + 9
    # a per-channel last layer: one wquant launch when not fresh; all per channel: one update launch
    pc = qa_model(bot=(5, 8), top=(14, 1), bot_pc=(1,), top_pc=(1,))
    assert count(pc, FRESH | REQUANT) == 3 * 2 + 2 + 2 + 9 - 1
    assert count(pc, REQUANT) == 3 * 2 + 2 + 2 + 9 - 1 - 2 + 2
    # the quantized interaction's scale
    assert count(qa_model(qbits=16), FRESH | REQUANT) == base + 1
    # the next batch's forward: inside the update's launch where the plain step has it there
    nxt = FakeModel.make_batch(33)
    one = lib.dqrm_bwd_sgd_fwd_is_one_launch(C.byref(f.ts), C.byref(f.batch), C.byref(nxt), f.m.emb_fwd_flags)
    assert count(f, FRESH | REQUANT, nxt) == base + 1 - one
    bags = FakeModel.make_batch(33, pooling_one=False, max_lookups=90)
    assert count(f, FRESH | REQUANT, bags) == base + 1
    # and always the plain step's count plus what the mode adds
    plain = lib.dqrm_model_step_launches(C.byref(f.m), C.byref(f.batch), None, FRESH | REQUANT)
    assert count(f, FRESH | REQUANT) == plain + 2 + 2 + 2 + 1


# ------------------------------------------------------------------ the Python layers' own errors
def test_python_construction_errors():
    np.random.seed(0)
    with pytest.raises(NotImplementedError, match="quantize_activation"):
        dq.MLPStack(dq.create_mlp([6, 4, 3], -1, quantize_activation=True))
    # the settings are checked before the device
    with pytest.raises(ValueError, match="per_channel"):
        dq.MLPStack(dq.create_mlp([6, 4, 3], -1, quantize_activation=True, per_channel=True))
    layers = dq.create_mlp([6, 4, 3], -1, quantize_activation=True)
    layers[2].quantize_activation = False
    with pytest.raises(ValueError, match="weight-only"):
        dq.MLPStack(layers)
    layers = dq.create_mlp([6, 4, 3], -1, quantize_activation=True)
    layers[0].full_precision_flag = True
    with pytest.raises(ValueError, match="full precision"):
        dq.MLPStack(layers)
    # full precision throughout is the weight-only stack it always was
    fp = dq.MLPStack(dq.create_mlp([6, 4, 3], -1, quantize_activation=True, full_precision_flag=True))
    assert not fp._qact
    with pytest.raises(NotImplementedError, match="CPU description"):
        dq.DQRMNet([7, 300, 1000], 8, [5, 16, 8], [14, 16, 1], quantize_activation=True, device="cpu")
