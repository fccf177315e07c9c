"""CPU checks of DotInteraction's host side: the four dqrm_interact_* exports in the header, the
binding and the library (added within ABI 12), the output width, every argument rule rejected
before any device call, and the module's error behaviour without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import cpu_interact as R
import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dqrm_interact_out_features", "dqrm_interact_scale", "dqrm_interact_fwd", "dqrm_interact_bwd")
A = 0x1000  # a 16-byte aligned stand-in for a device pointer (never dereferenced: validation fails first)


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


def _cfg(F=27, D=16, itself=0, bits=0, sb=None, sf=None):
    c = L.Interact()
    c.num_features, c.dim, c.self_interaction, c.quant_bits = F, D, itself, bits
    c.emb_stride_b = (F - 1) * D if sb is None else sb
    c.emb_stride_f = D if sf is None else sf
    return c


def test_exports_struct_and_abi_version(lib):
    src = open(os.path.join(ROOT, "include", "dqrm.h")).read()
    assert int(re.search(r"^#define\s+DQRM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 12
    assert L.DQRM_ABI_VERSION == 12 and lib.dqrm_abi_version() == 12
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "typedef struct dqrm_interact" in code
    # dqrm_interact: 4 x i32 + 2 x i64
    assert C.sizeof(L.Interact) == 16 + 16
    assert [n for n, _ in L.Interact._fields_] == ["num_features", "dim", "self_interaction", "quant_bits",
                                                   "emb_stride_b", "emb_stride_f"]


def test_package_exports_module_and_function():
    from deep_quantized_recommendation_model_dqrm_amd.interaction import DotInteraction, interact_features

    assert dq.DotInteraction is DotInteraction and dq.interact_features is interact_features
    assert "DotInteraction" in dq.__all__ and "interact_features" in dq.__all__
    m = dq.DotInteraction()
    assert (m.arch_interaction_itself, m.quantize_bits) == (False, None)
    m = dq.DotInteraction(arch_interaction_itself=True, quantize_bits=16)
    assert tuple(m.feature_scaling_factor.shape) == (1,)
    assert "feature_scaling_factor" not in m.state_dict()
    for bad in (1, 17):
        with pytest.raises(ValueError, match="quantize_bits"):
            dq.DotInteraction(quantize_bits=bad)


def test_out_features(lib):
    assert lib.dqrm_interact_out_features(27, 16, 0) == 367
    assert lib.dqrm_interact_out_features(27, 64, 0) == 415
    for F, D in [(2, 4), (27, 16), (27, 64), (9, 128), (64, 256)]:
        P = F * (F - 1) // 2
        assert lib.dqrm_interact_out_features(F, D, 0) == D + P == D + R.num_pairs(F, False)
        assert lib.dqrm_interact_out_features(F, D, 1) == D + P + F == D + R.num_pairs(F, True)
        assert len(R.pair_lists(F, True)[0]) == P + F and len(R.pair_lists(F, False)[1]) == P
    for F, D, field in [(1, 16, b"num_features"), (65, 16, b"num_features"), (27, 0, b"dim"), (27, 18, b"dim"),
                        (27, 260, b"dim")]:
        assert lib.dqrm_interact_out_features(F, D, 0) < 0
        assert field in lib.dqrm_last_error()


def _calls(lib, c, B=3, scale=None, x=A, emb=A, r=A, dr=A, dx=A, demb=A):
    """The three launching calls on one config (the scale call only in quantized mode)."""
    out = [("fwd", lambda: lib.dqrm_interact_fwd(C.byref(c), x, emb, B, scale, r, None)),
           ("bwd", lambda: lib.dqrm_interact_bwd(C.byref(c), x, emb, dr, B, scale, dx, demb, None))]
    if c.quant_bits:
        out.append(("scale", lambda: lib.dqrm_interact_scale(C.byref(c), x, emb, B, scale, None)))
    return out


def _rejected(lib, calls, field):
    for name, call in calls:
        assert call() == L.DQRM_E_INVALID, (name, field)
        assert field in lib.dqrm_last_error(), (name, field, lib.dqrm_last_error())


def test_argument_rules_rejected_without_device(lib):
    assert lib.dqrm_interact_fwd(None, A, A, 3, None, A, None) == L.DQRM_E_INVALID
    assert b"null interaction config" in lib.dqrm_last_error()
    for F in (1, 65, 0, -3):
        _rejected(lib, _calls(lib, _cfg(F=F, sb=64, sf=16)), b"num_features")
    for D in (0, 2, 6, 18, 258, 260, -4):
        _rejected(lib, _calls(lib, _cfg(D=D, sb=64, sf=16)), b"dim")
    for bits in (1, 17, -1, 32):
        _rejected(lib, _calls(lib, _cfg(bits=bits), scale=A), b"quant_bits")
    _rejected(lib, _calls(lib, _cfg(sb=27 * 16 + 2)), b"emb_stride_b")
    _rejected(lib, _calls(lib, _cfg(sb=-16)), b"emb_stride_b")
    _rejected(lib, _calls(lib, _cfg(sf=18)), b"emb_stride_f")
    _rejected(lib, _calls(lib, _cfg(sf=-4)), b"emb_stride_f")
    _rejected(lib, _calls(lib, _cfg(), B=-1), b"B must be")
    # the scale: non-NULL exactly when quantized
    _rejected(lib, _calls(lib, _cfg(bits=16), scale=None), b"scale")
    _rejected(lib, _calls(lib, _cfg(bits=0), scale=A), b"scale")
    assert lib.dqrm_interact_scale(C.byref(_cfg(bits=0)), A, A, 3, A, None) == L.DQRM_E_INVALID
    assert b"quant_bits" in lib.dqrm_last_error()
    # pointers: non-NULL and 16-byte aligned
    for kw, field in [(dict(x=None), b"null x"), (dict(x=A + 4), b"x is not 16-byte aligned"),
                      (dict(emb=None), b"null emb"), (dict(emb=A + 8), b"emb is not 16-byte aligned")]:
        _rejected(lib, _calls(lib, _cfg(), **kw), field)
        _rejected(lib, _calls(lib, _cfg(bits=8), scale=A, **kw), field)
    c = _cfg()
    assert lib.dqrm_interact_fwd(C.byref(c), A, A, 3, None, None, None) == L.DQRM_E_INVALID
    assert b"null r" in lib.dqrm_last_error()
    assert lib.dqrm_interact_fwd(C.byref(c), A, A, 3, None, A + 4, None) == L.DQRM_E_INVALID
    assert b"r is not 16-byte aligned" in lib.dqrm_last_error()
    for kw, field in [(dict(dr=None), b"null dr"), (dict(dr=A + 4), b"dr is not 16-byte aligned"),
                      (dict(dx=A + 4), b"dx is not 16-byte aligned"), (dict(demb=A + 12), b"demb is not 16-byte aligned")]:
        _rejected(lib, _calls(lib, c, **kw)[1:2], field)
    # a batch whose piece count leaves 32 bits is a capacity error, not a launch
    assert lib.dqrm_interact_fwd(C.byref(_cfg(F=64, D=256)), A, A, 2 ** 31 - 1, None, A, None) == L.DQRM_E_CAPACITY


def test_empty_batch_needs_no_device(lib):
    for bits, scale in ((0, None), (16, A)):
        c = _cfg(bits=bits)
        assert lib.dqrm_interact_fwd(C.byref(c), None, None, 0, scale, None, None) == L.DQRM_OK
        assert lib.dqrm_interact_bwd(C.byref(c), None, None, None, 0, scale, None, None, None) == L.DQRM_OK
    assert lib.dqrm_interact_scale(C.byref(_cfg(bits=16)), None, None, 0, A, None) == L.DQRM_OK
    # nothing asked of the backward: no launch either
    assert lib.dqrm_interact_bwd(C.byref(_cfg()), A, A, A, 3, None, None, None, None) == L.DQRM_OK


def test_module_errors_without_gpu():
    x, ly = torch.zeros(2, 8), torch.zeros(2, 3, 8)
    for m in (dq.DotInteraction(), dq.DotInteraction(True, 16)):
        with pytest.raises(L.DQRMError, match="no CPU path"):
            m(x, ly)
        with pytest.raises(L.DQRMError, match="no CPU path"):
            m(x, list(ly.unbind(1)))
    with pytest.raises(L.DQRMError, match="no CPU path"):
        dq.interact_features(x, ly, arch_interaction_itself=True)
    m = dq.DotInteraction()
    with pytest.raises(ValueError, match="float32"):
        m(x.double(), ly)
    with pytest.raises(ValueError, match="float32"):
        m(x, ly.half())
    with pytest.raises(ValueError, match="multiple of 4"):
        m(torch.zeros(2, 6), torch.zeros(2, 3, 6))
    with pytest.raises(ValueError, match="multiple of 4"):
        m(torch.zeros(2, 260), torch.zeros(2, 3, 260))
    with pytest.raises(ValueError, match=r"\[B, T, D\]"):
        m(x, torch.zeros(2, 8))            # rank
    with pytest.raises(ValueError, match=r"\[B, T, D\]"):
        m(x, torch.zeros(2, 3, 12))        # D of ly against D of x
    with pytest.raises(ValueError, match=r"\[B, T, D\]"):
        m(x, torch.zeros(3, 3, 8))         # batch
    with pytest.raises(ValueError, match="1..63"):
        m(x, torch.zeros(2, 64, 8))
    with pytest.raises(ValueError, match="quantize_bits"):
        dq.interact_features(x, ly, quantize_bits=1)


def test_stale_library_without_the_symbols_asks_for_a_rebuild(lib, monkeypatch):
    """load() on a libdqrm.so of the same ABI version built before these exports were added: the
    "rebuild it" DQRMError, not an AttributeError."""

    class Stale:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name.startswith("dqrm_interact_"):
                raise AttributeError(name)
            return getattr(self._real, name)

    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(C, "CDLL", lambda path, mode=0: Stale(lib))
    with pytest.raises(L.DQRMError, match="rebuild it"):
        L.load()


def test_restatement_matches_its_own_formula():
    """The float64 op sequence against the issue's closed form of the backward (c(i, j) and the
    chain over j), with and without the diagonal: the two agree to float64 rounding."""
    for B, F, D, itself in [(3, 5, 4, False), (2, 6, 8, True)]:
        x, emb, dr = R.random_case(B, F, D, itself, seed=F)
        Rr, dx, demb, s = R.forward_backward(x, emb, dr, itself, None)
        assert s is None and tuple(Rr.shape) == (B, D + R.num_pairs(F, itself))
        T = R.features(x, emb).double()
        li, lj = R.pair_lists(F, itself)
        Cm = torch.zeros(B, F, F, dtype=torch.float64)
        Cm[:, torch.tensor(li), torch.tensor(lj)] = dr[:, D:].double()
        Cm = Cm + Cm.transpose(1, 2)  # g(i,j) at (i,j) and (j,i); g(i,i) + g(i,i) on the diagonal
        dT = torch.bmm(Cm, T)
        torch.testing.assert_close(dx, dr[:, :D].double() + dT[:, 0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(demb, dT[:, 1:], rtol=1e-12, atol=1e-12)
        for p, (i, j) in enumerate(zip(li, lj)):
            torch.testing.assert_close(Rr[:, D + p], (T[:, i] * T[:, j]).sum(1), rtol=1e-12, atol=1e-12)
        assert torch.equal(Rr[:, :D], x.double())
    # the exact-data generators are what they say: s = 1/64, integers = m, float64 == f32
    for bits, shape in [(8, (3, 2, 4, True)), (16, (5, 27, 16, False))]:
        x, emb, dr = R.exact_case(*shape, bits, seed=1)
        T32 = R.features(x, emb)
        s = R.feature_scale(T32, bits)
        assert float(s) == 1.0 / 64 and float(1.0 / s) == 64.0
        Ti = R.feature_integers(T32, s, bits)
        assert torch.equal(Ti, T32 * 64) and float(Ti.abs().max()) == R.qmax(bits)
        for t in R.forward_backward(x, emb, dr, shape[3], bits)[:3]:
            assert torch.equal(t.float().double(), t)
