"""GPU: DotInteraction (interaction.py over csrc/dqrm_interact.hip) against a CPU restatement of
the reference's interact_features (tests/cpu_interact.py: dlrm_s_pytorch_comm_grad.py:701-806,
quant_utils.py:75-101, :196-220, :316-363), evaluated in float64 with autograd.

Shapes (B, F, D, itself), the smallest at which each mechanism can go wrong: one pair and one
16-byte load (1, 2, 4); the diagonal and its doubling (3, 2, 4, itself); the two real shapes with
351 pairs, which do not fill the last group of 64 lanes (5, 27, 16) and (7, 27, 64); more samples
than one pass of workgroups on a small device, ragged (130, 9, 128, itself); the F limit with 2016
pairs (67, 64, 8). The random-data test adds one shape for the kernels' other launch form (the largest
tile, past 64 KiB of LDS)."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import cpu_interact as R
import gen_inputs as G

pytestmark = pytest.mark.gpu


def _sid(s):
    return "B{}-F{}-D{}-{}".format(s[0], s[1], s[2], "self" if s[3] else "noself")


def _exact_ok(shape, bits):
    return bits != 16 or (shape[2] <= 16 and not shape[3])


EXACT_CASES = [(s, bits) for s in R.SHAPES for bits in (None, 8, 16) if _exact_ok(s, bits)]
EXACT_IDS = [_sid(s) + ("-plain" if not bits else f"-q{bits}") for s, bits in EXACT_CASES]
RANDOM_CASES = [(s, bits) for s in R.SHAPES + R.LDS_SHAPES for bits in (None, 16)]
RANDOM_IDS = [_sid(s) + ("-plain" if not bits else f"-q{bits}") for s, bits in RANDOM_CASES]


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


_REF = {}


def _reference(kind, shape, bits):
    """(x, emb, dr) and the float64 evaluation (R, dx, demb, s), computed once per case and
    shared by the tests (never modified)."""
    key = (kind, shape, bits)
    if key not in _REF:
        B, F, D, itself = shape
        if kind == "exact":
            inp = R.exact_case(B, F, D, itself, bits, seed=7 + B)
        else:
            inp = R.random_case(B, F, D, itself, seed=100 + D)
        _REF[key] = (inp, R.forward_backward(*inp, itself, bits))
    return _REF[key]


def _module_step(dq, x, emb, dr, itself, bits, x_grad=True, emb_grad=True, form="btd"):
    """R, x.grad, the slab's grad as [B, T, D], and the scale, of one forward + backward through
    the module. form: "btd" contiguous slab; "tbd" a [T, B, D] slab passed as its transposed view;
    "list" the reference's list of [B, D] tensors."""
    m = dq.DotInteraction(arch_interaction_itself=itself, quantize_bits=bits)
    xg = x.cuda().requires_grad_(x_grad)
    if form == "tbd":
        leaf = emb.transpose(0, 1).contiguous().cuda().requires_grad_(emb_grad)
        ly = leaf.transpose(0, 1)
        assert not ly.is_contiguous() or ly.shape[0] == 1 or ly.shape[1] == 1
    elif form == "list":
        leaf = [e.contiguous().cuda().requires_grad_(emb_grad) for e in emb.unbind(1)]
        ly = leaf
    else:
        leaf = emb.cuda().requires_grad_(emb_grad)
        ly = leaf
    out = m(xg, ly)
    if x_grad or emb_grad:
        out.backward(dr.cuda())
    if not emb_grad:
        de = None
    elif form == "tbd":
        de = leaf.grad.transpose(0, 1).cpu()
    elif form == "list":
        de = torch.stack([l.grad for l in leaf], dim=1).cpu()
    else:
        de = leaf.grad.cpu()
    s = m.feature_scaling_factor.cpu() if bits else None
    return out.detach().cpu(), (xg.grad.cpu() if x_grad else None), de, s


class CInteract:
    """The bare C calls on caller-owned buffers."""

    def __init__(self, dq, x, emb, itself, bits):
        self.L = dq._lib
        self.lib = self.L.load()
        self.x, self.emb = x.cuda().contiguous(), emb.cuda()
        assert self.emb.stride(2) == 1
        self.B, self.D = x.shape
        self.T = emb.shape[1]
        c = self.L.Interact()
        c.num_features, c.dim, c.self_interaction, c.quant_bits = self.T + 1, self.D, int(itself), bits or 0
        c.emb_stride_b, c.emb_stride_f = self.emb.stride(0), self.emb.stride(1)
        self.c = c
        self.W = self.lib.dqrm_interact_out_features(self.T + 1, self.D, int(itself))
        self.s = torch.zeros(1, device="cuda") if bits else None
        self.st = torch.cuda.current_stream().cuda_stream

    def _sp(self):
        return None if self.s is None else self.s.data_ptr()

    def scale(self):
        self.L.check(self.lib.dqrm_interact_scale(C.byref(self.c), self.x.data_ptr(), self.emb.data_ptr(), self.B,
                                                  self.s.data_ptr(), self.st), "scale")
        return self.s.cpu()

    def fwd(self):
        r = torch.full((self.B, self.W), float("nan"), device="cuda")
        self.L.check(self.lib.dqrm_interact_fwd(C.byref(self.c), self.x.data_ptr(), self.emb.data_ptr(), self.B,
                                                self._sp(), r.data_ptr(), self.st), "fwd")
        return r.cpu()

    def bwd(self, dr, want_dx=True, want_demb=True):
        dr = dr.cuda().contiguous()
        dx = torch.full_like(self.x, float("nan")) if want_dx else None
        de = torch.full((self.B, self.T, self.D), float("nan"), device="cuda") if want_demb else None
        self.L.check(self.lib.dqrm_interact_bwd(C.byref(self.c), self.x.data_ptr(), self.emb.data_ptr(),
                                                dr.data_ptr(), self.B, self._sp(),
                                                dx.data_ptr() if want_dx else None,
                                                de.data_ptr() if want_demb else None, self.st), "bwd")
        return (dx.cpu() if want_dx else None), (de.cpu() if want_demb else None)


def _eq(got, want64, what):
    """Bit equality with the float64 evaluation (which the caller has shown to be representable)."""
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.double().numpy(), want64.numpy(), err_msg=what)


def _same(a, b, what):
    np.testing.assert_array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32), err_msg=what)


# ------------------------------------------------------------------ 1. exact data, bit-exact
@pytest.mark.parametrize("shape,bits", EXACT_CASES, ids=EXACT_IDS)
def test_exact_data_forward_backward_bit_exact(dq, shape, bits):
    B, F, D, itself = shape
    (x, emb, dr), (R64, dx64, de64, s_r) = _reference("exact", shape, bits)
    # the construction: the float64 evaluation is representable in f32, so it is what exact f32
    # arithmetic gives in any order; in quantized mode s = 1/64 and the integers are 64 * T
    for t in (R64, dx64, de64):
        assert torch.equal(t.float().double(), t)
    if bits:
        T32 = R.features(x, emb)
        assert float(s_r) == 1.0 / 64
        assert torch.equal(R.feature_integers(T32, s_r, bits), T32 * 64)
        assert float((T32 * 64).abs().max()) == R.qmax(bits)
    # swapped features or a transposed pair order would change values
    assert not torch.equal(R64[:, D:], R.forward_backward(x, emb.flip(1), dr, itself, bits)[0][:, D:]) or F == 2
    # through the module with autograd
    r, dx, de, s = _module_step(dq, x, emb, dr, itself, bits)
    _eq(r, R64, "module R")
    _eq(dx, dx64, "module x.grad")
    _eq(de, de64, "module ly.grad")
    if bits:
        _same(s, s_r, "module feature_scaling_factor")
    # through the bare C calls
    c = CInteract(dq, x, emb, itself, bits)
    if bits:
        _same(c.scale(), s_r, "C scale")
    _eq(c.fwd(), R64, "C R")
    dx, de = c.bwd(dr)
    _eq(dx, dx64, "C dx")
    _eq(de, de64, "C demb")
    # dx = NULL and demb = NULL
    dx, de = c.bwd(dr, want_dx=False)
    assert dx is None
    _eq(de, de64, "C demb (dx NULL)")
    dx, de = c.bwd(dr, want_demb=False)
    assert de is None
    _eq(dx, dx64, "C dx (demb NULL)")
    r, dx, de, _ = _module_step(dq, x, emb, dr, itself, bits, x_grad=False)
    assert dx is None
    _eq(r, R64, "module R (x needs no gradient)")
    _eq(de, de64, "module ly.grad (x needs no gradient)")
    r, dx, de, _ = _module_step(dq, x, emb, dr, itself, bits, emb_grad=False)
    assert de is None
    _eq(dx, dx64, "module x.grad (ly needs no gradient)")
    # the [T, B, D] slab read in place through its transposed view, and the reference's list form
    for form in ("tbd", "list"):
        r, dx, de, s = _module_step(dq, x, emb, dr, itself, bits, form=form)
        _eq(r, R64, f"module R ({form})")
        _eq(dx, dx64, f"module x.grad ({form})")
        _eq(de, de64, f"module ly.grad ({form})")
    ct = CInteract(dq, x, emb.transpose(0, 1).contiguous().cuda().transpose(0, 1), itself, bits)
    if B > 1 and F > 2:  # (a dimension of one element has no stride to speak of)
        assert (ct.c.emb_stride_b, ct.c.emb_stride_f) == (D, B * D)
    if bits:
        _same(ct.scale(), s_r, "C scale (tbd strides)")
    _eq(ct.fwd(), R64, "C R (tbd strides)")
    dx, de = ct.bwd(dr)
    _eq(dx, dx64, "C dx (tbd strides)")
    _eq(de, de64, "C demb (tbd strides)")


# ------------------------------------------------------------------ 2. random data, derived bound
def _check_bound(got, want64, bound, what):
    err = (got.double() - want64).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


def _implied_integers(dq, x, emb, bits, s):
    """The integers the kernels form from (x, emb) in quantized mode, read back through the
    backward: with self-interaction and a gradient of 1/2 on the diagonal pairs only,
    dT[i, k] = ((g*s2 + g*s2) * Ti[i, k]) / s with g*s2 + g*s2 = s2, so round(dT / s) is Ti[i, k]
    (|Ti| < 2^15 and three roundings of 2^-24 relative error each)."""
    B, D = x.shape
    F = emb.shape[1] + 1
    li, lj = R.pair_lists(F, True)
    dr = torch.zeros(B, D + len(li))
    dr[:, D + torch.tensor([p for p, (i, j) in enumerate(zip(li, lj)) if i == j])] = 0.5
    c = CInteract(dq, x, emb, True, bits)
    _same(c.scale(), s, "scale of the probe")
    dx, de = c.bwd(dr)
    dT = torch.cat([dx.unsqueeze(1), de], dim=1).double()
    return torch.round(dT / s.double().view(()))


@pytest.mark.parametrize("shape,bits", RANDOM_CASES, ids=RANDOM_IDS)
def test_random_data_within_chain_bound(dq, shape, bits):
    """|result - float64 evaluation| <= gamma(m) * (sum of |products|), m the operation count:
    forward D + 1 (D + 2 quantized: s * s and the multiply by it); backward F + 2 (F + 3
    quantized: g * s2 with its s2, and / s), one more for dx's add. In quantized mode the float64
    evaluation runs on the restatement's f32 scale and integers, which the kernels' own must match
    bit for bit."""
    B, F, D, itself = shape
    (x, emb, dr), (R64, dx64, de64, s_r) = _reference("random", shape, bits)
    r, dx, de, s = _module_step(dq, x, emb, dr, itself, bits)
    q = 1 if bits else 0
    T64 = R.features(x, emb).double()
    if bits:
        _same(s, s_r, "feature_scaling_factor")
        Ti = R.feature_integers(R.features(x, emb), s_r, bits).double()
        np.testing.assert_array_equal(_implied_integers(dq, x, emb, bits, s_r).numpy(), Ti.numpy())
        s64 = s_r.double().view(())
        A, s2, inv = Ti.abs(), s64 * s64, 1.0 / s64
    else:
        A, s2, inv = T64.abs(), 1.0, 1.0
    li, lj = R.pair_lists(F, itself)
    _same(r[:, :D], x, "R[:, :D] is x, bit for bit")
    absZ = torch.bmm(A, A.transpose(1, 2))[:, torch.tensor(li), torch.tensor(lj)] * s2
    _check_bound(r[:, D:], R64[:, D:], R.gamma(D + 1 + q) * absZ, "R pairs")
    absdT = torch.bmm(R.coefficient_matrix(dr, F, D, itself) * s2, A) * inv
    _check_bound(de, de64, R.gamma(F + 2 + q) * absdT[:, 1:], "demb")
    _check_bound(dx, dx64, R.gamma(F + 3 + q) * (dr[:, :D].double().abs() + absdT[:, 0]), "dx")


# ------------------------------------------------------------------ 3. determinism, batch invariance
@pytest.mark.parametrize("bits", [None, 16], ids=["plain", "q16"])
def test_deterministic_and_batch_invariant(dq, bits):
    shape = (130, 9, 128, True)
    (x, emb, dr), _ = _reference("random", shape, bits)
    first = _module_step(dq, x, emb, dr, True, bits)
    second = _module_step(dq, x, emb, dr, True, bits)
    for a, b, what in zip(first[:3], second[:3], ("R", "dx", "demb")):
        _same(a, b, what + " run to run")
    if bits:
        _same(first[3], second[3], "scale run to run")
        return  # the scale is the batch's: rows alone quantize differently, as in the reference
    alone = _module_step(dq, x[:7].contiguous(), emb[:7].contiguous(), dr[:7].contiguous(), True, bits)
    for a, b, what in zip(alone[:3], first[:3], ("R", "dx", "demb")):
        _same(a, b[:7], what + ": rows 0..6 alone against rows 0..6 of the batch of 130")


# ------------------------------------------------------------------ 4. end to end
def test_end_to_end_with_package_modules(dq):
    """QuantEmbeddingBagCollection(layout="btd") -> DotInteraction -> QuantLinear, x from another
    QuantLinear, one backward(): the gradients that reach the collection's output and x are the
    bare C call's on the same tensors, and the list form gives the same R."""
    rows, D, B = [4, 300], 16, 12
    torch.manual_seed(0)
    coll = dq.QuantEmbeddingBagCollection(rows, D, weights=[torch.from_numpy(w) for w in G.table_weights(rows, D, 12)],
                                          grad_mode="dp")

    def ql(i, o):
        q = dq.QuantLinear(weight_bit=4, bias_bit=4, per_channel=True)
        q.set_param(nn.Linear(i, o).cuda())
        return q

    bot, inter = ql(13, D), dq.DotInteraction()
    top = ql(inter.out_features(len(rows) + 1, D), 1)
    lS_i = torch.from_numpy(G.pooling_one(rows, B, 20)).cuda()
    lS_o = torch.arange(B, device="cuda").repeat(len(rows), 1)
    dense = torch.rand(B, 13, device="cuda")

    x, _ = bot(dense)
    ly = coll(lS_o, lS_i, layout="btd")
    assert tuple(ly.shape) == (B, len(rows), D)
    x.retain_grad()
    ly.retain_grad()
    Rm = inter(x, ly)
    assert tuple(Rm.shape) == (B, D + 3)
    Rm.retain_grad()
    y, _ = top(Rm)
    y.pow(2).mean().backward()
    assert float(Rm.grad.abs().max()) > 0

    c = CInteract(dq, x.detach(), ly.detach(), False, None)
    assert c.emb.data_ptr() == ly.data_ptr()  # the slab is read in place
    _same(c.fwd(), Rm.detach().cpu(), "R")
    dx, de = c.bwd(Rm.grad)
    _same(dx, x.grad.cpu(), "x.grad")
    _same(de, ly.grad.cpu(), "gradient at the collection's output")
    assert bot.weight.grad is not None and float(bot.weight.grad.abs().max()) > 0
    # the reference's list form of ly, and the functional wrapper
    Rl = inter(x.detach(), list(ly.detach().unbind(1)))
    _same(Rl.cpu(), Rm.detach().cpu(), "R from the list form")
    Rf = dq.interact_features(x.detach(), tuple(ly.detach().unbind(1)))
    _same(Rf.cpu(), Rm.detach().cpu(), "interact_features, the functional wrapper")
    assert coll._tset.read_errors() == 0


# ------------------------------------------------------------------ 5. graph capture
def test_step_is_capturable_in_a_graph(dq):
    """The quantized step's calls (memset + scale, forward, backward) allocate nothing, do not
    synchronise and read nothing back: captured once on caller-owned buffers, each replay on new
    contents of those buffers equals the direct calls bit for bit."""
    shape = (5, 27, 16, False)
    (x, emb, dr), _ = _reference("random", shape, 16)
    c = CInteract(dq, x, emb, False, 16)
    drc = dr.cuda()
    r = torch.empty(c.B, c.W, device="cuda")
    dx, de = torch.empty_like(c.x), torch.empty(c.B, c.T, c.D, device="cuda")

    def calls(st):
        for rc in (c.lib.dqrm_interact_scale(C.byref(c.c), c.x.data_ptr(), c.emb.data_ptr(), c.B, c.s.data_ptr(), st),
                   c.lib.dqrm_interact_fwd(C.byref(c.c), c.x.data_ptr(), c.emb.data_ptr(), c.B, c.s.data_ptr(),
                                           r.data_ptr(), st),
                   c.lib.dqrm_interact_bwd(C.byref(c.c), c.x.data_ptr(), c.emb.data_ptr(), drc.data_ptr(), c.B,
                                           c.s.data_ptr(), dx.data_ptr(), de.data_ptr(), st)):
            c.L.check(rc, "captured call")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls(side.cuda_stream)  # first launches outside the capture (code object load)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls(torch.cuda.current_stream().cuda_stream)
    for scale_by in (1.0, 0.5):
        c.x.copy_(x.cuda() * scale_by)
        c.emb.copy_(emb.cuda() * (2.0 - scale_by))
        for t in (r, dx, de):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = (r.cpu(), dx.cpu(), de.cpu(), c.s.cpu())
        want_s, want_r = c.scale(), c.fwd()
        want_dx, want_de = c.bwd(dr)
        for a, b, what in zip(got, (want_r, want_dx, want_de, want_s), ("R", "dx", "demb", "scale")):
            _same(a, b, f"{what}: replay against the direct calls (inputs x {scale_by})")
