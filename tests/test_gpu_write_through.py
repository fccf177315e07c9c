"""GPU: the once-written outputs the kernels store write-through (16-B sc1 stores, DQRM_WT_STORES;
dqrm_device.h st4_out): the forwards' y and the N > 1 hand-over buffers. A store that goes past the L2 must still be what every later reader
sees -- a consumer on another stream, the next step into the same y, the host -- must write
whole rows and nothing around them, and must give the bits of the plain store.

Shapes: tables of 3 rows (dimension-split), 300 (narrow, one block pair), 2304 (row-split, nine
blocks over eight slots: an uneven slot) and 70000 (wide-span) rows; D = 16 (64-B rows, half an
L2 line) and 64; B = 96 (k_sgd_small takes the SGD step) and 257 (one past its 256 lookups, and
no multiple of any tile).
Reference: quant_modules_not_quantize_grad.py:317-398 (forward),
sgd_quantized_gradients_parallel_comm.py:601-628,850-890 (the DP update at world size 1)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ROWS = [3, 300, 2304, 70000]
CASES = [(16, 96), (16, 257), (64, 96), (64, 257)]
STEPS = 3
LR = 0.1
NAN_BITS = 0x7FC0BEEF  # a quiet NaN no kernel produces


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


def make_set(dq, Ws, packed=False):
    return dq.EmbeddingTableSet([w.shape[0] for w in Ws], Ws[0].shape[1], device="cuda", packed=packed,
                                init=None, weights=[torch.from_numpy(w) for w in Ws])


def inputs(D, B, ROWS=ROWS):
    Ws = G.table_weights(ROWS, D, 311)
    Ps = [G.pooling_one(ROWS, B, 320 + k, dist="zipf" if k else "uniform") for k in range(2)]
    dys = [G.upstream_grad(len(ROWS), B, D, 330 + k) * 10 for k in range(STEPS)]
    return Ws, Ps, dys


def run_steps(dq, D, B, consumer=None, ROWS=ROWS):
    """STEPS consecutive one-launch steps over two alternating batches into the same y; after
    each, consumer(k, ts, y, s_avg) (ordered on the device, no host wait in between)."""
    Ws, Ps, dys = inputs(D, B, ROWS)
    T = len(ROWS)
    ts = make_set(dq, Ws)
    bs = [dq.LookupBatch.pooling_one(torch.from_numpy(P).cuda()) for P in Ps]
    assert ts.apply_fwd_local_is_one_launch(bs[0], bs[1])
    ws = dq.CoalescedGrad.allocate(ROWS, B, D, "cuda")
    s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")
    y = torch.empty(T, B, D, dtype=torch.float32, device="cuda")
    ts.forward(bs[0], out=y)
    if consumer:
        consumer(-1, ts, y, s_avg)
    for k in range(STEPS):
        ts.backward_apply_forward_local(bs[k % 2], torch.from_numpy(dys[k]).cuda(), ws, 8, s_avg, LR, bs[(k + 1) % 2],
                                        out=y)
        if consumer:
            consumer(k, ts, y, s_avg)
    assert ts.read_errors() == 0
    return ts, y


_oracle_cache = {}


def oracle_steps(D, B):
    """Per step -1 .. STEPS-1: (y [T, B, D], scales [T], s_avg [T] or None, W copies); computed once
    per shape and never modified."""
    if (D, B) in _oracle_cache:
        return _oracle_cache[(D, B)]
    Ws, Ps, dys = inputs(D, B)
    T = len(ROWS)
    ar = np.arange(B, dtype=np.int64)
    Wo = [w.copy() for w in Ws]
    out = []

    def snap(nextP, s_avg):
        s = np.array([O.table_scale(Wo[t], 4) for t in range(T)], dtype=np.float32)
        y = np.stack([O.emb_fwd(Wo[t], nextP[t], ar, s[t])[0] for t in range(T)])
        out.append((y, s, s_avg, [w.copy() for w in Wo]))
        return s

    s = snap(Ps[0], None)
    for k in range(STEPS):
        P = Ps[k % 2]
        res = O.dp_step(Wo, [[(P[t], ar) for t in range(T)]], [[dys[k][t] for t in range(T)]], list(s), LR)
        s = snap(Ps[(k + 1) % 2], np.array([r[0] for r in res], dtype=np.float32))
    _oracle_cache[(D, B)] = out
    return out


@pytest.mark.parametrize("D,B", CASES)
def test_consecutive_steps_with_consumer_on_second_stream(dq, D, B):
    """Three one-launch steps into the same y; after each a copy kernel on a second stream,
    ordered behind the step by an event, reads y: oracle.emb_fwd on the oracle's W, bit for bit.
    W, the scales and the averaged gradient scale equal oracle.dp_step; the |W| hierarchy equals a
    rebuild."""
    ref = oracle_steps(D, B)
    side = torch.cuda.Stream()
    seen = []

    def consumer(k, ts, y, s_avg):
        main = torch.cuda.current_stream()
        done = torch.cuda.Event()
        done.record(main)
        side.wait_event(done)
        with torch.cuda.stream(side):
            yc = y.clone()                       # the consumer kernel: reads y from memory
            back = torch.cuda.Event()
            back.record(side)
        main.wait_event(back)                    # the next step rewrites y only after the read
        seen.append((yc, ts.scale.clone(), s_avg.clone(), ts.W.clone()))

    ts, _ = run_steps(dq, D, B, consumer)
    torch.cuda.synchronize()
    assert len(seen) == STEPS + 1
    for k, ((yc, sc, sa, W), (y_o, s_o, sa_o, W_o)) in enumerate(zip(seen, ref)):
        np.testing.assert_array_equal(yc.cpu().numpy(), y_o, err_msg=f"y after step {k - 1}")
        np.testing.assert_array_equal(sc.cpu().numpy(), s_o, err_msg=f"scale after step {k - 1}")
        if sa_o is not None:
            np.testing.assert_array_equal(sa.cpu().numpy(), sa_o, err_msg=f"s_avg of step {k - 1}")
        Wh = W.cpu().numpy()
        for t in range(len(ROWS)):
            b0 = ts.row_base[t]
            np.testing.assert_array_equal(Wh[b0:b0 + ROWS[t]], W_o[t], err_msg=f"W after step {k - 1} table {t}")
    inc = [x.clone() for x in (ts.rowmax, ts.blkmax, ts.sblkmax, ts.tmax)]
    ts.refresh_absmax()
    for name, a, b in zip(("rowmax", "blkmax", "sblkmax", "tmax"), inc, (ts.rowmax, ts.blkmax, ts.sblkmax, ts.tmax)):
        assert torch.equal(a, b), name


class DoubledOutStrides:
    """The library with the output strides of the named calls doubled: (..., out, stride_t,
    stride_b, stream) -> rows 2*D floats apart. The Python API derives the strides from the
    layout; the C ABI takes any multiple of 4 floats."""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in self._names:
            return f
        return lambda *a: f(*a[:-3], 2 * a[-3], 2 * a[-2], a[-1])


def strided_out(T, B, D):
    buf = torch.empty(T, B, 2 * D, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(NAN_BITS)
    return buf


def check_strided(buf, y_ref, D, what):
    h = buf.cpu().numpy()
    np.testing.assert_array_equal(h[:, :, :D], y_ref, err_msg=what)
    gap = h[:, :, D:].view(np.int32)
    assert (gap == np.int32(NAN_BITS)).all(), f"{what}: bytes between the rows were written"


@pytest.mark.parametrize("D,B", CASES)
def test_strided_output_keeps_the_bytes_between_rows(dq, D, B):
    """y as a strided view (row stride 2*D floats) of a buffer pre-filled with a NaN pattern, for
    every forward kernel: the rows are exact, every byte between them keeps the pattern."""
    from deep_quantized_recommendation_model_dqrm_amd import _lib as L
    from deep_quantized_recommendation_model_dqrm_amd.comm import HipExchangeKernels, payload_bytes

    ref = oracle_steps(D, B)
    Ws, Ps, dys = inputs(D, B)
    T = len(ROWS)
    ar = np.arange(B, dtype=np.int64)
    bs = [dq.LookupBatch.pooling_one(torch.from_numpy(P).cuda()) for P in Ps]
    names = {"dqrm_emb_fwd", "dqrm_emb_bwd_apply_fwd_local", "dqrm_emb_bwd_sgd_fwd", "dqrm_apply_sparse_update_fwd"}

    # k_emb_fwd
    ts = make_set(dq, Ws)
    ts.lib = DoubledOutStrides(ts.lib, names)
    buf = strided_out(T, B, D)
    ts.forward(bs[0], out=buf)
    check_strided(buf, ref[0][0], D, "forward")
    # k_coalesce_p1<., ., true>
    ws = dq.CoalescedGrad.allocate(ROWS, B, D, "cuda")
    s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")
    assert ts.apply_fwd_local_is_one_launch(bs[0], bs[1])
    buf = strided_out(T, B, D)
    ts.backward_apply_forward_local(bs[0], torch.from_numpy(dys[0]).cuda(), ws, 8, s_avg, LR, bs[1], out=buf)
    check_strided(buf, ref[1][0], D, "backward_apply_forward_local")
    assert ts.read_errors() == 0

    # k_emb_fwd_packed (the frozen scale the rows were packed with)
    tp = make_set(dq, Ws, packed=True)
    tp.refresh_scale_and_pack(4)
    tp.lib = DoubledOutStrides(tp.lib, names)
    buf = strided_out(T, B, D)
    tp.forward(bs[0], refresh_scale=False, use_packed=True, out=buf)
    check_strided(buf, ref[0][0], D, "packed forward")
    assert tp.read_errors() == 0

    # k_sgd_small<., true> (B <= 256 lookups), else the general kernel and k_emb_fwd
    tg = make_set(dq, Ws)
    tg.forward(bs[0])
    assert tg.sgd_fwd_is_one_launch(bs[0], bs[1]) == (B <= 256)
    Wg = [w.copy() for w in Ws]
    for t in range(T):
        assert O.emb_bwd_sgd(Wg[t], Ps[0][t], ar, dys[0][t], ref[0][1][t], LR) == 0
    sg = [O.table_scale(Wg[t], 4) for t in range(T)]
    yg = np.stack([O.emb_fwd(Wg[t], Ps[1][t], ar, sg[t])[0] for t in range(T)])
    tg.lib = DoubledOutStrides(tg.lib, names)
    buf = strided_out(T, B, D)
    tg.backward_sgd_forward(bs[0], torch.from_numpy(dys[0]).cuda(), LR, bs[1], out=buf)
    check_strided(buf, yg, D, "backward_sgd_forward")
    assert tg.read_errors() == 0

    # the N > 1 step's apply + forward at one rank (forced collectives): the flat apply with
    # k_finalize_fwd, then the merge apply's k_apply_pos<., true>
    caps = dq.default_caps(ROWS, B)
    cap_base = torch.tensor(np.concatenate([[0], np.cumsum(caps)]), dtype=torch.int64, device="cuda")
    cap_total = int(sum(caps))
    Pb = payload_bytes(T, cap_total, D, 8)
    lib = L.load()
    for kind in (L.DQRM_APPLY_AUTO, L.DQRM_APPLY_MERGE):
        prev = lib.dqrm_set_apply_kernel(kind)
        try:
            tc = make_set(dq, Ws)
            tc.forward(bs[0])
            k = HipExchangeKernels(tc)
            ws = dq.CoalescedGrad.allocate(ROWS, B, D, "cuda")
            payload = torch.zeros(1, Pb, dtype=torch.uint8, device="cuda")
            k.coalesce(bs[0], torch.from_numpy(dys[0]).cuda(), ws, True, "tbd")
            k.quant_pack(ws, ws.absmax.view(1, -1), 1, 8, cap_base, cap_total, s_avg, payload[0])
            k.lib = DoubledOutStrides(k.lib, names)
            buf = strided_out(T, B, D)
            k.apply_fwd(cap_base, cap_total, payload, Pb, 1, 8, s_avg, LR, L.DQRM_UPD_DP, False, bs[1], buf,
                        workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
            check_strided(buf, ref[1][0], D, f"apply_forward, apply kernel {kind}")
            assert tc.read_errors() == 0
        finally:
            lib.dqrm_set_apply_kernel(prev)


@pytest.mark.parametrize("D,B", CASES)
def test_hand_over_buffers_read_back_on_the_host(dq, D, B):
    """The coalesce workspace (rows, values, counts) and the quantize-pack payload, each written
    once for the next launch or the collective: on the host they equal the oracle's coalesced
    gradient and its int8 values (FP32 payload: the coalesced values themselves). Here under the
    process's switch value; test_switch_values_give_the_same_bits runs the same check in its
    children, so also with these buffers stored write-through (all)."""
    check_hand_over(dq, D, B)


def check_hand_over(dq, D, B):
    from deep_quantized_recommendation_model_dqrm_amd import _lib as L
    from deep_quantized_recommendation_model_dqrm_amd.comm import HipExchangeKernels, payload_bytes

    ref = oracle_steps(D, B)
    Ws, Ps, dys = inputs(D, B)
    T, S = len(ROWS), L.DQRM_TABLE_SPLIT
    ar = np.arange(B, dtype=np.int64)
    ts = make_set(dq, Ws)
    b = dq.LookupBatch.pooling_one(torch.from_numpy(Ps[0]).cuda())
    ts.forward(b)
    k = HipExchangeKernels(ts)
    ws = dq.CoalescedGrad.allocate(ROWS, B, D, "cuda")
    k.coalesce(b, torch.from_numpy(dys[0]).cuda(), ws, True, "tbd")
    rows_h, vals_h, cnt_h = ws.rows.cpu().numpy(), ws.vals.cpu().numpy(), ws.ucount.cpu().numpy()
    co = [O.emb_bwd_coalesce(ROWS[t], Ps[0][t], ar, dys[0][t], ref[0][1][t]) for t in range(T)]
    for t in range(T):
        r, v = [], []
        for s in range(S):
            b0, n = ws.slot_base[t * S + s], int(cnt_h[t * S + s])
            r.append(rows_h[b0:b0 + n])
            v.append(vals_h[b0:b0 + n])
        np.testing.assert_array_equal(np.concatenate(r), co[t][0], err_msg=f"workspace rows {t}")
        np.testing.assert_array_equal(np.concatenate(v), co[t][1], err_msg=f"workspace values {t}")
    caps = dq.default_caps(ROWS, B)
    base = np.concatenate([[0], np.cumsum(caps)])
    cap_base = torch.tensor(base, dtype=torch.int64, device="cuda")
    cap_total = int(sum(caps))
    a16 = lambda x: (x + 15) & ~15
    rows_off = a16(4 * T * S)
    vals_off = rows_off + a16(4 * cap_total)
    for bits, dt in ((8, np.int8), (32, np.float32)):
        Pb = payload_bytes(T, cap_total, D, bits)
        payload = torch.zeros(Pb, dtype=torch.uint8, device="cuda")
        s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")
        k.quant_pack(ws, ws.absmax.view(1, -1), 1, bits, cap_base, cap_total, s_avg, payload)
        ph = payload.cpu().numpy()
        counts = ph[:4 * T * S].view(np.int32).reshape(T, S)
        prow = ph[rows_off:rows_off + 4 * cap_total].view(np.int32)
        pval = ph[vals_off:vals_off + cap_total * D * np.dtype(dt).itemsize].view(dt).reshape(cap_total, D)
        for t in range(T):
            n = int(counts[t].sum())
            assert n == co[t][0].size
            np.testing.assert_array_equal(prow[base[t]:base[t] + n], co[t][0], err_msg=f"payload rows {bits} {t}")
            if bits == 32:
                want = co[t][1]
            else:
                sa = O.average_scale([O.grad_scale(co[t][1], bits)], 1)
                assert s_avg[t].item() == sa
                want = O.quantize(co[t][1], sa, bits)
            np.testing.assert_array_equal(pval[base[t]:base[t] + n].astype(np.float32), want,
                                          err_msg=f"payload values {bits} {t}")
    assert ts.read_errors() == 0


CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [{here!r}, {golden!r}, {oracle!r}, {root!r}]
import deep_quantized_recommendation_model_dqrm_amd as dq
import test_gpu_write_through as M
dq._lib.load()
out = {{}}
for D, B in M.CASES:
    ts, y = M.run_steps(dq, D, B)
    out["W_%d_%d" % (D, B)] = ts.W.cpu().numpy()
    out["y_%d_%d" % (D, B)] = y.cpu().numpy()
    M.check_hand_over(dq, D, B)
np.savez({path!r}, **out)
"""


def test_switch_values_give_the_same_bits(dq, tmp_path):
    """DQRM_WT_STORES is read once per process: one child per value (0 = plain stores everywhere,
    all = y and the hand-over buffers write-through, and the default) runs the consecutive steps
    of every shape and dumps W and y; the dumps are equal bit for bit. Each child also checks
    the hand-over buffers against the oracle (check_hand_over), under its switch value."""
    dumps = {}
    for val in ("0", "all", None):
        path = str(tmp_path / f"wt_{val}.npz")
        code = CHILD.format(here=HERE, golden=os.path.join(HERE, "golden"), oracle=os.path.join(ROOT, "oracle"),
                            root=ROOT, path=path)
        env = dict(os.environ)
        env.pop("DQRM_WT_STORES", None)
        if val is not None:
            env["DQRM_WT_STORES"] = val
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        dumps[val] = dict(np.load(path))
    ref = dumps["0"]
    assert sorted(ref) == sorted("%s_%d_%d" % (n, D, B) for n in "Wy" for D, B in CASES)
    for val in ("all", None):
        for name, a in ref.items():
            assert np.array_equal(a.view(np.uint32), dumps[val][name].view(np.uint32)), (val, name)
    D, B = CASES[-1]
    np.testing.assert_array_equal(ref["y_%d_%d" % (D, B)], oracle_steps(D, B)[-1][0])
