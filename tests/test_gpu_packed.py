"""GPU: the INT4 packed-row path (use_packed_int4 / EmbeddingTableSet(packed=True) /
forward(use_packed=True)) against the CPU oracle, at every width and through every update.

The reference has no packed rows, so the path must be invisible: `packed` always equals
oracle.pack_int4 of the W on the device with the scale the rows were packed with (pscale), and a
packed forward equals oracle.emb_fwd and the FP32-row forward. Every comparison is
np.testing.assert_array_equal on values (a packed single-lookup bag yields +0.0 where the FP32
path yields -0.0; the sign of a zero is not part of the contract). Inputs, references and the
preconditions that keep these cases from being vacuous: cpu_packed.py / test_packed_host.py.

  1  test_packed_forward_all_widths_and_bag_shapes   k_emb_fwd_packed's three row loads (one
     uint32, one uint2, 1..8 uint4) and k_emb_fwd's use_packed branch (D = 4); Criteo form,
     general bags of one, bags of 0..10; [T, B, D], [B, T, D], a strided view, both stores
  2  test_packed_forward_second_pass                 the bag loop's later passes, the partial
     last chunk, y above the write-through cut-off
  3  test_packed_forward_error_flags                 flags and zero rows as the FP32-row forward
  4  test_update_keeps_packed_rows / test_exchange_apply_keeps_packed_rows /
     test_simulated_dp_apply_keeps_packed_rows
                                                     every update with repack, also while
                                                     scale[] != pscale[]
  5  test_flagged_repack_and_repack_all
  6  test_modules_packed_on_equals_packed_off

Where the rows are packed (every store site, by function) and the section 4 - 6 cases that
reach it; found by building each site to store a marker byte of its own and running this file
(test ids: update = test_update_keeps_packed_rows, exchange = test_exchange_apply_keeps_packed_rows):

  site                                         reached by
  k_repack_flagged (dqrm_tables.hip)           every case (refresh_scale_and_pack, repack_all)
  k_rows_changed                               update[rows_changed-*]
  k_sgd_small                                  update[sgd / sgd_fwd, p96, D <= 64], modules[fused_sgd, sparse]
  fused_write (k_bwd_fused)                    update[local_mask-*; sgd / sgd_fwd on zipf1024, uni700,
  fused_segments_staged (k_bwd_fused)            bags130, and p96 at D = 256], modules[fused_sgd, sparse]
  update (k_coalesce_p1's update stage)        update[bwd_apply_local / bwd_apply_fwd_local on the Criteo forms]
  flat_row_apply (k_apply_flat*, apply_local)  update[hip_apply_local-*; bwd_apply_local / bwd_apply_fwd_local
                                               on bags130], exchange[flat / flat2 / flat4], simulated DP at
                                               D >= 16, modules[dp]
  apply_segments, the short-segment store      exchange[slot-*], simulated DP at D = 8 (two payloads >= D/4)
  apply_segments, the long-segment store       none here: a segment longer than LONG_SEG = 8 needs more than
    (dl_pack_int4)                             8 ranks' payloads; two ranks stay on the short-segment store
  k_apply_ranges                               exchange[ranges-*]
  k_apply_pos (merge)                          exchange[merge-*]
  recover_stalled (k_coalesce_p1)              none: it runs only after a workgroup gave up waiting for its
                                               table's other workgroups (DQRM_ERRF_STALL), which a healthy
                                               device does not produce and a test must not provoke
"""
import os

import numpy as np
import pytest
import torch

import cpu_packed as CP
import oracle as O

pytestmark = pytest.mark.gpu

f32 = np.float32
T = CP.T


@pytest.fixture(scope="module")
def dq():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import deep_quantized_recommendation_model_dqrm_amd as d

    d.build(verbose=False)
    d._lib.load()
    return d


APPLY_KERNELS = ["flat", "flat2", "flat4", "slot", "ranges", "merge"]


class _ApplyKernel:
    """Force dqrm_apply_sparse_update onto one kernel (as test_gpu_parity.py's apply_kernel)."""

    def __init__(self, dq, name):
        L = dq._lib
        self.lib = L.load()
        self.kind = {"flat": L.DQRM_APPLY_FLAT, "flat2": L.DQRM_APPLY_FLAT, "flat4": L.DQRM_APPLY_FLAT,
                     "slot": L.DQRM_APPLY_SLOT, "ranges": L.DQRM_APPLY_RANGES, "merge": L.DQRM_APPLY_MERGE}[name]
        self.dual = {"flat2": "2", "flat4": "4"}.get(name, "0")

    def __enter__(self):
        self.prev = self.lib.dqrm_set_apply_kernel(self.kind)
        self.old = os.environ.get("DQRM_FLAT_DUAL")
        os.environ["DQRM_FLAT_DUAL"] = self.dual

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DQRM_FLAT_DUAL", None)
        else:
            os.environ["DQRM_FLAT_DUAL"] = self.old
        self.lib.dqrm_set_apply_kernel(self.prev)


def make_set(dq, Ws, packed=True):
    return dq.EmbeddingTableSet([w.shape[0] for w in Ws], Ws[0].shape[1], device="cuda", packed=packed,
                                init=None, weights=[torch.from_numpy(w) for w in Ws])


def to_batch(dq, idxs, offs, p1):
    if p1:
        return dq.LookupBatch.pooling_one(torch.from_numpy(np.stack(idxs)).cuda())
    return dq.LookupBatch([torch.from_numpy(np.ascontiguousarray(i)) for i in idxs],
                          [torch.from_numpy(np.ascontiguousarray(o)) for o in offs], device="cuda")


def host(x):
    return x.detach().cpu().numpy()


def tables_of(ts, arr):
    return [arr[ts.row_base[t]: ts.row_base[t] + ts.num_rows[t]] for t in range(ts.T)]


def assert_packed_is_oracle(ts, scales=None):
    """packed[t] == pack_int4(W_t on the device, scales[t]) for ALL rows of every table;
    scales default to the set's pscale. Returns (W tables, scales)."""
    Wt = tables_of(ts, host(ts.W))
    Pt = tables_of(ts, host(ts.packed))
    s = host(ts.pscale) if scales is None else scales
    for t in range(ts.T):
        np.testing.assert_array_equal(Pt[t], O.pack_int4(Wt[t], s[t]), err_msg="table %d" % t)
    return Wt, s


def assert_fresh_pack(ts):
    """After refresh_scale_and_pack: scale == pscale == table_scale(W_t), rows packed with it."""
    Wt = tables_of(ts, host(ts.W))
    want = np.array([O.table_scale(w, 4) for w in Wt], dtype=f32)
    np.testing.assert_array_equal(host(ts.scale), want)
    np.testing.assert_array_equal(host(ts.pscale), want)
    assert_packed_is_oracle(ts, want)
    return Wt, want


# ------------------------------------------------------------------ 1. packed forward
@pytest.fixture(scope="module")
def fwd_sets(dq):
    """One packed set per width, packed once and checked against the oracle once."""
    cache = {}

    def get(D):
        if D not in cache:
            Ws = CP.fwd_weights(D)
            ts = make_set(dq, Ws)
            ts.refresh_scale_and_pack(4)
            _, s = assert_fresh_pack(ts)
            np.testing.assert_array_equal(s, CP.scales_of(Ws))
            cache[D] = (ts, Ws, s)
        return cache[D]

    return get


@pytest.mark.parametrize("form", CP.FWD_FORMS)
@pytest.mark.parametrize("D", CP.FWD_D)
def test_packed_forward_all_widths_and_bag_shapes(dq, fwd_sets, D, form):
    ts, Ws, s = fwd_sets(D)
    SENT = 12345.0
    for B in CP.fwd_B(D):
        idxs, offs, p1 = CP.fwd_batch(form, B, D)
        want = CP.fwd_reference(Ws, idxs, offs, s)
        b = to_batch(dq, idxs, offs, p1)
        assert b.pooling_one == p1
        y_u = host(ts.forward(b, refresh_scale=False, use_packed=False))
        y_p = host(ts.forward(b, refresh_scale=False, use_packed=True))
        np.testing.assert_array_equal(y_p, want, err_msg="B=%d" % B)
        np.testing.assert_array_equal(y_p, y_u, err_msg="B=%d" % B)
        for nt in (False, True):
            y = host(ts.forward(b, refresh_scale=False, use_packed=True, nt_store=nt))
            np.testing.assert_array_equal(y, want, err_msg="B=%d nt=%s" % (B, nt))
        y = host(ts.forward(b, refresh_scale=False, use_packed=True, layout="btd"))
        np.testing.assert_array_equal(y.transpose(1, 0, 2), want, err_msg="B=%d btd" % B)
        for nt in (False, True):  # a strided view of a wider buffer; nothing outside it is written
            buf = torch.full((B, T + 1, 2 * D), SENT, dtype=torch.float32, device="cuda")
            out = ts.forward(b, refresh_scale=False, use_packed=True, layout="btd", out=buf[:, :T, :D], nt_store=nt)
            assert out.data_ptr() == buf.data_ptr()
            h = host(buf)
            np.testing.assert_array_equal(h[:, :T, :D].transpose(1, 0, 2), want, err_msg="B=%d strided" % B)
            np.testing.assert_array_equal(h[:, T, :], f32(SENT))
            np.testing.assert_array_equal(h[:, :, D:], f32(SENT))
    assert ts.read_errors() == 0
    np.testing.assert_array_equal(host(ts.scale), s)  # no forward here refreshed the scale


# ------------------------------------------------------------------ 2. second pass
@pytest.fixture(scope="module")
def pass2_set(dq):
    Ws = CP.pass2_weights()
    ts = make_set(dq, Ws)
    ts.refresh_scale_and_pack(4)
    _, s = assert_fresh_pack(ts)
    return ts, Ws, s


@pytest.mark.parametrize("form", CP.P2_FORMS)
def test_packed_forward_second_pass(dq, pass2_set, form):
    """T = 256, B = 16384 + 257: the grid is capped at 64 chunks of 256 bags per table, so
    workgroups 0 and 1 run a second pass over the LDS staging (s_pk / s_len / s_beg) and the
    last one is a single bag; y (136 MB) is above the 32 MB write-through cut-off."""
    ts, Ws, s = pass2_set
    idxs, offs, p1 = CP.pass2_batch(form)
    want = CP.fwd_reference(Ws, idxs, offs, s)
    b = to_batch(dq, idxs, offs, p1)
    for nt in (False, True):
        y = ts.forward(b, refresh_scale=False, use_packed=True, nt_store=nt)
        np.testing.assert_array_equal(host(y), want, err_msg="nt=%s" % nt)
        del y
    y = ts.forward(b, refresh_scale=False, use_packed=False)
    np.testing.assert_array_equal(host(y), want)
    assert ts.read_errors() == 0


# ------------------------------------------------------------------ 3. error flags
@pytest.mark.parametrize("form", CP.ERR_FORMS)
@pytest.mark.parametrize("D", CP.ERR_D)
def test_packed_forward_error_flags(dq, D, form):
    """Out-of-range and negative indices (bags of one, bags of several) and a decreasing
    offset: all bounds-checked in the kernels. The packed forward raises the flags the
    FP32-row forward raises and yields its y (an invalid lookup contributes nothing)."""
    L = dq._lib
    ts = make_set(dq, CP.fwd_weights(D))
    ts.refresh_scale_and_pack(4)
    idxs, offs, p1 = CP.err_batch(form)
    b = to_batch(dq, idxs, offs, p1)
    assert ts.read_errors() == 0
    y_u = host(ts.forward(b, refresh_scale=False, use_packed=False))
    e_u = ts.read_errors()
    y_p = host(ts.forward(b, refresh_scale=False, use_packed=True))
    e_p = ts.read_errors()
    assert e_u == (L.DQRM_ERRF_OFFSET if form == "offsets" else L.DQRM_ERRF_INDEX)
    assert e_p == e_u
    np.testing.assert_array_equal(y_p, y_u)
    if form in ("single", "pool1"):  # the invalid bags of one are zero rows
        for t, bag in ((0, 3), (0, 6), (3, 0), (3, 7)):
            assert not y_p[t, bag].any()
    assert ts.read_errors() == 0


# ------------------------------------------------------------------ 4. updates keep packed == pack_int4(W, pscale)
def _gpu_inputs(dq, kind, D, step, ranks):
    ins = CP.upd_step_inputs(kind, D, step, ranks)
    return [(to_batch(dq, b[0], b[1], b[2]), torch.from_numpy(dy).cuda(), b) for b, dy in ins]


def _run_update_case(dq, D, kind, ranks, update, after_step=None):
    """The section 4 protocol. update(ts, step, inputs, next_batch) runs one update with
    repack=True and returns the next batch's y if it forwards it (else None)."""
    Ws = CP.upd_weights(D, kind)
    ts = make_set(dq, Ws)
    ts.refresh_scale_and_pack(4)
    assert_fresh_pack(ts)
    for step in range(CP.STEPS):
        odd = step % 2 == 1
        ins = _gpu_inputs(dq, kind, D, step, ranks)
        nb_host = CP.fresh_batch(kind, D, step)
        nb = to_batch(dq, nb_host[0], nb_host[1], nb_host[2])
        if odd:  # an FP32 forward with refresh rewrites scale[] only: repacks must use pscale[]
            ts.forward(ins[0][0], refresh_scale=True, use_packed=False)
            assert (host(ts.scale) != host(ts.pscale)).any()
        else:
            ts.refresh_scale_and_pack(4)
            np.testing.assert_array_equal(host(ts.scale), host(ts.pscale))
        ps0 = host(ts.pscale).copy()
        before = (ts.W.clone(), ts.packed.clone())
        y_upd = update(ts, step, ins, nb)
        Wt, ps = assert_packed_is_oracle(ts)
        np.testing.assert_array_equal(ps, ps0, err_msg="step %d: the update moved pscale" % step)
        if after_step is not None:
            after_step(ts, before)
        assert not torch.equal(before[0], ts.W)
        assert not torch.equal(before[1], ts.packed)
        if not odd:
            y_p = host(ts.forward(nb, refresh_scale=False, use_packed=True))
            y_u = host(ts.forward(nb, refresh_scale=False, use_packed=False))
            np.testing.assert_array_equal(y_p, y_u, err_msg="step %d" % step)
            want = CP.fwd_reference(Wt, nb_host[0], nb_host[1], ps)
            np.testing.assert_array_equal(y_p, want, err_msg="step %d" % step)
            if y_upd is not None:
                np.testing.assert_array_equal(host(y_upd), y_p, err_msg="step %d" % step)
        assert ts.read_errors() == 0, step
    ts.refresh_scale_and_pack(4)
    assert_fresh_pack(ts)
    return ts


def _ws(dq, b, D):
    return dq.CoalescedGrad.allocate(CP.ROWS, b.max_lookups, D, "cuda")


def _upd_sgd(dq, D):
    def f(ts, step, ins, nb):
        b, dy, _ = ins[0]
        ts.backward_sgd(b, dy, CP.LR, repack=True)
    return f


def _upd_sgd_fwd(dq, D):
    def f(ts, step, ins, nb):
        b, dy, _ = ins[0]
        return ts.backward_sgd_forward(b, dy, CP.LR, nb, refresh_scale=False, repack=True)
    return f


def _upd_local_mask(dq, D):
    mask = torch.tensor(CP.MASK, dtype=torch.int32, device="cuda")

    def f(ts, step, ins, nb):
        b, dy, _ = ins[0]
        ts.local_update(b, dy, CP.LR, table_mask=mask, repack=True)
    return f


def _upd_rows_changed(dq, D):
    def f(ts, step, ins, nb):
        _, _, hb = ins[0]
        rows, delta = [], []
        for t in range(T):
            u = CP.touched_rows(hb[0][t], CP.ROWS[t])
            rows.append(u + ts.row_base[t])
            delta.append(CP.write_delta(u.size, D, 9000 + 10 * step + t))
        rows = torch.from_numpy(np.concatenate(rows)).cuda()
        with torch.no_grad():
            ts.W[rows] = ts.W[rows] + torch.from_numpy(np.concatenate(delta)).cuda()
        ts.rows_changed(rows, repack=True)
    return f


def _upd_bwd_apply_local(dq, D):
    s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")

    def f(ts, step, ins, nb):
        b, dy, _ = ins[0]
        ts.backward_apply_local(b, dy, _ws(dq, b, D), 8, s_avg, CP.LR, repack=True)
    return f


def _upd_bwd_apply_fwd_local(dq, D):
    s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")

    def f(ts, step, ins, nb):
        b, dy, _ = ins[0]
        return ts.backward_apply_forward_local(b, dy, _ws(dq, b, D), 8, s_avg, CP.LR, nb, refresh_scale=False,
                                               repack=True)
    return f


def _upd_hip_apply_local(dq, D):
    from deep_quantized_recommendation_model_dqrm_amd.comm import HipExchangeKernels

    s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")

    def f(ts, step, ins, nb):
        b, dy, _ = ins[0]
        ws = _ws(dq, b, D)
        ts.backward_coalesce(b, dy, ws)
        HipExchangeKernels(ts).apply_local(ws, 8, s_avg, CP.LR, True)
    return f


UPDATES = {"sgd": _upd_sgd, "sgd_fwd": _upd_sgd_fwd, "local_mask": _upd_local_mask, "rows_changed": _upd_rows_changed,
           "bwd_apply_local": _upd_bwd_apply_local, "bwd_apply_fwd_local": _upd_bwd_apply_fwd_local,
           "hip_apply_local": _upd_hip_apply_local}


@pytest.mark.parametrize("kind", CP.BATCH_KINDS)
@pytest.mark.parametrize("D", CP.UPD_D)
@pytest.mark.parametrize("update", list(UPDATES))
def test_update_keeps_packed_rows(dq, update, D, kind):
    after = None
    if update == "local_mask":
        def after(ts, before):  # masked-out tables: W and packed rows byte-identical
            for t in range(T):
                if not CP.MASK[t]:
                    lo, hi = ts.row_base[t], ts.row_base[t] + ts.num_rows[t]
                    assert torch.equal(before[0][lo:hi], ts.W[lo:hi]), t
                    assert torch.equal(before[1][lo:hi], ts.packed[lo:hi]), t
    _run_update_case(dq, D, kind, 1, UPDATES[update](dq, D), after)


def test_sgd_forward_runs_in_both_forms(dq):
    """test_update_keeps_packed_rows[sgd_fwd] runs backward_sgd_forward once as one launch
    (the small Criteo batch) and once as two (1024 lookups per table), at D = 16."""
    ts = make_set(dq, CP.upd_weights(16, "p96"))
    forms = {}
    for kind in ("p96", "zipf1024"):
        b = CP.upd_batch(kind, 5016)
        nb = CP.fresh_batch(kind, 16, 0)
        forms[kind] = ts.sgd_fwd_is_one_launch(to_batch(dq, b[0], b[1], b[2]), to_batch(dq, nb[0], nb[1], nb[2]))
    assert forms == {"p96": True, "zipf1024": False}


def _payloads(dq, ts, ins, grad_bits):
    """Every rank's coalesce + quantize-pack on one GPU (the all-gathers become stacking), as
    test_gpu_parity.py's _emulate_ranks."""
    from deep_quantized_recommendation_model_dqrm_amd.comm import HipExchangeKernels, payload_bytes

    N = len(ins)
    k = HipExchangeKernels(ts)
    max_lookups = max(b.max_lookups for b, _, _ in ins)
    wss = []
    for b, dy, _ in ins:
        ws = dq.CoalescedGrad.allocate(ts.num_rows, max_lookups, ts.D, "cuda")
        k.coalesce(b, dy, ws, True, "tbd")
        wss.append(ws)
    absmax_all = torch.stack([ws.absmax for ws in wss])
    caps = dq.default_caps(ts.num_rows, max_lookups)
    cap_base = torch.tensor(np.concatenate([[0], np.cumsum(caps)]), dtype=torch.int64, device="cuda")
    cap_total = int(sum(caps))
    P = payload_bytes(ts.T, cap_total, ts.D, grad_bits)
    payloads = torch.zeros(N, P, dtype=torch.uint8, device="cuda")
    s_avg = torch.zeros(ts.T, dtype=torch.float32, device="cuda")
    for r in range(N):
        k.quant_pack(wss[r], absmax_all, N, grad_bits, cap_base, cap_total, s_avg, payloads[r])
    return k, cap_base, cap_total, payloads, P, s_avg


def _exchange_update(dq, kernel, call, mode, D):
    """update() of _run_update_case: HipExchangeKernels.apply / apply_fwd of the ranks' payloads
    under one apply kernel, quantized (DQRM_UPD_DP) or FP32 (DQRM_UPD_FP32) payloads."""
    L = dq._lib
    gb, m = (8, L.DQRM_UPD_DP) if mode == "dp" else (32, L.DQRM_UPD_FP32)

    def update(ts, step, ins, nb):
        N = len(ins)
        k, cap_base, cap_total, payloads, P, s_avg = _payloads(dq, ts, ins, gb)
        with _ApplyKernel(dq, kernel):
            if call == "apply":
                k.apply(cap_base, cap_total, payloads, P, N, gb, s_avg, CP.LR, m, True)
                return None
            ws = torch.zeros(max(16, int(k.lib.dqrm_apply_workspace_bytes(N, cap_total))), dtype=torch.uint8,
                             device="cuda")
            y = torch.empty(T, nb.num_bags, D, device="cuda")
            return k.apply_fwd(cap_base, cap_total, payloads, P, N, gb, s_avg, CP.LR, m, True, nb, y,
                               refresh_scale=False, workspace=ws)

    return update


@pytest.mark.parametrize("kind", CP.FAMILY_KINDS["dp2"])
@pytest.mark.parametrize("D", CP.UPD_D)
@pytest.mark.parametrize("mode", ["dp", "fp32"])
@pytest.mark.parametrize("call", ["apply", "apply_fwd"])
@pytest.mark.parametrize("kernel", APPLY_KERNELS)
def test_exchange_apply_keeps_packed_rows(dq, kernel, call, mode, D, kind):
    """HipExchangeKernels.apply / apply_fwd of two emulated ranks' payloads, under each apply
    kernel, quantized (DQRM_UPD_DP) and FP32 (DQRM_UPD_FP32) payloads."""
    _run_update_case(dq, D, kind, 2, _exchange_update(dq, kernel, call, mode, D))


@pytest.mark.parametrize("kind", CP.BATCH_KINDS)
@pytest.mark.parametrize("D", CP.UPD_D)
def test_simulated_dp_apply_keeps_packed_rows(dq, D, kind):
    """The simulated-DP buffer (sgd_quantized_gradients._MicroStepBuffer): two micro-steps
    accumulated, then its apply with repack (DQRM_UPD_SIMULATED)."""
    from deep_quantized_recommendation_model_dqrm_amd.sgd_quantized_gradients import _MicroStepBuffer

    def update(ts, step, ins, nb):
        buf = _MicroStepBuffer(ts, max(b.max_lookups for b, _, _ in ins))
        for b, dy, _ in ins:
            buf.accumulate(b, dy, True, "tbd")
        buf.apply(CP.LR, len(ins), True)
        buf.zero()

    _run_update_case(dq, D, kind, 2, update)


# ------------------------------------------------------------------ 5. flagged repack, repack_all
@pytest.mark.parametrize("D", CP.FLAG_D)
def test_flagged_repack_and_repack_all(dq, D):
    """refresh_scale_and_pack repacks only tables whose scale moved (k_refresh_scale flags,
    k_repack_flagged packs): a sentinel byte in an untouched row survives in the table that kept
    its scale and is overwritten in the one that did not; repack_all rewrites every table."""
    ts = make_set(dq, CP.flag_weights(D))
    ts.refresh_scale_and_pack(4)
    _, s0 = assert_fresh_pack(ts)
    idxs, offs, p1, B = CP.flag_batch(D)
    sites = [(CP.FLAG_KEEP, CP.FLAG_KEEP_ROW), (CP.FLAG_MOVE, CP.FLAG_MOVE_ROW)]
    col = D // 2 - 1
    sent = {}
    for t, r in sites:
        true = int(ts.table_packed(t)[r, col].item())
        sent[t] = true ^ 0xFF
        ts.table_packed(t)[r, col] = sent[t]
    ts.backward_sgd(to_batch(dq, idxs, offs, p1), torch.from_numpy(CP.flag_dy(D)).cuda(), CP.LR, repack=True)
    for t, r in sites:  # the update repacks the rows it touched, no others
        assert int(ts.table_packed(t)[r, col].item()) == sent[t]
    ts.refresh_scale_and_pack(4)
    s1 = host(ts.scale)
    assert s1[CP.FLAG_KEEP] == s0[CP.FLAG_KEEP] and s1[CP.FLAG_MOVE] != s0[CP.FLAG_MOVE]
    assert int(ts.table_packed(CP.FLAG_KEEP)[CP.FLAG_KEEP_ROW, col].item()) == sent[CP.FLAG_KEEP]
    Wt = tables_of(ts, host(ts.W))
    Pt = tables_of(ts, host(ts.packed))
    for t in range(T):  # everything but the kept sentinel is the oracle's packing
        want = O.pack_int4(Wt[t], s1[t])
        if t == CP.FLAG_KEEP:
            assert want[CP.FLAG_KEEP_ROW, col] == sent[t] ^ 0xFF
            want[CP.FLAG_KEEP_ROW, col] = sent[t]
        np.testing.assert_array_equal(Pt[t], want, err_msg="table %d" % t)
    ts.repack_all(4)
    assert_fresh_pack(ts)
    assert ts.read_errors() == 0


# ------------------------------------------------------------------ 6. modules
class _Model(torch.nn.Module):
    """emb_l (a collection, or a ModuleList of one-table modules) as the DP hooks expect it."""

    def __init__(self, kind, D, Ws, mode, packed):
        super().__init__()
        from deep_quantized_recommendation_model_dqrm_amd.quant_modules_not_quantize_grad import (
            QuantEmbeddingBagCollection, QuantEmbeddingBagTwo)

        kw = dict(grad_mode=mode, lr=CP.MOD_LR if mode == "fused_sgd" else None, use_packed_int4=packed)
        self.kind = kind
        if kind == "collection":
            self.emb_l = QuantEmbeddingBagCollection(CP.ROWS, D, weights=[torch.from_numpy(w) for w in Ws], **kw)
        else:
            self.emb_l = torch.nn.ModuleList([QuantEmbeddingBagTwo(n, D, weight=torch.from_numpy(w), embedding_id=t, **kw)
                                              for t, (n, w) in enumerate(zip(CP.ROWS, Ws))])
        self.bot_l = torch.nn.Sequential()
        self.top_l = torch.nn.Sequential()

    def forward(self, idxs, offs, **kw):
        """y [B, T, D]"""
        if self.kind == "collection":
            return self.emb_l(offs, idxs, layout="btd", **kw)
        return torch.stack([e(idxs[t], offs[t], **kw) for t, e in enumerate(self.emb_l)], dim=1)

    def sets(self):
        mods = [self.emb_l] if self.kind == "collection" else list(self.emb_l)
        return [m._tset for m in mods]


def _train_module(dq, kind, D, mode, packed):
    """4 steps (Criteo form, bags, Criteo form, bags), one full-precision forward after step 2.
    Returns (ys, final W per table, model)."""
    from deep_quantized_recommendation_model_dqrm_amd import sgd_quantized_gradients_parallel_comm as H

    model = _Model(kind, D, CP.mod_weights(D), mode, packed)
    opt = torch.optim.SGD(model.parameters(), lr=CP.MOD_LR) if mode == "sparse" else None
    ys = []
    for step in range(CP.MOD_STEPS):
        idxs, offs = CP.mod_batch(step, D)
        idxs = [torch.from_numpy(i).cuda() for i in idxs]
        offs = [torch.from_numpy(o).cuda() for o in offs]
        g = torch.from_numpy(CP.mod_grad(step, D)).cuda()
        if mode == "dp":
            H.clear_gradients(model)
        elif opt is not None:
            opt.zero_grad(set_to_none=True)
        y = model(idxs, offs)
        ys.append(host(y))
        (y * g).sum().backward()
        if mode == "dp":
            H.grad_update_parallel_comm(model, 1, emb_grad_quantized=True, num_bits=8)
            H.weight_update_parallel_comm(model, CP.MOD_LR, emb_grad_quantized=True, num_gpus=1)
        elif opt is not None:
            opt.step()
        if step == 2:
            with torch.no_grad():
                ys.append(host(model(idxs, offs, full_precision_flag=True)))
    sets = model.sets()
    assert all(ts.read_errors() == 0 for ts in sets)
    W = [w for ts in sets for w in tables_of(ts, host(ts.W))]
    return ys, W, model


@pytest.mark.parametrize("D", CP.MOD_D)
@pytest.mark.parametrize("mode", CP.MOD_MODES)
@pytest.mark.parametrize("kind", CP.MOD_KINDS)
def test_modules_packed_on_equals_packed_off(dq, kind, mode, D):
    """QuantEmbeddingBagCollection (T = 4) and a ModuleList of QuantEmbeddingBagTwo, built with
    use_packed_int4 on and off from the same weights: every step's y (the full-precision
    forward included) and the final W are equal, no error flag, and the packed build's rows
    are pack_int4(W, pscale) at the end."""
    ys1, W1, m1 = _train_module(dq, kind, D, mode, True)
    ys0, W0, m0 = _train_module(dq, kind, D, mode, False)
    assert len(ys1) == CP.MOD_STEPS + 1
    for k, (a, b) in enumerate(zip(ys1, ys0)):
        np.testing.assert_array_equal(a, b, err_msg="y %d" % k)
    W_init = CP.mod_weights(D)
    for t in range(T):
        np.testing.assert_array_equal(W1[t], W0[t], err_msg="table %d" % t)
        assert not np.array_equal(W1[t], W_init[t])
    assert all(ts.packed is None for ts in m0.sets())
    for ts in m1.sets():
        assert ts.packed is not None
        assert_packed_is_oracle(ts)
