"""What each launch-form query of the embedding step says is what its launcher issues, by the
kernel names torch.profiler records: dqrm_bwd_sgd_fwd_is_one_launch, the two local-step queries
and dqrm_apply_fwd_form against dqrm_emb_bwd_sgd_fwd, dqrm_emb_bwd_apply_local,
dqrm_emb_bwd_apply_fwd_local and dqrm_apply_sparse_update_fwd. Small shapes (T = 3, B = 64): only
the launches are looked at here, the results are tests/test_gpu_parity.py's."""
import numpy as np
import pytest
import torch

import gen_inputs as G
from test_gpu_metrics import _kernels
from test_gpu_parity import _payloads_for_ranks, dq, to_batch  # noqa: F401  (dq: the fixture)

pytestmark = pytest.mark.gpu

ROWS, B = [7, 300, 5000], 64
T = len(ROWS)


def _criteo(dq, seed):
    return dq.LookupBatch.pooling_one(torch.from_numpy(G.pooling_one(ROWS, B, seed)).cuda())


def _two_per_bag(dq, seed):
    rs = np.random.RandomState(seed)
    return to_batch(dq, [rs.randint(0, n, 2 * B).astype(np.int64) for n in ROWS],
                    [np.arange(B, dtype=np.int64) * 2 for _ in ROWS])


BATCH = {"criteo": _criteo, "two_per_bag": _two_per_bag}


def _launched(fn):
    """The library's kernels fn launched. A torch op runs first as the control: if the profile
    does not show it, the profile shows nothing and the test fails."""
    def both():
        torch.ones(8, device="cuda").mul_(2.0)
        fn()

    _, names = _kernels(both)
    control = [n for n in names if "at::native" in n]
    assert control, ("the profile lacks the control launch", names)
    return [n for n in names if "at::native" not in n]


def _has(names, what):
    return any(what in n for n in names)


def _set(dq, D):
    return dq.EmbeddingTableSet(ROWS, D, device="cuda", init="uniform", seed=5)


def _dy(D, seed):
    return torch.from_numpy(G.upstream_grad(T, B, D, seed)).cuda()


@pytest.mark.parametrize("D", [16, 64])
def test_sgd_fwd_query_is_what_the_launcher_issues(dq, D):
    ts = _set(dq, D)
    said = set()
    for update, nxt in [("criteo", "criteo"), ("two_per_bag", "criteo"), ("criteo", "two_per_bag"),
                        ("two_per_bag", "two_per_bag")]:
        b, nb = BATCH[update](dq, 11), BATCH[nxt](dq, 12)
        ts.forward(b)
        one = ts.sgd_fwd_is_one_launch(b, nb)
        names = _launched(lambda: ts.backward_sgd_forward(b, _dy(D, 13), 0.1, nb))
        print(D, update, nxt, "one launch:", one, names)
        if one:
            assert len(names) == 1 and not _has(names, "k_emb_fwd"), names
        else:
            assert _has(names, "k_emb_fwd"), names
        said.add(one)
    assert said == {True, False}  # both forms were looked at
    assert ts.read_errors() == 0


@pytest.mark.parametrize("D", [16, 64])
def test_local_step_queries_are_what_the_launchers_issue(dq, D):
    ts = _set(dq, D)
    ws = dq.CoalescedGrad.allocate(ROWS, 2 * B, D, "cuda")
    s_avg = torch.zeros(T, dtype=torch.float32, device="cuda")
    said, said_fwd = set(), set()
    for update, nxt in [("criteo", "criteo"), ("criteo", "two_per_bag"), ("two_per_bag", "criteo")]:
        b, nb = BATCH[update](dq, 21), BATCH[nxt](dq, 22)
        ts.forward(b)
        one = ts.apply_local_is_one_launch(b)
        names = _launched(lambda: ts.backward_apply_local(b, _dy(D, 23), ws, 8, s_avg, 0.1))
        print(D, update, "update in one launch:", one, names)
        assert not _has(names, "k_emb_fwd"), names
        assert (len(names) == 1) == one, names
        said.add(one)
        one_fwd = ts.apply_fwd_local_is_one_launch(b, nb)
        names = _launched(lambda: ts.backward_apply_forward_local(b, _dy(D, 24), ws, 8, s_avg, 0.1, nb))
        print(D, update, nxt, "update and forward in one launch:", one_fwd, names)
        if one_fwd:
            assert len(names) == 1 and not _has(names, "k_emb_fwd"), names
        else:
            assert _has(names, "k_emb_fwd"), names
            assert (len(names) == 2) == one, names  # the one-launch update, then the forward
        said_fwd.add(one_fwd)
    assert said == {True, False} and said_fwd == {True, False}
    assert ts.read_errors() == 0


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("D", [16, 64])
def test_apply_fwd_form_is_what_the_launcher_issues(dq, D, N):
    from deep_quantized_recommendation_model_dqrm_amd import _lib as L
    from deep_quantized_recommendation_model_dqrm_amd.comm import HipExchangeKernels

    lib = L.load()
    ts = _set(dq, D)
    rb = [_criteo(dq, 31 + r) for r in range(N)]
    ts.forward(rb[0])
    payloads, s_avg, cap_base, cap_total = _payloads_for_ranks(dq, ts, rb, [_dy(D, 41 + r) for r in range(N)], 8)
    kern = HipExchangeKernels(ts)
    ws = torch.zeros(max(16, int(lib.dqrm_apply_workspace_bytes(N, cap_total))), dtype=torch.uint8, device="cuda")
    out = torch.empty(T, B, D, device="cuda")
    flags = ts._fwd_flags(True, False, False)
    forms = set()
    for kind in ("AUTO", "FLAT", "SLOT", "RANGES", "MERGE"):
        prev = lib.dqrm_set_apply_kernel(getattr(L, "DQRM_APPLY_" + kind))
        try:
            for nxt in ("criteo", "two_per_bag"):
                nb = BATCH[nxt](dq, 51)
                form = lib.dqrm_apply_fwd_form(ts.c, N, cap_total, ws.numel(), nb.c, flags)
                names = _launched(lambda: kern.apply_fwd(cap_base, cap_total, payloads, payloads.shape[1], N, 8, s_avg,
                                                         0.1, L.DQRM_UPD_DP, False, nb, out, workspace=ws))
                print(D, N, kind, nxt, "form:", form, names)
                fin_fwd, fin, fwd = (_has(names, k) for k in ("k_finalize_fwd", "k_table_finalize", "k_emb_fwd"))
                if form == L.DQRM_APPLY_FWD_FIN_FWD:
                    assert fin_fwd and not fin and not fwd, names
                elif form == L.DQRM_APPLY_FWD_ONE_LAUNCH:
                    assert not fin_fwd and not fin and not fwd, names
                else:
                    assert form == L.DQRM_APPLY_FWD_SEPARATE and fwd and not fin_fwd, names
                forms.add(form)
        finally:
            lib.dqrm_set_apply_kernel(prev)
    assert forms == {L.DQRM_APPLY_FWD_SEPARATE, L.DQRM_APPLY_FWD_ONE_LAUNCH, L.DQRM_APPLY_FWD_FIN_FWD}
    assert ts.read_errors() == 0
