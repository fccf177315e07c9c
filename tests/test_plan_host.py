"""CPU characterisation of the embedding step's host layer (csrc/dqrm_kernels.hip): which launch
form dqrm_apply_fwd_form reports for every apply kind, rank count, row length, workspace, next
batch and forward flag, under the environment switches that change it, and the error code and
full dqrm_last_error() text of the faults several exports share. Nothing here touches a device:
the table set and batches hold dummy non-null pointers, as in tests/test_abi.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

import deep_quantized_recommendation_model_dqrm_amd as dq
from deep_quantized_recommendation_model_dqrm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEP, ONE, FIN = L.DQRM_APPLY_FWD_SEPARATE, L.DQRM_APPLY_FWD_ONE_LAUNCH, L.DQRM_APPLY_FWD_FIN_FWD
T, B, CAP = 3, 64, 150

KINDS = {"auto": L.DQRM_APPLY_AUTO, "flat": L.DQRM_APPLY_FLAT, "slot": L.DQRM_APPLY_SLOT,
         "ranges": L.DQRM_APPLY_RANGES, "merge": L.DQRM_APPLY_MERGE}
RANKS = (1, 2, 4, 16, 17)
DIMS = (8, 16, 64)
FLAGS = {"plain": 0, "packed": L.DQRM_FWD_USE_PACKED, "full": L.DQRM_FWD_FULL_PRECISION}
BATCHES = ("criteo", "bags", "empty")

# include/dqrm.h, dqrm_apply_sparse_update_fwd / dqrm_apply_fwd_form. Which kernel takes the apply:
#   MERGE, at most 16 ranks, with the positions workspace (one rank needs none): the merge kernel
#   RANGES: the ranges kernel;  SLOT: the slot kernel;  FLAT, and MERGE otherwise: the flat kernel
#   AUTO: the flat kernel at num_ranks < dim / 4 or one rank, the slot kernel beyond
AUTO_KERNEL = {  # (dim, num_ranks)
    (8, 1): "flat", (8, 2): "slot", (8, 4): "slot", (8, 16): "slot", (8, 17): "slot",
    (16, 1): "flat", (16, 2): "flat", (16, 4): "slot", (16, 16): "slot", (16, 17): "slot",
    (64, 1): "flat", (64, 2): "flat", (64, 4): "flat", (64, 16): "slot", (64, 17): "slot",
}
MERGE_KERNEL = {  # (num_ranks, workspace given)
    (1, False): "merge", (1, True): "merge", (2, False): "flat", (2, True): "merge", (4, False): "flat",
    (4, True): "merge", (16, False): "flat", (16, True): "merge", (17, False): "flat", (17, True): "flat",
}
# ... and the form by kernel, next batch and forward flags (every dim here is >= 8, where
# DQRM_FWD_USE_PACKED without DQRM_FWD_FULL_PRECISION is the packed gather):
#   merge: ONE_LAUNCH for a Criteo-form batch with bags, without DQRM_FWD_USE_PACKED
#   flat:  FIN_FWD for any batch with bags whose forward reads the exact FP32 rows
#   slot, ranges: SEPARATE
FORM = {
    ("merge", "criteo", "plain"): ONE, ("merge", "criteo", "packed"): SEP, ("merge", "criteo", "full"): ONE,
    ("merge", "bags", "plain"): SEP, ("merge", "bags", "packed"): SEP, ("merge", "bags", "full"): SEP,
    ("merge", "empty", "plain"): SEP, ("merge", "empty", "packed"): SEP, ("merge", "empty", "full"): SEP,
    ("flat", "criteo", "plain"): FIN, ("flat", "criteo", "packed"): SEP, ("flat", "criteo", "full"): FIN,
    ("flat", "bags", "plain"): FIN, ("flat", "bags", "packed"): SEP, ("flat", "bags", "full"): FIN,
    ("flat", "empty", "plain"): SEP, ("flat", "empty", "packed"): SEP, ("flat", "empty", "full"): SEP,
}
# the switches, each read once per process (so each in a child): what they turn into SEPARATE,
# and DQRM_APPLY=merge, which makes AUTO the MERGE kind
ENV_CASES = {
    "default": {},
    "DQRM_FIN_FWD=0": {"DQRM_FIN_FWD": "0"},
    "DQRM_FUSED_FWD=0": {"DQRM_FUSED_FWD": "0"},
    "DQRM_FINALIZE=inline": {"DQRM_FINALIZE": "inline"},
    "DQRM_APPLY=merge": {"DQRM_APPLY": "merge"},
}


def expected_form(case, kind, N, D, ws, batch, flags):
    if kind == "auto" and case == "DQRM_APPLY=merge":
        kind = "merge"
    kernel = {"auto": AUTO_KERNEL.get((D, N)), "flat": "flat", "slot": "slot", "ranges": "ranges",
              "merge": MERGE_KERNEL[(N, ws)]}[kind]
    form = FORM.get((kernel, batch, flags), SEP)
    if case in ("DQRM_FIN_FWD=0", "DQRM_FINALIZE=inline") and form == FIN:
        form = SEP
    if case == "DQRM_FUSED_FWD=0" and form == ONE:
        form = SEP
    return form


def dummy_set(D, packed=False):
    ts = L.TableSet()
    ts.num_tables, ts.dim, ts.total_rows, ts.total_blocks, ts.total_sblocks = T, D, 5307, 23, 3
    for k, name in enumerate(("W", "rowmax", "blkmax", "sblkmax", "tmax", "scale", "pscale", "meta", "err",
                              "tflags", "sdirty", "bdirty", "sync")):
        setattr(ts, name, 0x10000 * (k + 1))
    if packed:
        ts.packed = 0xF0000
    return ts


def dummy_batch(form="criteo"):
    num_bags = 0 if form == "empty" else B
    return L.Batch(0x1000, 0x2000, 0x3000, num_bags, 2 * B if form == "bags" else num_bags,
                   0 if form == "bags" else L.DQRM_BATCH_POOLING_ONE, 0)


def form_table(lib, case):
    """{combination: (reported, expected)} over the whole grid, in this process's environment."""
    out = {}
    batches = {f: dummy_batch(f) for f in BATCHES}
    for kind, N, D, ws, batch, flags in itertools.product(KINDS, RANKS, DIMS, (False, True), BATCHES, FLAGS):
        ts = dummy_set(D)
        prev = lib.dqrm_set_apply_kernel(KINDS[kind]) if not (kind == "auto" and case == "DQRM_APPLY=merge") else None
        try:
            ws_bytes = lib.dqrm_apply_workspace_bytes(N, CAP) if ws else 0
            got = lib.dqrm_apply_fwd_form(C.byref(ts), N, CAP, ws_bytes, C.byref(batches[batch]), FLAGS[flags])
            one = lib.dqrm_apply_fwd_is_one_launch(C.byref(ts), N, CAP, ws_bytes, C.byref(batches[batch]), FLAGS[flags])
        finally:
            if prev is not None:
                lib.dqrm_set_apply_kernel(prev)
        assert one == (1 if got == ONE else 0)
        out[(kind, N, D, ws, batch, flags)] = (got, expected_form(case, kind, N, D, ws, batch, flags))
    return out


def check_case(case):
    """Run in a child process with ENV_CASES[case] in the environment."""
    lib = L.load()
    if case == "DQRM_APPLY=merge":  # the variable seeds the kind: nothing has set one yet
        prev = lib.dqrm_set_apply_kernel(L.DQRM_APPLY_MERGE)
        assert prev == L.DQRM_APPLY_MERGE, prev
    table = form_table(lib, case)
    assert len(table) == 5 * 5 * 3 * 2 * 3 * 3
    wrong = {k: v for k, v in table.items() if v[0] != v[1]}
    assert not wrong, (case, len(wrong), sorted(wrong.items())[:8])
    if case == "default":  # every form occurs, so the table tells them apart
        assert {v[0] for v in table.values()} == {SEP, ONE, FIN}
    print("forms ok", case, len(table))


@pytest.fixture(scope="module")
def lib():
    dq.build(verbose=False)
    return L.load()


@pytest.mark.parametrize("case", list(ENV_CASES))
def test_apply_fwd_form_table(lib, case):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQRM_") or k == "DQRM_LIB_PATH"}
    env.update(ENV_CASES[case])
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path)
    r = subprocess.run([sys.executable, "-c", f"import test_plan_host as m; m.check_case({case!r})"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"forms ok {case}" in r.stdout


def test_apply_fwd_form_rejects_bad_arguments(lib):
    ts, nb = dummy_set(16), dummy_batch()
    assert lib.dqrm_apply_fwd_form(None, 1, CAP, 0, C.byref(nb), 0) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"dqrm: null table set"
    assert lib.dqrm_apply_fwd_form(C.byref(ts), 1, CAP, 0, None, 0) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"dqrm_apply_fwd_form: null batch pointer"
    for n in (0, 65):
        assert lib.dqrm_apply_fwd_form(C.byref(ts), n, CAP, 0, C.byref(nb), 0) == L.DQRM_E_INVALID
        assert lib.dqrm_last_error() == b"dqrm_apply_fwd_form: bad ranks (%d)" % n
        assert lib.dqrm_apply_fwd_is_one_launch(C.byref(ts), n, CAP, 0, C.byref(nb), 0) == L.DQRM_E_INVALID


# ---- the shared faults: every export that has one, its code and whole text -------------------
DY, OUT, WS = 0x7000, 0x8000, 0x9000  # 16-byte aligned dummies
SLOT_WS = (0xA000, 0xB000, 0xC000, 0xD000, 0xE000)  # ws_cap_base, rows, vals, ucount, absmax
S_AVG = 0xF000


def _calls(lib, D=16):
    """{export: (the name its shared checks report, call(dy=, repack=, slot_ws=))} -- every other
    argument valid, so that a call fails on the argument under test alone."""
    ts, b, nb = dummy_set(D), dummy_batch(), dummy_batch()
    s, bb, nn = C.byref(ts), C.byref(b), C.byref(nb)
    fwd = (nn, 4, 0, OUT, B * D, D)
    P = lib.dqrm_payload_bytes(T, CAP, D, 8)

    def slot(w, total=None):  # the slot workspace as the local-step exports take it
        return (w[0],) + (() if total is None else (total,)) + tuple(w[1:])

    return {
        "dqrm_emb_bwd_sgd": ("dqrm_emb_bwd_sgd", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                             lib.dqrm_emb_bwd_sgd(s, bb, dy, B * D, D, 1, 0.1, repack, WS, 1 << 20, None)),
        "dqrm_emb_bwd_sgd_fwd": ("dqrm_emb_bwd_sgd_fwd", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                 lib.dqrm_emb_bwd_sgd_fwd(s, bb, dy, B * D, D, 1, 0.1, repack, WS, 1 << 20, *fwd, None)),
        "dqrm_emb_bwd_lookup_grad": ("dqrm_emb_bwd_lookup_grad", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                     lib.dqrm_emb_bwd_lookup_grad(s, bb, dy, B * D, D, 1, 0x100, 0x200, None)),
        "dqrm_emb_bwd_coalesce": ("dqrm_emb_bwd_coalesce", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                  lib.dqrm_emb_bwd_coalesce(s, bb, dy, B * D, D, 1, *slot_ws, WS, 1 << 20, None)),
        "dqrm_emb_bwd_coalesce_scaled": ("dqrm_emb_bwd_coalesce_scaled", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                         lib.dqrm_emb_bwd_coalesce_scaled(s, bb, dy, B * D, D, 1, 2, *slot_ws, WS,
                                                                          1 << 20, None)),
        "dqrm_emb_local_update": ("dqrm_emb_local_update", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                  lib.dqrm_emb_local_update(s, bb, dy, B * D, D, 1, 0.1, None, repack, WS, 1 << 20, None)),
        "dqrm_emb_bwd_apply_local": ("dqrm_emb_bwd_apply_local", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                     lib.dqrm_emb_bwd_apply_local(s, bb, dy, B * D, D, 1, *slot(slot_ws, CAP), 8, S_AVG,
                                                                  0.1, repack, WS, 1 << 20, None)),
        "dqrm_emb_bwd_apply_fwd_local": ("dqrm_emb_bwd_apply_local", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                         lib.dqrm_emb_bwd_apply_fwd_local(s, bb, dy, B * D, D, 1, *slot(slot_ws, CAP), 8,
                                                                          S_AVG, 0.1, repack, WS, 1 << 20, *fwd, None)),
        "dqrm_rows_changed": ("dqrm_rows_changed", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                              lib.dqrm_rows_changed(s, 0x100, 5, repack, None)),
        "dqrm_apply_local": ("dqrm_apply_local", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                             lib.dqrm_apply_local(s, *slot(slot_ws, CAP), 8, S_AVG, 0.1, repack, None)),
        "dqrm_apply_sparse_update": ("dqrm_apply_sparse_update", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                     lib.dqrm_apply_sparse_update(s, 0x100, CAP, 0x200, P, 2, 8, S_AVG, 0.1,
                                                                  L.DQRM_UPD_DP, repack, None)),
        "dqrm_apply_sparse_update_strided": ("dqrm_apply_sparse_update", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                             lib.dqrm_apply_sparse_update_strided(s, 0x100, CAP, 0x200, P, (P + 15) // 16 * 16,
                                                                                  2, 8, S_AVG, 0.1, L.DQRM_UPD_DP,
                                                                                  repack, None)),
        "dqrm_apply_sparse_update_fwd": ("dqrm_apply_sparse_update", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                         lib.dqrm_apply_sparse_update_fwd(s, 0x100, CAP, 0x200, P, (P + 15) // 16 * 16, 2,
                                                                          8, S_AVG, 0.1, L.DQRM_UPD_DP, repack, None,
                                                                          0, *fwd, None)),
        "dqrm_apply_sparse_update_fwd(no next)": ("dqrm_apply_sparse_update", lambda dy=DY, repack=0, slot_ws=SLOT_WS:
                                                  lib.dqrm_apply_sparse_update_fwd(s, 0x100, CAP, 0x200, P,
                                                                                   (P + 15) // 16 * 16, 2, 8, S_AVG, 0.1,
                                                                                   L.DQRM_UPD_DP, repack, None, 0, None,
                                                                                   4, 0, None, 0, 0, None)),
    }


HAS_DY = ("dqrm_emb_bwd_sgd", "dqrm_emb_bwd_sgd_fwd", "dqrm_emb_bwd_lookup_grad", "dqrm_emb_bwd_coalesce",
          "dqrm_emb_bwd_coalesce_scaled", "dqrm_emb_local_update", "dqrm_emb_bwd_apply_local",
          "dqrm_emb_bwd_apply_fwd_local")
HAS_REPACK = ("dqrm_emb_bwd_sgd", "dqrm_emb_bwd_sgd_fwd", "dqrm_rows_changed", "dqrm_emb_local_update",
              "dqrm_apply_sparse_update", "dqrm_apply_sparse_update_strided", "dqrm_apply_sparse_update_fwd",
              "dqrm_apply_sparse_update_fwd(no next)", "dqrm_apply_local", "dqrm_emb_bwd_apply_local",
              "dqrm_emb_bwd_apply_fwd_local")
HAS_SLOT_WS = ("dqrm_emb_bwd_coalesce", "dqrm_emb_bwd_coalesce_scaled", "dqrm_emb_bwd_apply_local",
               "dqrm_emb_bwd_apply_fwd_local")


@pytest.mark.parametrize("name", HAS_DY)
def test_dy_fault_text(lib, name):
    who, call = _calls(lib)[name]
    for dy in (None, DY + 8):  # null, misaligned
        assert call(dy=dy) == L.DQRM_E_INVALID
        assert lib.dqrm_last_error() == b"%s: dy must be 16-B aligned with strides %% 4 == 0" % who.encode()


@pytest.mark.parametrize("name", HAS_REPACK)
def test_repack_fault_text(lib, name):
    who, call = _calls(lib)[name]
    for bits in (4, 8):  # 4 without packed rows, and a width that is never packed
        assert call(repack=bits) == L.DQRM_E_INVALID
        assert lib.dqrm_last_error() == b"%s: repack needs packed rows and bits == 4 (got %d)" % (who.encode(), bits)


@pytest.mark.parametrize("name", HAS_SLOT_WS)
def test_slot_workspace_fault_text(lib, name):
    who, call = _calls(lib)[name]
    for k in range(5):  # each pointer null in turn, then the values misaligned
        ws = list(SLOT_WS)
        ws[k] = None
        assert call(slot_ws=tuple(ws)) == L.DQRM_E_INVALID
        assert lib.dqrm_last_error() == b"%s: null/unaligned workspace" % who.encode()
    ws = list(SLOT_WS)
    ws[2] += 4
    assert call(slot_ws=tuple(ws)) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"%s: null/unaligned workspace" % who.encode()


def test_apply_local_workspace_fault_text(lib):
    """dqrm_apply_local reads the workspace only: it asks for the pointers, not for an alignment."""
    _, call = _calls(lib)["dqrm_apply_local"]
    for k in range(5):
        ws = list(SLOT_WS)
        ws[k] = None
        assert call(slot_ws=tuple(ws)) == L.DQRM_E_INVALID
        assert lib.dqrm_last_error() == b"dqrm_apply_local: null workspace pointer"


def test_fused_forward_is_checked_before_the_update(lib):
    """The exports that also run the next batch's forward reject it under their own name, before
    the update's arguments."""
    calls = _calls(lib)
    ts, b = dummy_set(16), dummy_batch()
    s, bb = C.byref(ts), C.byref(b)
    bad = (bb, 4, 0, OUT + 4, B * 16, 16)  # out misaligned
    assert lib.dqrm_emb_bwd_sgd_fwd(s, bb, None, B * 16, 16, 1, 0.1, 0, WS, 1 << 20, *bad, None) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"dqrm_emb_bwd_sgd_fwd: out must be 16-B aligned with strides % 4 == 0"
    assert lib.dqrm_emb_bwd_apply_fwd_local(s, bb, None, B * 16, 16, 1, SLOT_WS[0], CAP, *SLOT_WS[1:], 8, S_AVG, 0.1, 0,
                                            WS, 1 << 20, *bad, None) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"dqrm_emb_bwd_apply_fwd_local: out must be 16-B aligned with strides % 4 == 0"
    assert lib.dqrm_apply_sparse_update_fwd(s, None, CAP, None, 0, 0, 0, 8, None, 0.1, 0, 0, None, 0, *bad,
                                            None) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"dqrm_apply_sparse_update_fwd: out must be 16-B aligned with strides % 4 == 0"
    assert lib.dqrm_apply_sparse_update_fwd(s, None, CAP, None, 0, 0, 0, 8, None, 0.1, 0, 0, WS + 8, 64, *bad,
                                            None) == L.DQRM_E_INVALID
    assert lib.dqrm_last_error() == b"dqrm_apply_sparse_update_fwd: workspace must be 16-B aligned"
    assert set(calls) >= set(HAS_DY) | set(HAS_REPACK) | set(HAS_SLOT_WS)
