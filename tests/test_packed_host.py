"""CPU half of the INT4 packed-row tests: every device case's input generation and reference
run here (cpu_packed.py), and the preconditions that keep test_gpu_packed.py from passing
vacuously are asserted from the references alone."""
import numpy as np
import pytest

import cpu_packed as CP
import oracle as O

f32 = np.float32


# ------------------------------------------------------------------ section 1
@pytest.mark.parametrize("D", CP.FWD_D)
def test_forward_cases_generate_and_have_every_bag_kind(D):
    Ws = CP.fwd_weights(D)
    s = CP.scales_of(Ws)
    assert 257 in CP.fwd_B(D)
    for t, w in enumerate(Ws):
        P = O.pack_int4(w, s[t])
        assert P.shape == (CP.ROWS[t], D // 2)
        assert np.unique(P).size > 4  # the rows hold real nibbles
    for form in CP.FWD_FORMS:
        for B in CP.fwd_B(D):
            idxs, offs, p1 = CP.fwd_batch(form, B, D)
            y = CP.fwd_reference(Ws, idxs, offs, s)
            assert y.shape == (CP.T, B, D) and np.isfinite(y).all()
            for t in range(CP.T):
                lens = CP.bag_lengths(idxs[t], offs[t])
                assert lens.size == B and (lens >= 0).all()
                assert idxs[t].min(initial=0) >= 0 and idxs[t].max(initial=0) < CP.ROWS[t]
                if form != "bags":
                    assert (lens == 1).all()
                    continue
                if B >= 3:  # an empty bag, a bag of one, a bag of at least two; the stated bags
                    assert (lens == 0).any() and (lens == 1).any() and (lens >= 2).any()
                    assert lens[1] == 0 and lens[-1] == 0
                    bag0 = idxs[t][: lens[0]]
                    assert np.unique(bag0).size < bag0.size
                    # an empty bag is a zero row; a clamped sum shows the FP32 path's clamp
                    assert not y[t][1].any() and not y[t][-1].any()
                else:
                    assert lens[0] == 2


def test_forward_bag_sums_reach_the_clamp():
    """Some multi-lookup bag sums leave the 4-bit range: the FP32 path's clamp is exercised."""
    D = 16
    Ws = CP.fwd_weights(D)
    s = CP.scales_of(Ws)
    idxs, offs, _ = CP.fwd_batch("bags", 700, D)
    y = CP.fwd_reference(Ws, idxs, offs, s)
    for t in range(CP.T):
        q = y[t] / s[t]
        assert (np.rint(q) == -8).any() or (np.rint(q) == 7).any()


# ------------------------------------------------------------------ section 2
@pytest.mark.parametrize("form", CP.P2_FORMS)
def test_second_pass_case_generates(form):
    assert CP.P2_B > 256 * ((16384 + CP.P2_T - 1) // CP.P2_T)       # more bags than one pass of the capped grid
    assert CP.P2_B % 256 != 0                                       # the last pass is partial
    assert CP.P2_T * CP.P2_B * CP.P2_D * 4 > (32 << 20)             # above the write-through cut-off
    Ws = CP.pass2_weights()
    s = CP.scales_of(Ws)
    idxs, offs, p1 = CP.pass2_batch(form)
    y = CP.fwd_reference(Ws, idxs, offs, s)
    assert y.shape == (CP.P2_T, CP.P2_B, CP.P2_D)
    if form == "mixed":
        lens = CP.bag_lengths(idxs[0], offs[0])
        assert set(np.unique(lens).tolist()) == {0, 1, 2}
        # bags past the first pass (>= 16384) of every kind
        assert set(np.unique(lens[16384:]).tolist()) == {0, 1, 2}


# ------------------------------------------------------------------ section 3
@pytest.mark.parametrize("form", CP.ERR_FORMS)
def test_error_cases_hold_the_stated_faults(form):
    idxs, offs, p1 = CP.err_batch(form)
    bad_idx = sum(int(((idxs[t] < 0) | (idxs[t] >= CP.ROWS[t])).sum()) for t in range(CP.T))
    dec = sum(int((np.diff(offs[t]) < 0).sum()) for t in range(CP.T))
    if form == "offsets":
        assert bad_idx == 0 and dec == 1
    else:
        assert bad_idx == 4 and dec == 0
    for t in range(CP.T):
        assert offs[t].size == 8 and offs[t][0] == 0 and offs[t].max() <= idxs[t].size
        if form == "multi" and t in (1, 2):  # the faults sit in bags of more than one lookup
            lens = CP.bag_lengths(idxs[t], offs[t])
            bag_of = np.repeat(np.arange(8), lens)
            bad = (idxs[t] < 0) | (idxs[t] >= CP.ROWS[t])
            assert (lens[bag_of[bad]] >= 2).all()


# ------------------------------------------------------------------ section 4
CASES4 = [(f, D, k) for f in CP.FAMILY_KINDS for D in CP.UPD_D for k in CP.FAMILY_KINDS[f]]


@pytest.mark.parametrize("family,D,kind", CASES4)
def test_update_cases_change_nibbles_and_move_one_scale(family, D, kind):
    recs = CP.simulate(family, D, kind)
    assert len(recs) == CP.STEPS
    for step, rec in enumerate(recs):
        frac = CP.nibble_change_fraction(rec)
        assert frac >= 0.01, (step, frac)
        for t in range(CP.T):  # the planted row is never touched
            assert t != CP.PLANT_TABLE or CP.PLANT_ROW not in rec["touched"][t]
        if rec["odd"]:  # the refreshing FP32 forward moved scale[] away from pscale[]
            assert (rec["scale"] != rec["pscale"]).any(), step
        else:
            np.testing.assert_array_equal(rec["scale"], rec["pscale"])
    s0 = CP.scales_of(recs[0]["W_old"])
    s1 = CP.scales_of(recs[-1]["W_new"])
    assert (s0 != s1).any() and (s0 == s1).any()
    assert s0[CP.PLANT_TABLE] == s1[CP.PLANT_TABLE] == O.sym_scale(CP.PLANT[kind], 4)
    if family == "local":  # masked-out tables stay as they were
        for t in range(CP.T):
            if not CP.MASK[t]:
                np.testing.assert_array_equal(recs[-1]["W_new"][t], recs[0]["W_old"][t])


# ------------------------------------------------------------------ section 5
@pytest.mark.parametrize("D", CP.FLAG_D)
def test_flagged_repack_tables_behave_as_stated(D):
    Ws = CP.flag_weights(D)
    s0 = CP.scales_of(Ws)
    idxs, offs, p1, B = CP.flag_batch(D)
    assert B == CP.FLAG_B and p1
    assert CP.FLAG_MOVE_ROW not in idxs[CP.FLAG_MOVE] and CP.FLAG_KEEP_ROW not in idxs[CP.FLAG_KEEP]
    assert CP.PLANT_ROW not in idxs[CP.FLAG_KEEP]
    dy = CP.flag_dy(D)
    for t in range(CP.T):
        O.emb_bwd_sgd(Ws[t], idxs[t], offs[t], dy[t], s0[t], CP.LR)
    s1 = CP.scales_of(Ws)
    assert s1[CP.FLAG_KEEP] == s0[CP.FLAG_KEEP]   # its maximum does not move: rows are kept
    assert s1[CP.FLAG_MOVE] != s0[CP.FLAG_MOVE]   # its maximum moves: the table is repacked
    # the sentinel rows' true bytes exist under both scales (the sentinel is their complement)
    for t, r in ((CP.FLAG_KEEP, CP.FLAG_KEEP_ROW), (CP.FLAG_MOVE, CP.FLAG_MOVE_ROW)):
        assert O.pack_int4(Ws[t][r: r + 1], s1[t]).shape == (1, D // 2)


# ------------------------------------------------------------------ section 6
@pytest.mark.parametrize("D", CP.MOD_D)
def test_module_inputs_generate(D):
    Ws = CP.mod_weights(D)
    assert [w.shape for w in Ws] == [(n, D) for n in CP.ROWS]
    for step in range(CP.MOD_STEPS):
        idxs, offs = CP.mod_batch(step, D)
        g = CP.mod_grad(step, D)
        assert g.shape == (CP.MOD_B, CP.T, D) and g.dtype == f32
        for t in range(CP.T):
            lens = CP.bag_lengths(idxs[t], offs[t])
            assert lens.size == CP.MOD_B
            assert (lens == 1).all() if step % 2 == 0 else ((lens == 0).any() and (lens >= 2).any())
            assert idxs[t].min() >= 0 and idxs[t].max() < CP.ROWS[t]
