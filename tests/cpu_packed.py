"""TEST INFRASTRUCTURE: inputs and CPU references of the INT4 packed-row tests, shared by
test_gpu_packed.py (the device runs) and test_packed_host.py (the same generation and
references on the CPU, with the preconditions that keep the device cases from being vacuous).
Not collected; never used by the product.

Everything is regenerated from seeds (numpy RandomState) and compared exactly: the references
are oracle.pack_int4 / table_scale / emb_fwd / quantize and numpy.

The update trajectories (section 4) are simulated here with the oracle's update of the same
family, only to state on the CPU that the device cases do something: rows change nibbles, one
table's scale moves and one does not, and scale[] really leaves pscale[] on the odd steps.
The device tests never compare W with these trajectories (W is pinned by test_gpu_parity.py);
they compare `packed` with pack_int4 of the W that is on the device."""
from __future__ import annotations

import numpy as np

import gen_inputs as G
import oracle as O

f32 = np.float32

ROWS = [3, 300, 2304, 20000]
T = len(ROWS)

# ------------------------------------------------------------------ batches
def pool1_batch(rows, B, seed, dist="uniform"):
    """Criteo form: (idx [T, B], offsets arange(B) per table)."""
    P = G.pooling_one(rows, B, seed, dist=dist)
    ar = np.arange(B, dtype=np.int64)
    return [P[t] for t in range(len(rows))], [ar.copy() for _ in rows]


def bag_batch(rows, B, seed, max_len=10):
    """Bags of 0..max_len lookups. B >= 3: bag 0 holds at least three lookups and one row
    twice, bag 1 and the last bag are empty; B >= 5: bag 2 holds one lookup and bag 3 two.
    B == 1: one bag of two lookups of one row."""
    rs = np.random.RandomState(seed)
    idxs, offs = [], []
    for n in rows:
        lens = rs.randint(0, max_len + 1, size=B).astype(np.int64)
        if B >= 3:
            lens[0] = max(int(lens[0]), 3)
            lens[1] = 0
            lens[-1] = 0
        if B >= 5:
            lens[2] = 1
            lens[3] = 2
        if B == 1:
            lens[0] = 2
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        idx = rs.randint(0, n, size=int(lens.sum())).astype(np.int64)
        if lens[0] >= 2:
            idx[lens[0] - 1] = idx[0]
        idxs.append(idx)
        offs.append(off)
    return idxs, offs


def bag_lengths(idx, off):
    return np.diff(np.concatenate([off, [idx.size]]))


def mixed_batch(rows, B, seed):
    """Bag lengths drawn from {0, 1, 2} (section 2's mixed form)."""
    rs = np.random.RandomState(seed)
    idxs, offs = [], []
    for n in rows:
        lens = rs.randint(0, 3, size=B).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        idxs.append(rs.randint(0, n, size=int(lens.sum())).astype(np.int64))
        offs.append(off)
    return idxs, offs


def fwd_reference(Ws, idxs, offs, scales):
    """[T, B, D]: oracle.emb_fwd of every table with its (frozen) scale, 4 bits."""
    return np.stack([O.emb_fwd(Ws[t], idxs[t], offs[t], scales[t], bits=4)[0] for t in range(len(Ws))])


def scales_of(Ws):
    return np.array([O.table_scale(w, 4) for w in Ws], dtype=f32)


# ------------------------------------------------------------------ section 1
FWD_D = [4, 8, 16, 32, 64, 128, 256]
FWD_FORMS = ["pool1", "ones", "bags"]


def fwd_B(D):
    """The bag counts of a width: 255 / 256 / 257 straddle the packed kernel's 256-bag pass;
    D >= 128 keeps 1, 257 (two passes' worth of chunks, the second of one bag) and 700."""
    return [1, 255, 256, 257, 700] if D < 128 else [1, 257, 700]


def fwd_weights(D):
    return G.table_weights(ROWS, D, 900 + D)


def fwd_batch(form, B, D):
    """(idxs, offs, pooling_one flag). "ones" is the pool1 data as a general batch."""
    seed = 7 * D + B
    if form == "bags":
        idxs, offs = bag_batch(ROWS, B, seed)
        return idxs, offs, False
    idxs, offs = pool1_batch(ROWS, B, seed)
    return idxs, offs, form == "pool1"


# ------------------------------------------------------------------ section 2
P2_T, P2_D, P2_B = 256, 8, 16384 + 257
P2_ROWS = [3 + (t % 3) for t in range(P2_T)]
P2_FORMS = ["pool1", "mixed"]


def pass2_weights():
    return G.table_weights(P2_ROWS, P2_D, 4242)


def pass2_batch(form):
    if form == "pool1":
        idxs, offs = pool1_batch(P2_ROWS, P2_B, 4243)
        return idxs, offs, True
    idxs, offs = mixed_batch(P2_ROWS, P2_B, 4244)
    return idxs, offs, False


# ------------------------------------------------------------------ section 3
ERR_D = [16, 64]
ERR_FORMS = ["single", "multi", "offsets", "pool1"]


def err_batch(form):
    """8 bags per table; every fault is one the kernels bounds-check and flag.
    single: an index == num_rows and a negative index, each in a bag of one (tables 0, 3);
    multi: the same inside bags of three and two (tables 1, 2); offsets: a decreasing offset
    (table 2); pool1: the single faults in a Criteo-form batch."""
    B = 8
    ar = np.arange(B, dtype=np.int64)
    idxs = [np.array([0, 1, 2, 1, 0, 2, 1, 0], np.int64), np.array([5, 299, 0, 17, 100, 250, 3, 9], np.int64),
            np.array([7, 2303, 0, 1000, 10, 11, 12, 13], np.int64),
            np.array([19999, 0, 5, 12345, 6, 7, 8, 9], np.int64)]
    offs = [ar.copy() for _ in range(T)]
    if form in ("single", "pool1"):
        idxs[0][3] = 3
        idxs[0][6] = -1
        idxs[3][0] = 20000
        idxs[3][7] = -7
    elif form == "multi":
        idxs[1] = np.array([5, 300, 7, 8, -5, 9, 10, 11, 12, 13, 14], np.int64)
        offs[1] = np.array([0, 3, 5, 6, 7, 8, 9, 10], np.int64)
        idxs[2] = np.array([1, 2, 2304, 3, 4, -1, 5, 6, 7, 8, 9], np.int64)
        offs[2] = np.array([0, 1, 3, 4, 6, 8, 9, 10], np.int64)
    elif form == "offsets":
        offs[2] = np.array([0, 2, 1, 3, 4, 5, 6, 7], np.int64)
    return idxs, offs, form == "pool1"


# ------------------------------------------------------------------ section 4
UPD_D = [8, 16, 64, 256]
BATCH_KINDS = ["p96", "zipf1024", "uni700", "bags130"]
LR = 0.5
DY_SCALE = 30.0
STEPS = 3
# Table 2 keeps its scale: one row that no batch touches holds an element no update reaches
# (a row touched k times moves by about 0.75 * sqrt(k) per element; the Zipf batches put
# hundreds of lookups on a table's first and last rows).
PLANT_TABLE = 2
PLANT_ROW = ROWS[PLANT_TABLE] // 2
PLANT = {"p96": 16.0, "zipf1024": 1000.0, "uni700": 16.0, "bags130": 16.0}
MASK = [1, 0, 1, 0]  # local_update's table_mask: tables 1 and 3 are left out
# update family -> the batch kinds it runs on. The apply kernels of the two-rank exchange
# read payloads (rows and integers), not batches: the small batch (every row of the 3-row
# table from both ranks) and the Zipf batch (many rows that both ranks send) cover them.
FAMILY_KINDS = {"sgd": BATCH_KINDS, "local": BATCH_KINDS, "write": BATCH_KINDS, "dp1": BATCH_KINDS,
                "dp2": ["p96", "zipf1024"], "fp32_2": ["p96", "zipf1024"], "simdp": BATCH_KINDS}
FAMILY_RANKS = {"sgd": 1, "local": 1, "write": 1, "dp1": 1, "dp2": 2, "fp32_2": 2, "simdp": 2}


def upd_weights(D, kind):
    Ws = G.table_weights(ROWS, D, 700 + D)
    Ws[PLANT_TABLE][PLANT_ROW, D // 2] = f32(PLANT[kind])
    return Ws


def upd_batch(kind, seed):
    """(idxs, offs, pooling_one flag, B) of one batch of a kind; the planted row is never looked up."""
    if kind == "bags130":
        idxs, offs = bag_batch(ROWS, 130, seed)
        p1, B = False, 130
    else:
        B, dist = {"p96": (96, "uniform"), "zipf1024": (1024, "zipf"), "uni700": (700, "uniform")}[kind]
        idxs, offs = pool1_batch(ROWS, B, seed, dist=dist)
        p1 = True
    x = idxs[PLANT_TABLE]
    x[x == PLANT_ROW] = PLANT_ROW - 1
    return idxs, offs, p1, B


def upd_dy(B, D, seed):
    return (G.upstream_grad(T, B, D, seed) * f32(DY_SCALE)).astype(f32)


def upd_step_inputs(kind, D, step, ranks=1):
    """Per rank (or micro-step) r: ((idxs, offs, p1, B), dy [T, B, D]) of one step."""
    out = []
    for r in range(ranks):
        b = upd_batch(kind, 5000 + 100 * step + 10 * r + D)
        out.append((b, upd_dy(b[3], D, 6000 + 100 * step + 10 * r + D)))
    return out


def fresh_batch(kind, D, step):
    """The batch of the forward after an even step (and the next batch of the fused calls)."""
    return upd_batch(kind, 8000 + 100 * step + D)


def write_delta(n, D, seed):
    """The torch write of the rows_changed case: W[rows] += delta on the batch's distinct rows."""
    return (np.random.RandomState(seed).standard_normal((n, D)) * 0.75).astype(f32)


def touched_rows(idxs, n):
    """Distinct valid rows of one table's lookups, ascending."""
    u = np.unique(idxs)
    return u[(u >= 0) & (u < n)]


def _simdp_table(W, n, micro, t, s_fwd, lr):
    """sgd_quantized_gradients.py:76-85,366-371 for one table: every micro-step's coalesced
    gradient quantized with the FIRST micro-step's scale, summed, W += -lr * (buf * (s / N))."""
    N = len(micro)
    cos = [O.emb_bwd_coalesce(n, b[0][t], b[1][t], dy[t], s_fwd) for b, dy in micro]
    s = O.grad_scale(cos[0][1], 8)
    buf: dict = {}
    for rows, vals, _ in cos:
        q = O.quantize(vals, s, 8)
        for r, v in zip(rows.tolist(), q):
            buf[r] = (buf[r] + v).astype(f32) if r in buf else v.copy()
    rows = np.array(sorted(buf), dtype=np.int64)
    if rows.size:
        O.simulated_dp_apply(W, rows, np.stack([buf[r] for r in rows.tolist()]), s, N, lr)


def apply_family(family, Ws, inputs, scale, D, step):
    """One update of `family` on the CPU, in place on Ws, with the forward scales `scale`."""
    (b0, dy0) = inputs[0]
    if family == "sgd":
        for t in range(T):
            O.emb_bwd_sgd(Ws[t], b0[0][t], b0[1][t], dy0[t], scale[t], LR)
    elif family == "local":
        for t in range(T):
            if MASK[t]:
                O.emb_local_update(Ws[t], b0[0][t], b0[1][t], dy0[t], scale[t], LR)
    elif family == "write":
        for t in range(T):
            u = touched_rows(b0[0][t], ROWS[t])
            Ws[t][u] = (Ws[t][u] + write_delta(u.size, D, 9000 + 10 * step + t)).astype(f32)
    elif family in ("dp1", "dp2", "fp32_2"):
        O.dp_step(Ws, [[(b[0][t], b[1][t]) for t in range(T)] for b, _ in inputs],
                  [[dy[t] for t in range(T)] for _, dy in inputs], list(scale), LR,
                  grad_bits=32 if family == "fp32_2" else 8)
    elif family == "simdp":
        for t in range(T):
            _simdp_table(Ws[t], ROWS[t], inputs, t, scale[t], LR)
    else:
        raise ValueError(family)


def simulate(family, D, kind):
    """The CPU trajectory of one section 4 case. Per step a dict: scale (the forward scales
    the update's STE uses), pscale (the scales the rows are packed with), W_old / W_new,
    touched (per table, the rows the update may write), odd."""
    Ws = upd_weights(D, kind)
    pscale = scales_of(Ws)
    out = []
    for step in range(STEPS):
        odd = step % 2 == 1
        scale = scales_of(Ws)  # odd: the refreshing FP32 forward; even: refresh_scale_and_pack
        if not odd:
            pscale = scale.copy()
        inputs = upd_step_inputs(kind, D, step, FAMILY_RANKS[family])
        W_old = [w.copy() for w in Ws]
        apply_family(family, Ws, inputs, scale, D, step)
        touched = []
        for t in range(T):
            if family == "local" and not MASK[t]:
                touched.append(np.empty(0, np.int64))
            else:
                touched.append(touched_rows(np.concatenate([b[0][t] for b, _ in inputs]), ROWS[t]))
        out.append(dict(scale=scale, pscale=pscale.copy(), W_old=W_old, W_new=[w.copy() for w in Ws],
                        touched=touched, odd=odd))
    return out


def nibble_change_fraction(rec):
    """Share of a step's touched rows whose packed bytes (with the step's pscale) change."""
    n = c = 0
    for t in range(T):
        u = rec["touched"][t]
        if u.size == 0:
            continue
        a = O.pack_int4(rec["W_old"][t][u], rec["pscale"][t])
        b = O.pack_int4(rec["W_new"][t][u], rec["pscale"][t])
        n += u.size
        c += int((a != b).any(axis=1).sum())
    return c / max(n, 1)


# ------------------------------------------------------------------ section 5
FLAG_D = [8, 64, 256]
FLAG_KEEP, FLAG_MOVE = PLANT_TABLE, 0   # the table whose scale stays / moves
FLAG_KEEP_ROW, FLAG_MOVE_ROW = 5, 2     # packed rows that get the sentinel; not in the batch
FLAG_B = 96


def flag_weights(D):
    return upd_weights(D, "p96")


def flag_batch(D):
    """A Criteo-form batch that leaves row 2 of the 3-row table, row 5 of table 2 and the
    planted row alone."""
    idxs, offs, p1, B = upd_batch("p96", 3100 + D)
    idxs[FLAG_MOVE] = idxs[FLAG_MOVE] % 2
    x = idxs[FLAG_KEEP]
    x[x == FLAG_KEEP_ROW] = FLAG_KEEP_ROW + 1
    return idxs, offs, p1, B


def flag_dy(D):
    return upd_dy(FLAG_B, D, 3200 + D)


# ------------------------------------------------------------------ section 6
MOD_D = [16, 64]
MOD_MODES = ["fused_sgd", "sparse", "dp"]
MOD_KINDS = ["collection", "list"]
MOD_STEPS = 4
MOD_B = 64
MOD_LR = 0.1


def mod_weights(D):
    return G.table_weights(ROWS, D, 300 + D)


def mod_batch(step, D):
    """Even steps the Criteo form, odd steps bags; (idxs, offs)."""
    if step % 2 == 0:
        return pool1_batch(ROWS, MOD_B, 3300 + step + D)
    return bag_batch(ROWS, MOD_B, 3300 + step + D)


def mod_grad(step, D):
    """The upstream gradient of step `step`, [B, T, D]."""
    return np.ascontiguousarray((G.upstream_grad(T, MOD_B, D, 3400 + step + D) * f32(10)).transpose(1, 0, 2))
