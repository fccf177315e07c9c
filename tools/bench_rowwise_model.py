#!/usr/bin/env python3
"""Inference of a whole DLRM from row-wise quantized tables, five forms in one process on one GPU,
on one DQRMNet per case:

  (a) fp32       ``model.predict`` on the FP32 tables (dqrm_model_fwd), as before quantize_embedding;
  (b) composed4  what a user could write before ``DQRMNet.quantize_embedding`` existed: 26 per-table
      composed8  ``embedding_bag_{4bit,byte}_rowwise_offsets`` calls, ``torch.stack`` into the [B, T, D]
                 slab, then ``bot_stack``, ``interact``, ``top_stack`` under no_grad;
  (c) q4         ``model.predict`` after ``quantize_embedding(4)`` (dqrm_model_fwd_rowwise);
  (d) q8         ``model.predict`` after ``quantize_embedding(8)``.

Cases: the Kaggle and Terabyte MLPs of workloads.MLPS with their 26 tables (rows capped at 500 k per
table; D = 16 / 64), B = 2048 and 16384 (the reference's --test-mini-batch-size), weight_bit = 4,
per_channel, plain interaction, Criteo-form batches, stacks fresh. Every form alternates between the
same two batches. Device events around `--iters` predicts, `--repeats` windows per form, the forms
alternating, medians; `--runs` runs of that per invocation; the summary quotes the median over the
runs and every window-by-window ratio. Acceptance: q4 <= composed4 and q8 <= composed8 in the median
of the alternating windows, for every case (composed is existing code: the baseline). q4 against
fp32 is reported, not gated. Kernels per predict are counted by torch.profiler in a pass of its own
and compared with dqrm_model_fwd_rowwise_launches. The device error words are read at the end.

The embedding launch's own time comes from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o rw --output-format csv -- \\
        python tools/bench_rowwise_model.py --trace-only CASE
    python tools/bench_rowwise_model.py --merge-kernel-stats CASE=DIR/.../rw_kernel_stats.csv [...]
(the second adds the kernels' average times to the JSON written before).

usage: python tools/bench_rowwise_model.py [--iters 100] [--repeats 5] [--runs 3] [--out profiles/rowwise_model.json]
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_quantized_recommendation_model_dqrm_amd as dq  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd import quantized_ops as Q  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd.workloads import CONFIGS, MLPS, synthetic_indices  # noqa: E402

ROW_CAP = 500_000
CASES = [(name, B) for name in ("kaggle", "terabyte") for B in (2048, 16384)]
FORMS = ("fp32", "composed4", "composed8", "q4", "q8")
BAG_OP = {4: Q.embedding_bag_4bit_rowwise_offsets, 8: Q.embedding_bag_byte_rowwise_offsets}


class Case:
    def __init__(self, name, B):
        rows, D = CONFIGS[name]
        rows = [min(n, ROW_CAP) for n in rows]
        bot, top = MLPS[name]
        np.random.seed(7)
        self.model = m = dq.DQRMNet(rows, D, bot, top, per_channel=True, weight_bit=4, device="cuda")
        self.T, self.B = len(rows), B
        g = torch.Generator(device="cuda").manual_seed(3)
        self.x = torch.rand(B, bot[0], device="cuda", generator=g)
        idx = [synthetic_indices(rows, B, seed, device="cuda") for seed in (11, 12)]
        self.batches = [dq.LookupBatch.pooling_one(i) for i in idx]
        self.per_table = [[i[t].contiguous() for t in range(self.T)] for i in idx]  # (b)'s inputs, made once
        self.off = torch.arange(B, dtype=torch.int64, device="cuda")
        self.sets = {bits: dq.RowwiseTableSet.from_tables(m.tables, bits) for bits in (4, 8)}
        self.fp32_bytes = m.tables.W.numel() * 4
        m.requantize()
        self.k = 0
        self.layers = len(bot) - 1 + len(top) - 1

    def use(self, form):
        """Point the model at the form's tables (outside the timed windows)."""
        m = self.model
        if form.startswith("q"):
            bits = int(form[1:])
            m.emb_q, m.quantize_emb, m.quantize_bits = self.sets[bits], True, bits
        else:
            m.dequantize_embedding()

    def step(self, form):
        m, k = self.model, self.k
        self.k = 1 - k
        if not form.startswith("composed"):
            return m.predict(self.x, self.batches[k])
        bits = int(form[len("composed"):])
        q, op, off = self.sets[bits], BAG_OP[bits], self.off
        with torch.no_grad():
            slab = torch.stack([op(q.table_packed(t), i, off, check=False) for t, i in enumerate(self.per_table[k])],
                               dim=1)
            return m.top_stack(m.interact(m.bot_stack(self.x), slab))

    def expected_launches(self, form):
        """libdqrm's launches, fresh stacks, plain interaction, no labels: embedding + L layers + the
        interaction; the composed form launches one gather per table (torch.stack's copy comes on top)."""
        if form.startswith("q"):
            self.use(form)
            return self.model.fwd_rowwise_launches(self.batches[0], labels=False, fresh=True)
        return (1 if form == "fp32" else self.T) + self.layers + 1

    def errors(self):
        e = {"tables": self.model.tables.read_errors()}
        for bits, s in self.sets.items():
            e[f"rowwise{bits}"] = s.read_errors()
        e["per_table_ops"] = int(Q._err_word(torch.device("cuda", torch.cuda.current_device())).item())
        return e


def window(case, form, iters):
    case.use(form)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        case.step(form)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def launches(case, form):
    """Device kernels of one predict (torch.profiler); None if the profiler reports none."""
    from torch.profiler import ProfilerActivity, profile

    case.use(form)
    for _ in range(2):
        case.step(form)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        case.step(form)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
    return (len(kernels) or None), len(names) - len(kernels)


def one_run(iters, repeats, cases):
    results = []
    for name, B in cases:
        c = Case(name, B)
        for form in FORMS:
            c.use(form)
            for _ in range(10):
                c.step(form)
        torch.cuda.synchronize()
        t = {f: [] for f in FORMS}
        for _ in range(repeats):
            for f in FORMS:
                t[f].append(window(c, f, iters))
        r = {"case": f"{name}-{B}", "mlp_bot": MLPS[name][0], "mlp_top": MLPS[name][1], "B": B, "tables": c.T,
             "dim": CONFIGS[name][1], "row_cap": ROW_CAP, "iters": iters, "repeats": repeats,
             "resident_bytes": {"fp32": c.fp32_bytes, "rowwise4": c.sets[4].nbytes, "rowwise8": c.sets[8].nbytes}}
        for f in FORMS:
            r[f + "_us_per_predict"] = round(statistics.median(t[f]), 1)
            r[f + "_us_windows"] = [round(v, 1) for v in t[f]]
        for a, b in (("q4", "composed4"), ("q8", "composed8"), ("q4", "fp32"), ("q8", "fp32")):
            r[f"window_ratios_{a}_over_{b}"] = [round(x / y, 3) for x, y in zip(t[a], t[b])]
        for f in FORMS:
            want = c.expected_launches(f)
            try:
                got, copies = launches(c, f)
            except Exception as e:  # the counts are bookkeeping; the timings stand without them
                print(f"launch count unavailable: {e}", file=sys.stderr)
                got = copies = None
            r[f + "_launches_profiled"], r[f + "_launches_expected"] = got, want
            r[f + "_memsets_and_copies_profiled"] = copies
        r["device_errors"] = c.errors()
        results.append(r)
        print(json.dumps(r), flush=True)
        del c
        torch.cuda.empty_cache()
    return results


def summarise(runs, cases):
    out = []
    for k, (name, B) in enumerate(cases):
        row = {"case": f"{name}-{B}", "resident_bytes": runs[-1]["results"][k]["resident_bytes"]}
        med = {}
        for f in FORMS:
            v = [r["results"][k][f + "_us_per_predict"] for r in runs]
            row[f + "_us_runs"], row[f + "_us"] = v, statistics.median(v)
            med[f] = statistics.median(v)
            row[f + "_launches_profiled"] = runs[-1]["results"][k][f + "_launches_profiled"]
            row[f + "_launches_expected"] = runs[-1]["results"][k][f + "_launches_expected"]
        for a, b in (("q4", "composed4"), ("q8", "composed8"), ("q4", "fp32"), ("q8", "fp32")):
            row[f"{a}_over_{b}"] = round(med[a] / med[b], 3)
            row[f"window_ratios_{a}_over_{b}"] = [r["results"][k][f"window_ratios_{a}_over_{b}"] for r in runs]
        row["accepted_q_not_slower_than_composed"] = med["q4"] <= med["composed4"] and med["q8"] <= med["composed8"]
        row["device_errors"] = [r["results"][k]["device_errors"] for r in runs]
        out.append(row)
    return out


def trace_only(case_name, iters):
    """The three one-call forms, `iters` predicts each, for a kernel trace (no timing here)."""
    (name, B), = [c for c in CASES if f"{c[0]}-{c[1]}" == case_name]
    c = Case(name, B)
    for form in ("fp32", "q4", "q8"):
        c.use(form)
        for _ in range(iters):
            c.step(form)
    torch.cuda.synchronize()
    print(json.dumps({"case": case_name, "device_errors": c.errors()}))


def merge_kernel_stats(out, specs):
    """Average time of the embedding kernels (k_emb_fwd: fp32; k_rowwise_bag_set<4 / 8, ...>) from
    rocprofv3's kernel_stats.csv of a --trace-only run, into the summary rows of `out`."""
    with open(out) as f:
        doc = json.load(f)
    for spec in specs:
        case, path = spec.split("=", 1)
        emb = {}
        for r in csv.DictReader(open(path)):
            n = r["Name"]
            if "k_rowwise_bag_set<" in n:
                key = "rowwise" + n.split("k_rowwise_bag_set<", 1)[1].split(",")[0].strip()
            elif "k_emb_fwd<" in n:
                key = "fp32"
            else:
                continue
            emb[key] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                        "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        for row in doc["summary"]:
            if row["case"] == case:
                row["embedding_launch_kernel_trace"] = emb
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for row in doc["summary"]:
        print(json.dumps({"case": row["case"], "embedding_launch_kernel_trace": row.get("embedding_launch_kernel_trace")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default=None, help="comma-separated subset, e.g. kaggle-2048,terabyte-16384")
    ap.add_argument("--trace-only", default=None, metavar="CASE", help="run CASE's one-call forms under a profiler")
    ap.add_argument("--merge-kernel-stats", nargs="+", default=None, metavar="CASE=CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rowwise_model.json"))
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.out, args.merge_kernel_stats)
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowwise_model.py measures on a GPU; none found")
    dq.build(verbose=False)
    if args.trace_only:
        return trace_only(args.trace_only, args.iters)
    cases = CASES if not args.cases else [c for c in CASES if f"{c[0]}-{c[1]}" in args.cases.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
           "forms": {"fp32": "DQRMNet.predict on the FP32 tables (dqrm_model_fwd)",
                     "composed4": "26 x embedding_bag_4bit_rowwise_offsets + torch.stack + bot_stack, interact, top_stack",
                     "composed8": "26 x embedding_bag_byte_rowwise_offsets + torch.stack + bot_stack, interact, top_stack",
                     "q4": "DQRMNet.predict after quantize_embedding(4) (dqrm_model_fwd_rowwise)",
                     "q8": "DQRMNet.predict after quantize_embedding(8) (dqrm_model_fwd_rowwise)"},
           "runs": [{"results": one_run(args.iters, args.repeats, cases)} for _ in range(args.runs)]}
    doc["summary"] = summarise(doc["runs"], cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for row in doc["summary"]:
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
