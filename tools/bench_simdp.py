#!/usr/bin/env python3
"""What simulated data parallelism costs on one DQRMNet, one process, one GPU:

  plain    ``train_step(update=False)`` alone: the forward and backward a micro-step starts with
           (existing code: the baseline);
  micro    ``micro_step``: plain + the tables' coalesce and quantize-pack + ONE
           dqrm_dense_ec_accumulate for both stacks;
  step     ``train_step`` with its update (existing code), so step - plain is one step's update;
  apply    ``apply_micro_steps(lr, N)`` after N untimed micro-steps (the tables' DQRM_UPD_SIMULATED
           apply, ONE dqrm_dense_sim_update, the zeroing, the requantization).

Cases: the Kaggle and Terabyte MLPs of workloads.MLPS with their 26 tables (rows capped at 500 k per
table), B = 128 and 2048, N = 4, weight_bit = 4, per_channel, Criteo-form batches. plain, micro and
step: device events around `--iters` calls, `--repeats` windows per form, the forms alternating,
medians. apply: device events around each of `--applies` calls, median. Nothing is gated: the
numbers are written to the JSON as measured.

The kernels' own times come from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -o sd --output-format csv -- \\
        python tools/bench_simdp.py --trace-only CASE
    python tools/bench_simdp.py --merge-kernel-stats CASE=DIR/.../sd_kernel_stats.csv [...]

usage: python tools/bench_simdp.py [--iters 50] [--repeats 4] [--applies 50] [--out profiles/simdp.json]
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
from deep_quantized_recommendation_model_dqrm_amd.workloads import CONFIGS, MLPS, synthetic_indices  # noqa: E402

ROW_CAP = 500_000
N = 4
LR = 0.1
CASES = [(name, B) for name in ("kaggle", "terabyte") for B in (128, 2048)]
FORMS = ("plain", "micro", "step")
TRACED = ("k_dense_ec_accumulate", "k_dense_sim_update")


class Case:
    def __init__(self, name, B):
        rows, D = CONFIGS[name]
        rows = [min(n, ROW_CAP) for n in rows]
        bot, top = MLPS[name]
        np.random.seed(7)
        self.model = dq.DQRMNet(rows, D, bot, top, per_channel=True, weight_bit=4, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(3)
        self.x = torch.rand(B, bot[0], device="cuda", generator=g)
        self.t = (torch.rand(B, device="cuda", generator=g) < 0.5).float()
        self.batches = [dq.LookupBatch.pooling_one(synthetic_indices(rows, B, seed, device="cuda")) for seed in (11, 12)]
        self.k = 0
        self.mlp_params = sum(p.numel() for l in (self.model.bot_l, self.model.top_l) for p in l.parameters())

    def call(self, form):
        m, k = self.model, self.k
        self.k = 1 - k
        if form == "plain":
            return m.train_step(self.x, self.batches[k], self.t, LR, update=False)
        if form == "step":
            return m.train_step(self.x, self.batches[k], self.t, LR)
        return m.micro_step(self.x, self.batches[k], self.t, N)

    def drain(self):
        """Empty the buffers the micro windows filled (outside every timed window)."""
        n = len(self.model._sim_emb.payloads) if self.model._sim_emb is not None else 0
        if n:
            self.model.apply_micro_steps(LR, n)


def window(case, form, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        case.call(form)
    e1.record()
    torch.cuda.synchronize()
    if form == "micro":
        case.drain()
    return e0.elapsed_time(e1) * 1e3 / iters


def apply_times(case, applies):
    out = []
    for _ in range(applies):
        for _ in range(N):
            case.call("micro")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        case.model.apply_micro_steps(LR, N)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def run(iters, repeats, applies, cases):
    results = []
    for name, B in cases:
        c = Case(name, B)
        for f in FORMS:
            for _ in range(5):
                c.call(f)
            c.drain()
        apply_times(c, 3)
        t = {f: [] for f in FORMS}
        for _ in range(repeats):
            for f in FORMS:
                t[f].append(window(c, f, iters))
        ap = apply_times(c, applies)
        med = {f: statistics.median(t[f]) for f in FORMS}
        r = {"case": f"{name}-{B}", "mlp_bot": MLPS[name][0], "mlp_top": MLPS[name][1], "mlp_params": c.mlp_params,
             "B": B, "N": N, "row_cap": ROW_CAP, "iters": iters, "repeats": repeats, "applies": applies,
             "calls_per_form": iters * repeats}
        for f in FORMS:
            r[f + "_us"] = round(med[f], 1)
            r[f + "_us_windows"] = [round(v, 1) for v in t[f]]
        r["micro_minus_plain_us"] = round(med["micro"] - med["plain"], 1)
        r["window_diffs_micro_minus_plain_us"] = [round(a - b, 1) for a, b in zip(t["micro"], t["plain"])]
        r["step_update_us"] = round(med["step"] - med["plain"], 1)
        r["apply_us"] = round(statistics.median(ap), 1)
        r["apply_us_min_max"] = [round(min(ap), 1), round(max(ap), 1)]
        r["device_errors"] = c.model.tables.read_errors()
        results.append(r)
        print(json.dumps(r), flush=True)
        del c
        torch.cuda.empty_cache()
    return results


def trace_only(case_name, iters):
    (name, B), = [c for c in CASES if f"{c[0]}-{c[1]}" == case_name]
    c = Case(name, B)
    for _ in range(iters):
        for _ in range(N):
            c.call("micro")
        c.model.apply_micro_steps(LR, N)
    torch.cuda.synchronize()
    print(json.dumps({"case": case_name, "device_errors": c.model.tables.read_errors()}))


def merge_kernel_stats(out, specs):
    with open(out) as f:
        doc = json.load(f)
    for spec in specs:
        case, path = spec.split("=", 1)
        ks = {}
        for r in csv.DictReader(open(path)):
            for k in TRACED:
                if k in r["Name"]:
                    ks[k] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                             "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
        for row in doc["results"]:
            if row["case"] == case:
                row["kernel_trace"] = ks
                print(json.dumps({"case": case, "kernel_trace": ks}))
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--applies", type=int, default=50)
    ap.add_argument("--cases", default=None, help="comma-separated subset, e.g. kaggle-128,terabyte-2048")
    ap.add_argument("--trace-only", default=None, metavar="CASE")
    ap.add_argument("--merge-kernel-stats", nargs="+", default=None, metavar="CASE=CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simdp.json"))
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.out, args.merge_kernel_stats)
    if not torch.cuda.is_available():
        raise SystemExit("bench_simdp.py measures on a GPU; none found")
    dq.build(verbose=False)
    if args.trace_only:
        return trace_only(args.trace_only, args.iters)
    cases = CASES if not args.cases else [c for c in CASES if f"{c[0]}-{c[1]}" in args.cases.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
           "forms": {"plain": "DQRMNet.train_step(update=False)", "micro": "DQRMNet.micro_step",
                     "step": "DQRMNet.train_step", "apply": f"DQRMNet.apply_micro_steps(lr, {N}), requantize=True"},
           "results": run(args.iters, args.repeats, args.applies, cases)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
