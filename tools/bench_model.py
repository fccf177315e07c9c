#!/usr/bin/env python3
"""A whole DLRM training step, three forms in one process on one GPU, on one DQRMNet per case:

  (a) the composed modules under autograd: ``model(x, batch)``, ``model.loss``, ``backward()``,
      ``tables.backward_sgd`` and ``sgd_step`` on both stacks -- what a user could write before
      ``train_step`` existed;
  (b) ``model.train_step(x, batch, labels, lr)``: one host call (dqrm_model_step);
  (c) ``train_step(..., next_batch=...)``: the next batch's embedding forward behind the update.

Cases: the Kaggle and Terabyte MLPs of workloads.MLPS with their 26 tables (rows capped at 500 k
per table so that four models fit beside each other's initialisation; D = 16 / 64), B = 128 and
2048, weight_bit = 4, per_channel, plain interaction, BCE, Criteo-form batches. Every form
alternates between the same two batches. Device events around `--iters` steps, `--repeats` windows
per form, the forms alternating, medians; `--runs` runs of that per invocation; the summary quotes
the median over the runs and every window-by-window ratio. Launches per step are counted by
torch.profiler over one step, in a pass of its own, and compared with dqrm_model_step_launches.

``--quantize-activation``: the same cases and protocol on ``DQRMNet(quantize_activation=True)``
(per tensor, as that mode's stacks of several layers must be): (a) is then quant_input, the
integer-activation stacks and quant_feature_outputs composed under autograd, (b) and (c) are
dqrm_model_step_qact, counted against dqrm_model_qact_step_launches, and a fourth form,
``composed_layers``, is what a user could write before MLPStack took such stacks: the same modules
with ``apply_mlp`` over the layers (every layer re-quantizes on every forward) and
``torch.optim.SGD`` on the MLP parameters; the default output file is
profiles/model_step_qact.json.

usage: python tools/bench_model.py [--iters 200] [--repeats 5] [--runs 3] [--quantize-activation]
                                   [--out profiles/model_step.json]
"""
import argparse
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

LR = 1e-3  # small: the same two batches every step, thousands of steps
ROW_CAP = 500_000
CASES = [(name, B) for name in ("kaggle", "terabyte") for B in (128, 2048)]
FORMS = ("composed", "train_step", "train_step_next")
QACT_FORMS = FORMS + ("composed_layers",)


class Case:
    def __init__(self, name, B, qact=False):
        rows, D = CONFIGS[name]
        rows = [min(n, ROW_CAP) for n in rows]
        bot, top = MLPS[name]
        np.random.seed(7)
        self.qact = qact
        self.model = m = dq.DQRMNet(rows, D, bot, top, per_channel=not qact, weight_bit=4, quantize_activation=qact,
                                    device="cuda")
        g = torch.Generator(device="cuda").manual_seed(3)
        self.x = torch.rand(B, bot[0], device="cuda", generator=g)
        self.t = (torch.rand(B, device="cuda", generator=g) < 0.5).float()
        self.batches = [dq.LookupBatch.pooling_one(synthetic_indices(rows, B, seed, device="cuda")) for seed in (11, 12)]
        self.params = list(m.bot_l.parameters()) + list(m.top_l.parameters())
        self.k = 0
        self.layers = len(bot) - 1 + len(top) - 1
        self.opt = torch.optim.SGD(self.params, lr=LR) if qact else None

    def step(self, form):
        m, cur, nxt = self.model, self.batches[self.k], self.batches[1 - self.k]
        self.k = 1 - self.k
        if form == "composed":
            for p in self.params:
                p.grad = None
            E = m.loss(m(self.x, cur), self.t)
            E.backward()
            m.tables.backward_sgd(cur, m.emb_out.grad, LR, ste=True, layout="btd")
            m.bot_stack.sgd_step(LR)
            m.top_stack.sgd_step(LR)
            return E
        if form == "composed_layers":
            self.opt.zero_grad(set_to_none=True)
            xq, s = m.quant_input(self.x)
            x = dq.apply_mlp(xq, m.bot_l, s)
            slab = m.tables.forward(cur, bits=m.embedding_bit, refresh_scale=True,
                                    full_precision=m.embedding_full_precision, layout="btd").requires_grad_(True)
            r, sf = m.quant_feature_outputs(m.interact(x, slab))
            E = m.loss(dq.apply_mlp(r, m.top_l, sf), self.t)
            E.backward()
            m.tables.backward_sgd(cur, slab.grad, LR, ste=True, layout="btd")
            self.opt.step()
            return E
        if form == "train_step":
            return m.train_step(self.x, cur, self.t, LR)
        return m.train_step(self.x, cur, self.t, LR, next_batch=nxt)

    def expected_launches(self, form):
        """Fresh stacks, plain interaction: 3L + 5 for the one call; the composition adds the
        loss's backward launch and updates the stacks in two launches (libdqrm's launches: the
        profiler also sees autograd's fill of backward()'s root gradient, one kernel more)."""
        m, cur, nxt = self.model, self.batches[self.k], self.batches[1 - self.k]
        if form == "composed_layers":  # torch's optimizer and autograd launch kernels of their own
            return None
        if form == "composed" and self.qact:  # per-tensor stacks: two update launches each, not two in all
            return m.step_launches(cur, fresh=True) + 1 + 2
        if form == "composed":
            return 3 * self.layers + 5 + 2
        if form == "train_step":
            return m.step_launches(cur, fresh=True)
        return m.step_launches(cur, next_batch=nxt, prefetched=True, fresh=True)


def window(case, form, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        case.step(form)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def launches(case, form):
    """Device kernels of one step (torch.profiler); None if the profiler reports none."""
    from torch.profiler import ProfilerActivity, profile

    for _ in range(2):  # the second of them is a steady-state step of this form (prefetch in place)
        case.step(form)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        case.step(form)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
    return (len(kernels) or None), len(names) - len(kernels)


def one_run(iters, repeats, cases, qact=False):
    results = []
    forms = QACT_FORMS if qact else FORMS
    for name, B in cases:
        c = Case(name, B, qact)
        for form in forms:
            for _ in range(20):
                c.step(form)
        torch.cuda.synchronize()
        t = {f: [] for f in forms}
        for _ in range(repeats):
            for f in forms:
                t[f].append(window(c, f, iters))
        r = {"case": f"{name}-{B}", "mlp_bot": MLPS[name][0], "mlp_top": MLPS[name][1], "B": B, "tables": 26,
             "dim": CONFIGS[name][1], "row_cap": ROW_CAP, "iters": iters, "repeats": repeats, "lr": LR,
             "quantize_activation": qact}
        for f in forms:
            r[f + "_us_per_step"] = round(statistics.median(t[f]), 1)
            r[f + "_us_windows"] = [round(v, 1) for v in t[f]]
        r["window_ratios_train_step_over_composed"] = [round(b / a, 3) for a, b in zip(t["composed"], t["train_step"])]
        if qact:
            r["window_ratios_train_step_over_composed_layers"] = [round(b / a, 3) for a, b in
                                                                  zip(t["composed_layers"], t["train_step"])]
        r["window_ratios_next_over_train_step"] = [round(b / a, 3) for a, b in zip(t["train_step"], t["train_step_next"])]
        for f in forms:
            want = c.expected_launches(f)
            try:
                got, copies = launches(c, f)
            except Exception as e:  # the counts are bookkeeping; the timings stand without them
                print(f"launch count unavailable: {e}", file=sys.stderr)
                got = copies = None
            r[f + "_launches_profiled"], r[f + "_launches_expected"] = got, want
            r[f + "_memsets_and_copies_profiled"] = copies
        r["one_launch_update_and_next_forward"] = c.model.tables.sgd_fwd_is_one_launch(c.batches[0], c.batches[1])
        r["device_errors"] = c.model.tables.read_errors()
        results.append(r)
        print(json.dumps(r), flush=True)
        del c
        torch.cuda.empty_cache()
    return results


def summarise(runs, cases, qact=False):
    out = []
    for k, (name, B) in enumerate(cases):
        row = {"case": f"{name}-{B}"}
        med = {}
        for f in (QACT_FORMS if qact else FORMS):
            v = [r["results"][k][f + "_us_per_step"] for r in runs]
            row[f + "_us_runs"], row[f + "_us"] = v, statistics.median(v)
            med[f] = statistics.median(v)
            row[f + "_launches_profiled"] = runs[-1]["results"][k][f + "_launches_profiled"]
            row[f + "_launches_expected"] = runs[-1]["results"][k][f + "_launches_expected"]
        row["train_step_over_composed"] = round(med["train_step"] / med["composed"], 3)
        row["next_over_train_step"] = round(med["train_step_next"] / med["train_step"], 3)
        ratios = [r["results"][k]["window_ratios_train_step_over_composed"] for r in runs]
        row["window_ratios_train_step_over_composed"] = ratios
        row["train_step_faster_in_every_window_pair"] = all(v < 1.0 for run in ratios for v in run)
        row["window_ratios_next_over_train_step"] = [r["results"][k]["window_ratios_next_over_train_step"] for r in runs]
        if qact:
            row["train_step_over_composed_layers"] = round(med["train_step"] / med["composed_layers"], 3)
            ratios = [r["results"][k]["window_ratios_train_step_over_composed_layers"] for r in runs]
            row["window_ratios_train_step_over_composed_layers"] = ratios
            row["train_step_faster_than_composed_layers_in_every_window_pair"] = all(v < 1.0 for run in ratios for v in run)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", default=None, help="comma-separated subset, e.g. kaggle-128,terabyte-2048")
    ap.add_argument("--quantize-activation", action="store_true",
                    help="DQRMNet(quantize_activation=True): the QuantActs and the integer-activation stacks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    qact = args.quantize_activation
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "model_step_qact.json" if qact else "model_step.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_model.py measures on a GPU; none found")
    dq.build(verbose=False)
    cases = CASES if not args.cases else [c for c in CASES if f"{c[0]}-{c[1]}" in args.cases.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
           "quantize_activation": qact,
           "forms": {"composed": "DQRMNet.forward + DLRMLoss under autograd, tables.backward_sgd, MLPStack.sgd_step x 2",
                     **({"composed_layers": "QuantAct + apply_mlp over the layers + DotInteraction + DLRMLoss under "
                                            "autograd, tables.backward_sgd, torch.optim.SGD on the MLPs"} if qact else {}),
                     "train_step": "DQRMNet.train_step (dqrm_model_step_qact)" if qact
                     else "DQRMNet.train_step (dqrm_model_step)",
                     "train_step_next": "DQRMNet.train_step(next_batch=...)"},
           "runs": [{"results": one_run(args.iters, args.repeats, cases, qact)} for _ in range(args.runs)]}
    doc["summary"] = summarise(doc["runs"], cases, qact)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for row in doc["summary"]:
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
