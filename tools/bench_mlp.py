#!/usr/bin/env python3
"""Forward + backward of the reference scripts' MLP stacks with the activations fused into
QuantLinear's kernels (mlp.fuse_activations) against the same package layers followed by torch's
ReLU / Sigmoid, same process, same GPU.

Cases and method are tools/bench_linear.py's: the Kaggle and Terabyte MLPs of workloads.MLPS at
B = 128 and 2048, weight_bit = bias_bit = 4, per_channel; one step = bottom stack forward, top
stack forward, backward of both; the first bottom layer's input needs no gradient, the top stack's
does. Both forms are ModuleLists run by mlp.apply_mlp (the reference's loop). Device events around
`--iters` steps, `--repeats` windows per form, the two forms alternating, medians; launches per
step counted by torch.profiler over one step, in a pass of its own.

One invocation is one run. --append adds the run to the runs already in --out (the host these
measurements come from moves whole cases between levels from run to run, so the figure to quote is
the median over several runs; "summary" holds it). --parent FILE... records, beside the summary,
the "module" column of the parent commit's tools/bench_linear.py outputs taken in the same session.

usage: python tools/bench_mlp.py [--iters 200] [--repeats 5] [--out profiles/mlp_fused.json] [--append]
                                 [--parent linear_mlp_run1.json ...]
       python tools/bench_mlp.py --trace-only CASE   (fused and unfused steps alternating, for
                                                      rocprofv3 --kernel-trace --stats; CASE e.g. kaggle-128)
       python tools/bench_mlp.py --layer-times TRACE.csv   (no GPU: from that run's kernel trace, the
                                                      average time of each k_linear_gemm<WT, MODE, ACT> per
                                                      grid, an ACT instantiation beside the NONE one that ran
                                                      the same layers in the unfused form)
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_quantized_recommendation_model_dqrm_amd as dq  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd.workloads import MLPS  # noqa: E402

BITS = 4
CASES = [(name, B) for name in ("kaggle", "terabyte") for B in (128, 2048)]


def stack(dims, sigmoid_last, seed, fused):
    """bench_linear.py's stack (same seeds, same nn.Linear initialisation) as a ModuleList."""
    torch.manual_seed(seed)
    layers = nn.ModuleList()
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        q = dq.QuantLinear(weight_bit=BITS, bias_bit=BITS, per_channel=True)
        q.set_param(nn.Linear(i, o).cuda())
        layers.append(q)
        layers.append(nn.Sigmoid() if sigmoid_last and k == len(dims) - 2 else nn.ReLU())
    if fused:
        assert dq.fuse_activations(layers) == len(dims) - 1
    return layers


class Case:
    def __init__(self, name, B, fused):
        bot, top = MLPS[name]
        self.bot, self.top = stack(bot, False, 1, fused), stack(top, True, 2, fused)
        g = torch.Generator(device="cuda").manual_seed(3)
        self.xd = torch.rand(B, bot[0], device="cuda", generator=g)
        self.z = torch.randn(B, top[0], device="cuda", generator=g).requires_grad_(True)
        self.dyb = torch.randn(B, bot[-1], device="cuda", generator=g)
        self.dyt = torch.randn(B, top[-1], device="cuda", generator=g)
        self.params = list(self.bot.parameters()) + list(self.top.parameters())

    def step(self):
        for p in self.params:
            p.grad = None
        self.z.grad = None
        yb, yt = dq.apply_mlp(self.xd, self.bot), dq.apply_mlp(self.z, self.top)
        torch.autograd.backward([yb, yt], [self.dyb, self.dyt])
        return yb, yt


def window(case, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        case.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def launches(case):
    """Device kernels of one step (torch.profiler); None if the profiler reports none."""
    from torch.profiler import ProfilerActivity, profile

    case.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        case.step()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def launches_by_construction(name):
    """wquant + forward per layer, dx + dw(+db) per layer, no dx for the first bottom layer;
    unfused, an activation kernel per layer each way on top."""
    bot, top = MLPS[name]
    layers = len(bot) - 1 + len(top) - 1
    return 4 * layers - 1, 4 * layers - 1 + 2 * layers


def one_run(iters, repeats):
    results = []
    for name, B in CASES:
        fus, unf = Case(name, B, True), Case(name, B, False)
        for c in (fus, unf):
            for _ in range(20):
                c.step()
        yf, yu = fus.step(), unf.step()
        relu_equal = bool(torch.equal(yf[0], yu[0])) and all(
            torch.equal(a.grad, b.grad) for a, b in zip(fus.bot.parameters(), unf.bot.parameters()))
        sig_diff = float((yf[1] - yu[1]).abs().max())
        torch.cuda.synchronize()
        tf, tu = [], []
        for _ in range(repeats):
            tf.append(window(fus, iters))
            tu.append(window(unf, iters))
        try:
            lf, lu = launches(fus), launches(unf)
        except Exception as e:  # the counts are bookkeeping; the timings stand without them
            print(f"launch count unavailable: {e}", file=sys.stderr)
            lf = lu = None
        bf, bu = launches_by_construction(name)
        r = {"case": f"{name}-{B}", "mlp_bot": MLPS[name][0], "mlp_top": MLPS[name][1], "B": B,
             "weight_bit": BITS, "per_channel": True, "iters": iters, "repeats": repeats,
             "fused_us_per_step": round(statistics.median(tf), 1),
             "unfused_us_per_step": round(statistics.median(tu), 1),
             "fused_us_windows": [round(t, 1) for t in tf], "unfused_us_windows": [round(t, 1) for t in tu],
             "fused_over_unfused": round(statistics.median(tf) / statistics.median(tu), 3),
             "fused_launches_per_step": lf, "unfused_launches_per_step": lu,
             "fused_launches_by_construction": bf, "unfused_launches_by_construction": bu,
             "bottom_stack_bit_identical": relu_equal, "max_abs_top_output_diff": sig_diff}
        results.append(r)
        print(json.dumps(r), flush=True)
    return results


def summarise(runs, parent_runs):
    """Per case: every run's medians and the median over the runs, the parent's likewise."""
    out = []
    for k, (name, B) in enumerate(CASES):
        case = f"{name}-{B}"
        f = [r["results"][k]["fused_us_per_step"] for r in runs]
        u = [r["results"][k]["unfused_us_per_step"] for r in runs]
        row = {"case": case, "fused_us_runs": f, "fused_us": statistics.median(f),
               "unfused_us_runs": u, "unfused_us": statistics.median(u),
               "fused_launches_per_step": runs[-1]["results"][k]["fused_launches_per_step"],
               "unfused_launches_per_step": runs[-1]["results"][k]["unfused_launches_per_step"]}
        if parent_runs:
            p = [next(x["module_us_per_step"] for x in pr["results"] if x["case"] == case) for pr in parent_runs]
            row.update(parent_module_us_runs=p, parent_module_us=statistics.median(p),
                       fused_no_slower_than_parent=statistics.median(f) <= statistics.median(p))
        out.append(row)
    return out


def layer_times(path):
    """An instantiation's average over all its launches mixes layers of different sizes, and the
    fused and unfused forms send different layers to it; a grid identifies the layer shapes."""
    import collections
    import csv
    import re

    t = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            m = re.search(r"k_linear_gemm<(\d), (\d), (\d)(?:, false)?>", r["Kernel_Name"])  # not the QA ones
            if m:
                wt, mode, act = map(int, m.groups())
                grid = (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]))
                t[(mode, wt, grid, act)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    total = collections.defaultdict(lambda: [0.0, 0.0])
    for mode, wt, grid in sorted({k[:3] for k in t}):
        none = t.get((mode, wt, grid, 0))
        acts = [(a, t[(mode, wt, grid, a)]) for a in (1, 2) if (mode, wt, grid, a) in t]
        if not none or not acts:
            continue
        n_act = sum(len(v) for _, v in acts)
        for a, v in acts:
            print(f"{('FWD', 'DX', 'DW')[mode]} WT={wt} grid={grid[0]}x{grid[1]} {('', 'RELU', 'SIGMOID')[a]:7s} "
                  f"{statistics.mean(v):7.2f} us (n={len(v)})   NONE {statistics.mean(none):7.2f} us (n={len(none)})   "
                  f"ratio {statistics.mean(v) / statistics.mean(none):.3f}")
        total[mode][0] += sum(sum(v) for _, v in acts) / n_act * len(none)
        total[mode][1] += sum(none)
    for mode, (a, n) in sorted(total.items()):
        print(f"{('FWD', 'DX', 'DW')[mode]} all layers: ACT / NONE time {a / n:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_fused.json"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[], metavar="FILE")
    ap.add_argument("--trace-only", default=None, metavar="CASE")
    ap.add_argument("--layer-times", default=None, metavar="TRACE.csv")
    args = ap.parse_args()
    if args.layer_times:
        return layer_times(args.layer_times)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp.py measures on a GPU; none found")
    dq.build(verbose=False)
    if args.trace_only:
        name, B = args.trace_only.rsplit("-", 1)
        fus, unf = Case(name, int(B), True), Case(name, int(B), False)
        for _ in range(args.iters):
            fus.step()
            unf.step()
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included", "runs": []}
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["runs"].append({"results": one_run(args.iters, args.repeats)})
    parents = []
    for p in args.parent:
        with open(p) as f:
            parents.append(json.load(f))
    if parents:
        doc["parent_bench_linear_runs"] = parents
    doc["summary"] = summarise(doc["runs"], doc.get("parent_bench_linear_runs", []))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for row in doc["summary"]:
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
