#!/usr/bin/env python3
"""Forward + backward of the reference scripts' MLP stacks through QuantLinear (libdqrm's f32
MFMA kernels) against the same arithmetic composed from torch ops, same process, same GPU.

Cases: the Kaggle (13-512-256-64-16 / 367-512-256-1) and Terabyte (13-512-256-64 /
415-512-512-256-1) MLPs of workloads.MLPS at B = 128 and 2048, weight_bit = bias_bit = 4,
per_channel. One step = bottom stack forward, top stack forward, backward of both (ReLU after
every layer, Sigmoid after the last top layer, all left in torch). The first bottom layer's input
needs no gradient; the top stack's input does (it is the interaction's output in the model).

The composed form is QuantLinear.forward of the reference restated on torch ops (min / max /
abs / clamp / div for the scale, round / clamp with the STE's `grad / s` backward for the
integers, F.linear, mul by the scale), so autograd runs its backward.

Timing: device events around `--iters` steps, `--repeats` windows per form, the two forms
alternating, median reported. Launches per step: device kernels counted by torch.profiler over
one step, in a pass of its own. Writes profiles/linear_mlp.json (or --out).

usage: python tools/bench_linear.py [--iters 200] [--repeats 5] [--out profiles/linear_mlp.json]
       python tools/bench_linear.py --trace-only CASE    (module steps only, for rocprofv3
                                                          --kernel-trace --stats; CASE e.g. kaggle-128)
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_quantized_recommendation_model_dqrm_amd as dq  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd.workloads import MLPS  # noqa: E402

BITS = 4


class _SymQuant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, s, zero):
        n = 2 ** (BITS - 1) - 1
        ctx.s = s
        return torch.clamp(torch.round(1.0 / s * v + zero), -n - 1, n)

    @staticmethod
    def backward(ctx, g):
        return g / ctx.s, None, None


class ComposedLinear(nn.Module):
    """QuantLinear.forward (per_channel, weight only) as torch ops."""

    def __init__(self, lin):
        super().__init__()
        self.weight = nn.Parameter(lin.weight.data.clone())
        self.bias = nn.Parameter(lin.bias.data.clone())
        self.register_buffer("zero", torch.zeros((), device=lin.weight.device))

    def forward(self, x):
        n = 2 ** (BITS - 1) - 1
        w = self.weight.data
        w_min, w_max = w.min(dim=1).values, w.max(dim=1).values
        s = torch.max(torch.stack([w_min.abs(), w_max.abs()], dim=1), dim=1).values
        s = torch.clamp(s, min=1e-8) / n
        wi = _SymQuant.apply(self.weight, s.view(-1, 1), self.zero)
        bi = _SymQuant.apply(self.bias, s, self.zero)
        return F.linear(x, wi, bi) * s.view(1, -1)


class ModuleLinear(nn.Module):
    def __init__(self, lin):
        super().__init__()
        self.q = dq.QuantLinear(weight_bit=BITS, bias_bit=BITS, per_channel=True)
        self.q.set_param(lin)

    def forward(self, x):
        return self.q(x)[0]


def stack(dims, wrap, sigmoid_last, seed):
    torch.manual_seed(seed)
    layers = []
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        layers.append(wrap(nn.Linear(i, o).cuda()))
        layers.append(nn.Sigmoid() if sigmoid_last and k == len(dims) - 2 else nn.ReLU())
    return nn.Sequential(*layers)


class Case:
    def __init__(self, name, B, wrap):
        bot, top = MLPS[name]
        self.bot, self.top = stack(bot, wrap, False, 1), stack(top, wrap, True, 2)
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
        yb, yt = self.bot(self.xd), self.top(self.z)
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


def module_launches_by_construction(name):
    """QuantLinear's own launches per step: wquant + fwd per layer, dx + dw(+db) per layer,
    no dx for the first bottom layer; the activations' kernels come on top."""
    bot, top = MLPS[name]
    layers = len(bot) - 1 + len(top) - 1
    return 2 * layers + 2 * layers - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_mlp.json"))
    ap.add_argument("--trace-only", default=None, metavar="CASE")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear.py measures on a GPU; none found")
    dq.build(verbose=False)
    if args.trace_only:
        name, B = args.trace_only.rsplit("-", 1)
        case = Case(name, int(B), ModuleLinear)
        for _ in range(args.iters):
            case.step()
        torch.cuda.synchronize()
        return
    results = []
    for name in ("kaggle", "terabyte"):
        for B in (128, 2048):
            mod, ref = Case(name, B, ModuleLinear), Case(name, B, ComposedLinear)
            for c in (mod, ref):  # warm-up: code objects, the GEMM library's algorithm choice
                for _ in range(20):
                    c.step()
            ym, yr = mod.step(), ref.step()
            diff = max(float((a - b).abs().max()) for a, b in zip(ym, yr))
            gdiff = max(float((a.grad - b.grad).abs().max()) for a, b in zip(mod.params, ref.params))
            grel = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max().clamp(min=1e-30))
                       for a, b in zip(mod.params, ref.params))
            torch.cuda.synchronize()
            tm, tr = [], []
            for _ in range(args.repeats):
                tm.append(window(mod, args.iters))
                tr.append(window(ref, args.iters))
            try:
                lm, lr_ = launches(mod), launches(ref)
            except Exception as e:  # the counts are bookkeeping; the timings stand without them
                print(f"launch count unavailable: {e}", file=sys.stderr)
                lm = lr_ = None
            r = {"case": f"{name}-{B}", "mlp_bot": MLPS[name][0], "mlp_top": MLPS[name][1], "B": B,
                 "weight_bit": BITS, "per_channel": True, "iters": args.iters, "repeats": args.repeats,
                 "module_us_per_step": round(statistics.median(tm), 1),
                 "composed_us_per_step": round(statistics.median(tr), 1),
                 "module_us_windows": [round(t, 1) for t in tm], "composed_us_windows": [round(t, 1) for t in tr],
                 "module_over_composed": round(statistics.median(tm) / statistics.median(tr), 3),
                 "module_launches_per_step": lm, "composed_launches_per_step": lr_,
                 "module_linear_launches_by_construction": module_launches_by_construction(name),
                 "max_abs_output_diff": diff, "max_abs_param_grad_diff": gdiff,
                 "max_param_grad_diff_over_max_grad": grel}
            results.append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
