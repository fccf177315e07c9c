#!/usr/bin/env python3
"""One training step of the Kaggle MLP stacks (workloads.MLPS["kaggle"]: bottom 13-512-256-64-16,
top 367-512-256-1) with activation quantization against the weight-only form, same process, same GPU.

  qact         quant_input(dense) -> bot_l, quant_feature_outputs(z) -> top_l, every layer built with
               quantize_activation=True (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:857-876); the two
               QuantAct modules are part of the step, as they are in the driver
  weight_only  the same stacks without the flag and without the QuantAct modules

weight_bit = 4, per-tensor scales in both forms (a per-channel scale cannot feed the next layer),
activations fused, B = 128 and 2048. One step = both stacks forward, backward of both; the dense
input needs no gradient, the top stack's does. Method as tools/bench_mlp.py: device events around
`--iters` steps, `--repeats` windows per form, the forms alternating, medians; the launches of one
step counted by torch.profiler in a pass of its own, beside the count by construction.

usage: python tools/bench_qact.py [--iters 200] [--repeats 5] [--out profiles/qact_mlp.json]
       python tools/bench_qact.py --trace-only B    (one warm-up and ONE qact step, for
                                                    rocprofv3 --kernel-trace: the launch counts)
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
from deep_quantized_recommendation_model_dqrm_amd.workloads import MLPS  # noqa: E402

BITS = 4
BOT, TOP = MLPS["kaggle"]


class Case:
    def __init__(self, B, qact):
        np.random.seed(1)
        self.bot = dq.create_mlp(BOT, -1, weight_bit=BITS, quantize_activation=qact).cuda()
        self.top = dq.create_mlp(TOP, len(TOP) - 2, weight_bit=BITS, quantize_activation=qact).cuda()
        self.qact = qact
        if qact:
            self.quant_input = dq.QuantAct(activation_bit=8, act_range_momentum=-1).cuda()
            self.quant_feature_outputs = dq.QuantAct(fixed_point_quantization=True, activation_bit=8,
                                                     act_range_momentum=-1).cuda()
        g = torch.Generator(device="cuda").manual_seed(3)
        self.xd = torch.rand(B, BOT[0], device="cuda", generator=g)
        self.z = torch.randn(B, TOP[0], device="cuda", generator=g).requires_grad_(True)
        self.dyb = torch.randn(B, BOT[-1], device="cuda", generator=g)
        self.dyt = torch.randn(B, TOP[-1], device="cuda", generator=g)
        self.params = list(self.bot.parameters()) + list(self.top.parameters())

    def step(self):
        for p in self.params:
            p.grad = None
        self.z.grad = None
        if self.qact:
            x, s = self.quant_input(self.xd)
            yb = dq.apply_mlp(x, self.bot, prev_act_scaling_factor=s)
            z, s2 = self.quant_feature_outputs(self.z)
            yt = dq.apply_mlp(z, self.top, prev_act_scaling_factor=s2)
        else:
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
    from torch.profiler import ProfilerActivity, profile

    case.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        case.step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")) or None


def launches_by_construction(B):
    """Per-tensor layers: wquant 2 + forward 1, backward 2 (1 for the first bottom layer, whose
    input needs no gradient). qact adds quant_input (2 launches up to 16384 elements, 3 beyond, no
    backward) and quant_feature_outputs (likewise, and 1 backward)."""
    layers = len(BOT) - 1 + len(TOP) - 1
    base = 5 * layers - 1
    act = sum(2 if B * k <= 16384 else 3 for k in (BOT[0], TOP[0])) + 1
    return base + act, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qact_mlp.json"))
    ap.add_argument("--trace-only", type=int, default=None, metavar="B")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qact.py measures on a GPU; none found")
    dq.build(verbose=False)
    if args.trace_only:
        c = Case(args.trace_only, True)
        c.step()
        torch.cuda.synchronize()
        c.step()
        torch.cuda.synchronize()
        return
    results = []
    for B in (128, 2048):
        qa, wo = Case(B, True), Case(B, False)
        for c in (qa, wo):
            for _ in range(20):
                c.step()
        torch.cuda.synchronize()
        tq, tw = [], []
        for _ in range(args.repeats):
            tq.append(window(qa, args.iters))
            tw.append(window(wo, args.iters))
        try:
            lq, lw = launches(qa), launches(wo)
        except Exception as e:  # the counts are bookkeeping; the timings stand without them
            print(f"launch count unavailable: {e}", file=sys.stderr)
            lq = lw = None
        bq, bw = launches_by_construction(B)
        r = {"case": f"kaggle-{B}", "mlp_bot": BOT, "mlp_top": TOP, "B": B, "weight_bit": BITS, "per_channel": False,
             "iters": args.iters, "repeats": args.repeats,
             "qact_us_per_step": round(statistics.median(tq), 1),
             "weight_only_us_per_step": round(statistics.median(tw), 1),
             "qact_us_windows": [round(t, 1) for t in tq], "weight_only_us_windows": [round(t, 1) for t in tw],
             "qact_over_weight_only": round(statistics.median(tq) / statistics.median(tw), 3),
             "qact_launches_per_step": lq, "weight_only_launches_per_step": lw,
             "qact_launches_by_construction": bq, "weight_only_launches_by_construction": bw}
        results.append(r)
        print(json.dumps(r), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
