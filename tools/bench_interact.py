#!/usr/bin/env python3
"""Forward + backward of DLRM's dot feature interaction through DotInteraction (libdqrm's fused
kernels) against the reference's op sequence composed from torch ops, same process, same GPU.

Cases: F = 27 features (26 tables + the bottom MLP's output) at D = 16 (Kaggle) and D = 64
(Terabyte), B = 128 and 2048, plain and 16-bit quantized (modify_feature_interaction), without
the diagonal. One step = the interaction's forward and the backward from a fixed output gradient
into x [B, D] and the embedding slab ly [B, 26, D] (both need gradients, as in the model).

The composed form is interact_features (dlrm_s_pytorch_comm_grad.py:701-806) on torch ops: cat,
view, bmm, Z[:, li, lj], cat; quantized: min / max / abs / clamp / div for the scale, round /
clamp with the STE's `grad / s` backward, bmm, mul by scale ** 2. li / lj are built once and kept
on the device (the reference builds them on the CPU in every call, which would flatter the
module); ly is the same [B, 26, D] slab, unbound into the reference's list.

Timing: device events around `--iters` steps, `--repeats` windows per form, the two forms
alternating, median reported (host launch cost included: at these sizes a step is mostly that).
Launches per step: device kernels counted by torch.profiler over one step, in a pass of its own.
floor_us: each kernel's algorithmic bytes (inputs read once, outputs written once) at the HBM
peak of 8 TB/s, for information. Writes profiles/interact.json (or --out).

usage: python tools/bench_interact.py [--iters 200] [--repeats 5] [--out profiles/interact.json]
       python tools/bench_interact.py --trace-only CASE   (module steps only, for rocprofv3
                                          --kernel-trace --stats; CASE e.g. terabyte-2048-q16)
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

F_ = 27
DIMS = {"kaggle": 16, "terabyte": 64}
HBM_PEAK = 8.0e12  # bytes / s


class _SymQuant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, bits, s, zero):
        n = 2 ** (bits - 1) - 1
        ctx.s = s
        return torch.clamp(torch.round(1.0 / s * v + zero), -n - 1, n)

    @staticmethod
    def backward(ctx, g):
        return g / ctx.s, None, None, None


class ComposedInteraction(nn.Module):
    """interact_features as torch ops, li / lj cached on the device."""

    def __init__(self, F, bits):
        super().__init__()
        self.bits = bits
        self.register_buffer("li", torch.tensor([i for i in range(F) for j in range(i)], device="cuda"))
        self.register_buffer("lj", torch.tensor([j for i in range(F) for j in range(i)], device="cuda"))
        self.register_buffer("zero", torch.zeros((), device="cuda"))

    def forward(self, x, ly):
        B, d = x.shape
        T = torch.cat([x] + list(ly.unbind(1)), dim=1).view((B, -1, d))
        if self.bits:
            n = 2 ** (self.bits - 1) - 1
            lo, hi = T.data.min(), T.data.max()
            s = torch.clamp(torch.maximum(lo.abs(), hi.abs()), min=1e-8) / n
            Ti = _SymQuant.apply(T, self.bits, s, self.zero)
            Z = torch.bmm(Ti, torch.transpose(Ti, 1, 2)) * (s ** 2)
        else:
            Z = torch.bmm(T, torch.transpose(T, 1, 2))
        return torch.cat([x] + [Z[:, self.li, self.lj]], dim=1)


class Case:
    def __init__(self, D, B, bits, module):
        self.form = dq.DotInteraction(quantize_bits=bits) if module else ComposedInteraction(F_, bits)
        g = torch.Generator(device="cuda").manual_seed(3)
        self.x = torch.randn(B, D, device="cuda", generator=g).requires_grad_(True)
        self.ly = torch.randn(B, F_ - 1, D, device="cuda", generator=g).requires_grad_(True)
        self.dr = torch.randn(B, D + F_ * (F_ - 1) // 2, device="cuda", generator=g)

    def step(self):
        self.x.grad = self.ly.grad = None
        r = self.form(self.x, self.ly)
        r.backward(self.dr)
        return r


def window(case, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        case.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def launches(case):
    """Device kernels (and memsets) of one step (torch.profiler); None if the profiler reports none."""
    from torch.profiler import ProfilerActivity, profile

    case.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        case.step()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return n or None


def floors(D, B, bits):
    """Microseconds each kernel's algorithmic bytes take at the HBM peak."""
    tile, out = 4 * B * F_ * D, 4 * B * (D + F_ * (F_ - 1) // 2)
    f = {"fwd": (tile + out) / HBM_PEAK * 1e6, "bwd": (tile + out + tile) / HBM_PEAK * 1e6}
    if bits:
        f["scale"] = tile / HBM_PEAK * 1e6
    return {k: round(v, 2) for k, v in f.items()}


def case_name(name, B, bits):
    return f"{name}-{B}-" + (f"q{bits}" if bits else "plain")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interact.json"))
    ap.add_argument("--trace-only", default=None, metavar="CASE")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_interact.py measures on a GPU; none found")
    dq.build(verbose=False)
    if args.trace_only:
        name, B, mode = args.trace_only.split("-")
        case = Case(DIMS[name], int(B), int(mode[1:]) if mode != "plain" else None, True)
        for _ in range(args.iters):
            case.step()
        torch.cuda.synchronize()
        return
    results = []
    for name, D in DIMS.items():
        for B in (128, 2048):
            for bits in (None, 16):
                mod, ref = Case(D, B, bits, True), Case(D, B, bits, False)
                for c in (mod, ref):  # warm-up: code objects, the GEMM library's algorithm choice
                    for _ in range(20):
                        c.step()
                rm, rr = mod.step(), ref.step()
                diff = float((rm - rr).abs().max() / rr.abs().max())
                gdiff = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max())
                            for a, b in ((mod.x, ref.x), (mod.ly, ref.ly)))
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
                r = {"case": case_name(name, B, bits), "F": F_, "D": D, "B": B, "quantize_bits": bits or 0,
                     "iters": args.iters, "repeats": args.repeats,
                     "module_us_per_step": round(statistics.median(tm), 1),
                     "composed_us_per_step": round(statistics.median(tr), 1),
                     "module_us_windows": [round(t, 1) for t in tm], "composed_us_windows": [round(t, 1) for t in tr],
                     "module_over_composed": round(statistics.median(tm) / statistics.median(tr), 3),
                     "module_launches_per_step": lm, "composed_launches_per_step": lr_,
                     "module_launches_by_construction": 2 + (2 if bits else 0),
                     "kernel_floor_us_at_hbm_peak": floors(D, B, bits),
                     "max_output_diff_over_max_output": diff, "max_grad_diff_over_max_grad": gdiff}
                results.append(r)
                print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
