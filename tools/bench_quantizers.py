#!/usr/bin/env python3
"""The LSQ and PACT embedding baselines, embedding forward + backward + SGD only, in one process
on one GPU, per quantizer four forms on the same tables and batches:

  (a) ``torch``: the same semantics composed from torch ops -- ``nn.EmbeddingBag(sparse=True)``
      per table, elementwise ops, ``torch.optim.SGD`` -- with the formulas restated here. This is
      what a user could run before. PACT's form maps the whole table on every forward, as the
      reference does;
  (b) ``modules``: the 26 per-table modules (QuantEmbeddingBagLSQ / QuantEmbeddingBagPACT) as a
      driver gets them by changing its imports: grad_mode "sparse" under ``torch.optim.SGD``;
      ``modules_fused``: the same modules with grad_mode "fused_sgd";
  (c) ``collection``: LSQEmbeddingBagCollection / PACTEmbeddingBagCollection, grad_mode
      "fused_sgd" (LSQ's steps under ``torch.optim.SGD``).

Workload: Kaggle's 26 tables capped at 500 k rows, D = 16, B = 128 and 2048, Criteo-form
batches (the modules are told so: set_pooling_one_inputs), bit width 4, every form alternating
between the same two batches and given the same upstream gradient. tools/bench_model.py's method:
device events around `--iters` steps, `--repeats` windows per form, the forms alternating, medians.
Kernels per step are counted by torch.profiler over one step, in a pass of its own.

usage: python tools/bench_quantizers.py [--iters 200] [--repeats 5] [--out profiles/quantizers.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_quantized_recommendation_model_dqrm_amd as dq  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd import quant_modules_not_quantize_grad as Q  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd.workloads import CONFIGS, synthetic_indices  # noqa: E402

LR = 1e-3  # small: the same two batches every step, thousands of steps
ROW_CAP = 500_000
BITS = 4
FORMS = ("torch", "modules", "modules_fused", "collection")


class _DoReFaSTE(torch.autograd.Function):
    """v = 2 * (round(sc * (tanh(w) / (2 max|tanh|) + 0.5)) / sc) - 1 over a whole table; identity backward."""

    @staticmethod
    def forward(ctx, w, k):
        sc = 2 ** k - 1
        t = torch.tanh(w)
        return 2 * (torch.round(sc * (t / (2 * t.abs().max()) + 0.5)) / sc) - 1

    @staticmethod
    def backward(ctx, g):
        return g, None


def _lsq_torch(x, s, bit):
    hi = 2 ** (bit - 1) - 1
    sg = s * (1.0 / math.sqrt(hi * x.numel()))
    s_scale = (s - sg).detach() + sg
    x = torch.clamp(x / s_scale, -hi - 1, hi)
    x = (x.round() - x).detach() + x
    return x * s_scale


class TorchForm:
    def __init__(self, kind, rows, D, Ws):
        self.kind = kind
        self.bags = [nn.EmbeddingBag(n, D, mode="sum", sparse=True, _weight=W.clone().cuda()) for n, W in zip(rows, Ws)]
        self.steps = [nn.Parameter((W.abs().mean() * 2 / ((2 ** (BITS - 1) - 1) ** 0.5)).reshape(1).cuda())
                      for W in Ws] if kind == "lsq" else []
        self.opt = torch.optim.SGD([b.weight for b in self.bags] + self.steps, lr=LR)

    def step(self, idx, off, dys):
        self.opt.zero_grad(set_to_none=True)
        ys = []
        for t, bag in enumerate(self.bags):
            if self.kind == "lsq":
                ys.append(_lsq_torch(bag(idx[t], off), self.steps[t], BITS))
            else:
                ys.append(F.embedding_bag(idx[t], _DoReFaSTE.apply(bag.weight, BITS), off, sparse=True, mode="sum"))
        torch.autograd.backward(ys, dys)
        self.opt.step()


class ModulesForm:
    def __init__(self, kind, rows, D, Ws, grad_mode):
        kw = dict(grad_mode=grad_mode, lr=LR)
        if kind == "lsq":
            self.mods = [dq.QuantEmbeddingBagLSQ(n, D, BITS, embedding_id=t, weight=W, **kw)
                         for t, (n, W) in enumerate(zip(rows, Ws))]
        else:
            self.mods = [dq.QuantEmbeddingBagPACT(n, D, BITS, embedding_id=t, weight=W, **kw)
                         for t, (n, W) in enumerate(zip(rows, Ws))]
        params = [m.quan_w_fn.s for m in self.mods] if kind == "lsq" else []
        if grad_mode == "sparse":
            params += [m.embedding_bag.weight for m in self.mods]
        self.opt = torch.optim.SGD(params, lr=LR) if params else None

    def step(self, idx, off, dys):
        if self.opt is not None:
            self.opt.zero_grad(set_to_none=True)
        ys = [m(idx[t], off) for t, m in enumerate(self.mods)]
        torch.autograd.backward(ys, dys)
        if self.opt is not None:
            self.opt.step()


class CollectionForm:
    def __init__(self, kind, rows, D, Ws):
        kw = dict(weights=Ws, grad_mode="fused_sgd", lr=LR)
        self.c = (dq.LSQEmbeddingBagCollection(rows, D, bit=BITS, **kw) if kind == "lsq"
                  else dq.PACTEmbeddingBagCollection(rows, D, BITS, **kw))
        self.opt = torch.optim.SGD([self.c.quan_w_fn.s], lr=LR) if kind == "lsq" else None

    def step(self, idx, off, dys):
        if self.opt is not None:
            self.opt.zero_grad(set_to_none=True)
        y = self.c(off, idx, layout="tbd")
        y.backward(dys)
        if self.opt is not None:
            self.opt.step()


class Case:
    def __init__(self, kind, B):
        rows, D = CONFIGS["kaggle"]
        self.rows = rows = [min(n, ROW_CAP) for n in rows]
        rs = np.random.RandomState(7)
        Ws = [torch.from_numpy(rs.uniform(-np.sqrt(1 / n), np.sqrt(1 / n), (n, D)).astype(np.float32)) for n in rows]
        self.forms = {"torch": TorchForm(kind, rows, D, Ws), "modules": ModulesForm(kind, rows, D, Ws, "sparse"),
                      "modules_fused": ModulesForm(kind, rows, D, Ws, "fused_sgd"),
                      "collection": CollectionForm(kind, rows, D, Ws)}
        self.idx = [synthetic_indices(rows, B, seed, device="cuda") for seed in (11, 12)]
        self.off = torch.arange(B, device="cuda")
        self.off_all = self.off.expand(len(rows), -1).contiguous()
        g = torch.Generator(device="cuda").manual_seed(3)
        self.dy = torch.randn(len(rows), B, D, device="cuda", generator=g) * 0.05
        self.dys = list(self.dy.unbind(0))
        self.k = 0
        self.table_bytes = sum(rows) * D * 4

    def step(self, form):
        idx = self.idx[self.k]
        self.k = 1 - self.k
        if form == "collection":
            self.forms[form].step(idx, self.off_all, self.dy)
        else:
            self.forms[form].step(idx, self.off, self.dys)


def window(case, form, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        case.step(form)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernels(case, form):
    """(device kernels of one step, of them this library's quantizer kernels, memsets and copies)."""
    from torch.profiler import ProfilerActivity, profile

    for _ in range(2):
        case.step(form)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        case.step(form)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    ks = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
    own = [n for n in ks if any(m in n for m in ("k_emb_fwd_quantizer", "k_lsq_bwd", "k_lsq_dstep"))]
    return len(ks) or None, len(own), len(names) - len(ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="128,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantizers.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quantizers.py measures on a GPU; none found")
    dq.build(verbose=False)
    Q.set_pooling_one_inputs(True)
    results = []
    for kind in ("lsq", "pact"):
        for B in [int(b) for b in args.batches.split(",")]:
            c = Case(kind, B)
            for f in FORMS:
                for _ in range(10):
                    c.step(f)
            torch.cuda.synchronize()
            t = {f: [] for f in FORMS}
            for _ in range(args.repeats):
                for f in FORMS:
                    t[f].append(window(c, f, args.iters))
            r = {"quantizer": kind, "B": B, "tables": len(c.rows), "dim": 16, "bits": BITS, "row_cap": ROW_CAP,
                 "table_bytes": c.table_bytes, "iters": args.iters, "repeats": args.repeats, "lr": LR}
            for f in FORMS:
                r[f + "_us_per_step"] = round(statistics.median(t[f]), 1)
                r[f + "_us_windows"] = [round(v, 1) for v in t[f]]
                try:
                    r[f + "_kernels_profiled"], r[f + "_quantizer_kernels_profiled"], r[f + "_memsets_and_copies"] = \
                        kernels(c, f)
                except Exception as e:  # the counts are bookkeeping; the timings stand without them
                    print(f"kernel count unavailable: {e}", file=sys.stderr)
            for f in FORMS[1:]:
                r["window_ratios_%s_over_torch" % f] = [round(b / a, 3) for a, b in zip(t["torch"], t[f])]
            r["device_errors"] = c.forms["collection"].c._tset.read_errors()
            results.append(r)
            print(json.dumps(r), flush=True)
            del c
            torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events, host launches included",
           "workload": "Kaggle's 26 tables capped at 500 k rows, D = 16, Criteo-form batches, embedding forward + "
                       "backward + SGD only, bit width 4",
           "forms": {"torch": "nn.EmbeddingBag(sparse=True) per table + elementwise torch ops + torch.optim.SGD",
                     "modules": "26 per-table modules, grad_mode 'sparse', torch.optim.SGD",
                     "modules_fused": "26 per-table modules, grad_mode 'fused_sgd'",
                     "collection": "the T-table collection, grad_mode 'fused_sgd'"},
           "not_measured": "kernel times (no rocprofv3 pass), other dims and bit widths, bags of several lookups, "
                           "Terabyte's tables, the uncapped Kaggle tables",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
