#!/usr/bin/env python3
"""The loss head, DLRMLoss against the torch sequence it replaces, same process, same GPU.

  dqrm    DLRMLoss(kind, weights, loss_threshold)(p, T) and .backward() to p.grad
          (dqrm_loss_fwd + dqrm_loss_bwd: 2 launches)
  torch   torch.clamp(p, min=th, max=1 - th), then loss_fn_wrap's body
          (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:193-212: BCELoss(reduction="mean"), or for
          wbce loss_ws[T.long()] * BCELoss(reduction="none") and .mean()), and .backward()

bce and wbce with loss_threshold = 0.01 at B = 128 and 2048 (forward + backward), and the forward
alone at B = 65536, the largest per-GPU batch of the drivers, where the one-workgroup forward is
at its worst. p is a leaf [B, 1] tensor in (0, 1), T is 0 / 1. Method as tools/bench_mlp.py:
device events around `--iters` steps, `--repeats` windows per form, the forms alternating,
medians; the launches of one step counted by torch.profiler in a pass of its own.

usage: python tools/bench_loss.py [--iters 500] [--repeats 5] [--out profiles/loss_head.json]
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

TH = 0.01
WS = [1.0, 2.5]


class Case:
    def __init__(self, B, kind, form, backward):
        g = torch.Generator(device="cuda").manual_seed(3)
        self.p = torch.rand(B, 1, device="cuda", generator=g).requires_grad_(backward)
        self.T = (torch.rand(B, 1, device="cuda", generator=g) < 0.3).float()
        self.kind, self.form, self.backward = kind, form, backward
        self.head = dq.DLRMLoss(kind, WS if kind == "wbce" else None, TH).cuda()
        self.loss_ws = torch.tensor(WS, device="cuda")
        self.bce_mean, self.bce_none = nn.BCELoss(reduction="mean"), nn.BCELoss(reduction="none")

    def step(self):
        self.p.grad = None
        if self.form == "dqrm":
            E = self.head(self.p, self.T)
        else:
            Z = torch.clamp(self.p, min=TH, max=1.0 - TH)
            if self.kind == "bce":
                E = self.bce_mean(Z, self.T)
            else:
                E = (self.loss_ws[self.T.data.view(-1).long()].view_as(self.T) * self.bce_none(Z, self.T)).mean()
        if self.backward:
            E.backward()
        return E


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_head.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py measures on a GPU; none found")
    dq.build(verbose=False)
    results = []
    for B, backward in ((128, True), (2048, True), (65536, False)):
        for kind in ("bce", "wbce"):
            mine, ref = Case(B, kind, "dqrm", backward), Case(B, kind, "torch", backward)
            for c in (mine, ref):
                for _ in range(30):
                    c.step()
            torch.cuda.synchronize()
            diff = abs(float(mine.step().detach()) - float(ref.step().detach()))
            tm, tr = [], []
            for _ in range(args.repeats):
                tm.append(window(mine, args.iters))
                tr.append(window(ref, args.iters))
            try:
                lm, lr = launches(mine), launches(ref)
            except Exception as e:  # the counts are bookkeeping; the timings stand without them
                print(f"launch count unavailable: {e}", file=sys.stderr)
                lm = lr = None
            r = {"case": f"{kind}-clamp-{B}-{'fwd+bwd' if backward else 'fwd'}", "B": B, "kind": kind,
                 "loss_threshold": TH, "backward": backward, "iters": args.iters, "repeats": args.repeats,
                 "dqrm_us_per_step": round(statistics.median(tm), 2), "torch_us_per_step": round(statistics.median(tr), 2),
                 "dqrm_us_windows": [round(t, 2) for t in tm], "torch_us_windows": [round(t, 2) for t in tr],
                 "dqrm_over_torch": round(statistics.median(tm) / statistics.median(tr), 3),
                 "dqrm_launches_per_step": lm, "torch_launches_per_step": lr,
                 "dqrm_launches_by_construction": 2 if backward else 1, "loss_abs_diff": diff}
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
