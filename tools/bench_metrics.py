#!/usr/bin/env python3
"""A test pass of the Kaggle-shape model, two forms in one process on one GPU, on one DQRMNet:

  (a) the reference's form of the loop (inference(), dlrm_s_pytorch_tb_dp_one_parallel_comm.py:
      1304-1404) on this package's forward: per batch ``predict(x, batch, labels)``,
      ``torch.cuda.synchronize()``, scores and targets ``.cpu()``, ``np.round(S, 0) == T``; at the
      end ``sklearn.metrics.roc_auc_score`` if sklearn imports on the machine, else the same area
      in numpy (sort + searchsorted). The result says which one ran;
  (b) ``model.evaluate(batches, metrics)``: every score stays on the device, one 40-byte read-back.

The model: workloads.MLPS["kaggle"] with its 26 tables (rows capped at 500 k as in bench_model.py),
D = 16, weight_bit = 4, per_channel, B = 2048, `--batches` batches per pass, each with dense inputs
and labels of its own (so the scores differ from batch to batch) over four index batches. This path
has no earlier form in the package, so (a) is the baseline.

A pass ends in host work in both forms, so a pass is timed by the host clock around work that ends
in a device synchronise; device events around the same work are reported beside it. `--repeats`
windows per form, the forms alternating, medians.

The finish alone (dqrm_metrics_finish, device events, reset + one update before each) at 2^16, 2^20
and 2^24 uniform-random samples, beside the host's AUC on the same samples.

usage: python tools/bench_metrics.py [--batches 128] [--repeats 5] [--out profiles/metrics.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deep_quantized_recommendation_model_dqrm_amd as dq  # noqa: E402
from deep_quantized_recommendation_model_dqrm_amd.workloads import CONFIGS, MLPS, synthetic_indices  # noqa: E402

ROW_CAP = 500_000
B = 2048

try:
    from sklearn.metrics import roc_auc_score as _sk_auc
    HOST_AUC = "sklearn.metrics.roc_auc_score"
except Exception:  # no sklearn on this machine
    _sk_auc = None
    HOST_AUC = "numpy (sort + searchsorted, the Mann-Whitney form)"


def host_auc(T, S):
    if _sk_auc is not None:
        return float(_sk_auc(T, S))
    pos, neg = np.sort(S[T == 1]), S[T == 0]
    lb = np.searchsorted(pos, neg, side="left").astype(np.int64).sum()
    ub = np.searchsorted(pos, neg, side="right").astype(np.int64).sum()
    return (2 * pos.size * neg.size - int(lb) - int(ub)) / (2 * pos.size * neg.size)


def reference_form(model, batches):
    scores, targets, correct, n = [], [], 0, 0
    for x, batch, t in batches:
        _, Z = model.predict(x, batch, t)
        torch.cuda.synchronize()
        S, T = Z.detach().cpu().numpy(), t.detach().cpu().numpy().reshape(-1, 1)
        scores.append(S)
        targets.append(T)
        correct += int(np.sum((np.round(S, 0) == T).astype(np.uint8)))
        n += T.shape[0]
    S, T = np.concatenate(scores, axis=0).ravel(), np.concatenate(targets, axis=0).ravel()
    return {"n": n, "n_correct": correct, "test_acc": correct / n, "roc_auc": host_auc(T, S)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def bench_pass(nb, repeats):
    rows, D = CONFIGS["kaggle"]
    rows = [min(n, ROW_CAP) for n in rows]
    bot, top = MLPS["kaggle"]
    np.random.seed(7)
    model = dq.DQRMNet(rows, D, bot, top, per_channel=True, weight_bit=4, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    idx = [dq.LookupBatch.pooling_one(synthetic_indices(rows, B, seed, device="cuda")) for seed in (11, 12, 13, 14)]
    batches = [(torch.rand(B, bot[0], device="cuda", generator=g), idx[k % 4],
                (torch.rand(B, device="cuda", generator=g) < 0.25).float()) for k in range(nb)]
    metrics = dq.DLRMMetrics(nb * B)
    forms = {"reference_form": lambda: reference_form(model, batches),
             "evaluate": lambda: model.evaluate(batches, metrics=metrics)}
    res = {}
    for name, fn in forms.items():  # warm-up: code objects, workspaces, the host's caches
        res[name] = fn()
        fn()
    t = {name: {"host_ms": [], "event_ms": []} for name in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            _, host_ms, event_ms = timed(fn)
            t[name]["host_ms"].append(host_ms)
            t[name]["event_ms"].append(event_ms)
    r = {"model": "kaggle", "B": B, "batches": nb, "samples": nb * B, "row_cap": ROW_CAP, "repeats": repeats,
         "host_auc": HOST_AUC, "results": res,
         "integers_agree": res["evaluate"]["n_correct"] == res["reference_form"]["n_correct"],
         "auc_difference": abs(res["evaluate"]["roc_auc"] - res["reference_form"]["roc_auc"]),
         "finish_launches": metrics.finish_launches()}
    for name in forms:
        r[name + "_host_ms"] = round(statistics.median(t[name]["host_ms"]), 3)
        r[name + "_host_ms_windows"] = [round(v, 3) for v in t[name]["host_ms"]]
        r[name + "_event_ms"] = round(statistics.median(t[name]["event_ms"]), 3)
    r["window_ratios_evaluate_over_reference_form"] = [
        round(b / a, 3) for a, b in zip(t["reference_form"]["host_ms"], t["evaluate"]["host_ms"])]
    r["evaluate_faster_in_every_window_pair"] = all(v < 1.0 for v in r["window_ratios_evaluate_over_reference_form"])
    return r


def bench_finish(n, repeats):
    g = torch.Generator(device="cuda").manual_seed(n)
    z = torch.rand(n, device="cuda", generator=g)
    t = (torch.rand(n, device="cuda", generator=g) < 0.25).float()
    m = dq.DLRMMetrics(n)
    ms = []
    for k in range(repeats + 1):  # the first is the warm-up
        m.reset()
        m.update(z, t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        m._finish()
        e1.record()
        torch.cuda.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    got = m.compute()
    S, T = z.cpu().numpy(), t.cpu().numpy()
    t0 = time.perf_counter()
    want = host_auc(T, S)
    host_ms = (time.perf_counter() - t0) * 1e3
    return {"samples": n, "finish_event_ms": round(statistics.median(ms), 4),
            "finish_event_ms_windows": [round(v, 4) for v in ms], "finish_launches": m.finish_launches(),
            "host_auc": HOST_AUC, "host_auc_ms_once": round(host_ms, 3),
            "roc_auc": got["roc_auc"], "host_roc_auc": want, "auc_difference": abs(got["roc_auc"] - want)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="65536,1048576,16777216")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on a GPU; none found")
    dq.build(verbose=False)
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": "a pass: host clock around work that ends in a device synchronise (device events beside it); "
                     "the finish alone: device events",
           "forms": {"reference_form": "per batch predict, synchronize, .cpu(), np.round count; " + HOST_AUC,
                     "evaluate": "DQRMNet.evaluate (dqrm_model_fwd + dqrm_metrics_update per batch, "
                                 "dqrm_metrics_finish, one 40-byte read-back)"}}
    doc["test_pass"] = bench_pass(args.batches, args.repeats)
    print(json.dumps(doc["test_pass"]), flush=True)
    doc["finish_alone"] = []
    for n in (int(s) for s in args.sizes.split(",")):
        r = bench_finish(n, args.repeats)
        doc["finish_alone"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
