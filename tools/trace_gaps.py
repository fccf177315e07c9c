"""Median duration of k_coalesce_p1 launches (any instance) and the median gap between consecutive
ones (start[i+1] - end[i]) from a rocprofv3 --kernel-trace directory. usage: python tools/trace_gaps.py <rocprof dir> <out.json>"""
import csv, glob, json, sys
import numpy as np
rows = []
for f in glob.glob(f"{sys.argv[1]}/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
dur, gap, names = [], [], set()
for i, (s, e, n) in enumerate(rows):
    if "k_coalesce_p1" not in n:
        continue
    dur.append((e - s) / 1e3)
    names.add(n)
    if i + 1 < len(rows) and "k_coalesce_p1" in rows[i + 1][2]:
        gap.append((rows[i + 1][0] - e) / 1e3)
d, g = np.array(dur), np.array(gap)
out = {"kernels": sorted(names), "launches": int(d.size), "median_us": round(float(np.median(d)), 2),
       "p10_us": round(float(np.percentile(d, 10)), 2), "p90_us": round(float(np.percentile(d, 90)), 2),
       "consecutive_pairs": int(g.size), "gap_median_us": round(float(np.median(g)), 2),
       "gap_p10_us": round(float(np.percentile(g, 10)), 2), "gap_p90_us": round(float(np.percentile(g, 90)), 2),
       "pitch_median_us": round(float(np.median(d) + np.median(g)), 2)}
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(json.dumps(out))
