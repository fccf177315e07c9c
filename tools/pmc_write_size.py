"""Per-kernel mean WRITE_SIZE (bytes per launch) from a rocprofv3 --pmc WRITE_SIZE directory.
usage: python tools/pmc_write_size.py <rocprof dir> <label> <out.jsonl>"""
import collections, csv, glob, json, re, sys
acc = collections.defaultdict(list)
for f in glob.glob(f"{sys.argv[1]}/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if r["Counter_Name"] == "WRITE_SIZE":
            m = re.search(r"k_[a-z0-9_]+", r["Kernel_Name"])
            acc[m.group(0) if m else r["Kernel_Name"][:40]].append(float(r["Counter_Value"]) * 1024.0)
with open(sys.argv[3], "a") as o:
    for k, v in sorted(acc.items()):
        if any(s in k for s in ("k_apply", "k_coalesce", "k_qpack", "k_finalize", "k_table_finalize")):
            line = {"variant": sys.argv[2], "kernel": k, "launches": len(v), "write_size_bytes_mean": round(sum(v) / len(v))}
            o.write(json.dumps(line) + "\n"); print(line)
