"""The cover count in a rocprofv3 kernel trace of `bench.py --gpus 1 --steps K --warmup W`: per iteration of the fresh start (1 .. W + K)
the two cover_delta_kernel launches (or the one full cover_wide_kernel launch of a build / run without the previous words), and the
sum of ALL kernel times per step over the timed window.  Iterations are delimited by the loop's last launch (reduce_finalize_kernel).

    python scripts/cover_delta_trace.py DIR [--steps 60 --warmup 5 --after 1]      (--after: iterations run after the timed window)"""
import argparse
import collections
import csv
import glob

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--after", type=int, default=1)
a = ap.parse_args()
f = glob.glob(a.dir + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(({"name": r["Kernel_Name"], "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"])} for r in csv.DictReader(open(f))),
              key=lambda r: r["t0"])
ends = [i for i, r in enumerate(rows) if "reduce_finalize_kernel" in r["name"]]
n_it = a.warmup + a.steps
print(f"{len(ends)} iterations in the trace; the fresh start is the {n_it} before the last {a.after}")
last = len(ends) - a.after
first = last - n_it
per_it, totals = [], []
for it in range(n_it):
    lo = ends[first + it - 1] + 1 if first + it > 0 else 0
    seg = rows[lo:ends[first + it] + 1]
    cov = [(r["t1"] - r["t0"]) / 1e3 for r in seg if "cover_delta_kernel" in r["name"] or "cover_wide_kernel" in r["name"] or "cover_kernel" in r["name"]]
    per_it.append(cov)
    totals.append(sum(r["t1"] - r["t0"] for r in seg) / 1e3)
print("iter  cover launches (us)            sum")
for it, cov in enumerate(per_it, 1):
    print(f"{it:4d}  {'  '.join('%7.2f' % c for c in cov):28s}  {sum(cov):7.2f}{'   (timed)' if it > a.warmup else ''}")
win = per_it[a.warmup:]
sums = [sum(c) for c in win]
print(f"timed window: cover per step mean {sum(sums) / len(sums):.2f} us, max {max(sums):.2f} us (iteration {a.warmup + 1 + sums.index(max(sums))}), min {min(sums):.2f} us")
print(f"timed window: all kernels per step {sum(totals[a.warmup:]) / a.steps:.2f} us")
acc = collections.defaultdict(list)
for r in rows[ends[first + a.warmup - 1] + 1:ends[last - 1] + 1]:
    acc[r["name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][-60:]].append((r["t1"] - r["t0"]) / 1e3)
for k, v in sorted(acc.items(), key=lambda kv: -sum(kv[1])):
    v.sort()
    print(f"{k:60s} calls {len(v):4d} mean {sum(v) / len(v):8.2f} median {v[len(v) // 2]:8.2f} min {v[0]:8.2f} max {v[-1]:8.2f} us  per step {sum(v) / a.steps:8.2f}")
