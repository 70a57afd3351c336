"""per-kernel means of a rocprofv3 kernel trace, the epilogue split by grid size (U and V launches)"""
import csv, glob, sys, collections
d = sys.argv[1]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
acc = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    n = r["Kernel_Name"]
    if "mu_epilogue" in n:
        key = ("mu_epilogue" + n.split("mu_epilogue")[1].split("(")[0], r.get("Grid_Size_X", r.get("Grid_Size", "?")))
        acc[key].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for k, v in sorted(acc.items()):
    v = sorted(v)
    print("%-44s grid %-8s calls %4d mean %7.2f us median %7.2f min %7.2f max %7.2f" % (k[0], k[1], len(v), sum(v) / len(v) / 1e3, v[len(v) // 2] / 1e3, v[0] / 1e3, v[-1] / 1e3))
