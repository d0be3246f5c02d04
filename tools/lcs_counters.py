"""nw_lcs_suffix_kernel's hardware counters per wave and per step, from rocprofv3 --pmc passes restricted to the kernel
(each pass a run of its own, with no tracing beside it; --output-format csv).  Every counter is summed over the
kernel's dispatches and divided by the waves of the same pass (SQ_WAVES, where the pass has it, else dispatches x
problems) and by the n + 63 skewed steps a wave runs.
python tools/lcs_counters.py DIR [DIR ..] nprob n"""
import csv
import glob
import os
import sys

dirs, nprob, n = sys.argv[1:-2], int(sys.argv[-2]), int(sys.argv[-1])
for d in dirs:
    files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        print("%s: no counter_collection.csv" % d)
        continue
    total, dispatches = {}, set()
    for f in files:
        for row in csv.DictReader(open(f)):
            if "nw_lcs_suffix_kernel" not in row.get("Kernel_Name", ""):
                continue
            dispatches.add(row.get("Dispatch_Id"))
            total[row["Counter_Name"]] = total.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    waves = total.get("SQ_WAVES") or len(dispatches) * nprob
    print("%s: %d dispatches, %.0f waves" % (d, len(dispatches), waves))
    for name in sorted(total):
        print("  %-22s %16.0f   per wave %12.1f   per step %8.2f" % (name, total[name], total[name] / waves, total[name] / waves / (n + 63)))
