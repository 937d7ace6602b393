"""Kernel timeline of one timed step from a rocprofv3 --kernel-trace CSV: start, end, duration (ms from the step's first kernel).
usage: python tools/step_timeline.py <kernel_trace.csv> [from_ms] [to_ms] [which_step] [min_ms]
min_ms (default 0.12) drops shorter kernels; 0 keeps every launch and adds the idle gap in front of each."""
import csv, re, sys
f = sys.argv[1]
lo = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0
hi = float(sys.argv[3]) if len(sys.argv) > 3 else 1e9
which = int(sys.argv[4]) if len(sys.argv) > 4 else 2
min_ms = float(sys.argv[5]) if len(sys.argv) > 5 else 0.12
rows = list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
idx = [i for i, r in enumerate(rows) if "smem_search_kernel<true>" in r["Kernel_Name"]]
i0 = idx[which]
i1 = idx[which + 1] if which + 1 < len(idx) else len(rows)
t0 = int(rows[i0]["Start_Timestamp"])
def short(n):
    n = n.replace("bwams::", "").replace("(anonymous namespace)::", "").replace("void ", "")
    m = re.match(r"([A-Za-z0-9_:]+(<[^(]*>)?)", n)
    return (m.group(1) if m else n)[:50]
busy_to = 0.0                       # end of the latest kernel seen so far: the gap column is the time nothing ran
for r in rows[i0:i1]:
    s = (int(r["Start_Timestamp"]) - t0) / 1e6
    e = (int(r["End_Timestamp"]) - t0) / 1e6
    gap = s - busy_to
    busy_to = max(busy_to, e)
    if s < lo or s > hi or e - s < min_ms:
        continue
    print("%8.3f %8.3f %7.3f %s %s lds=%s grid=%s" % (s, e, e - s, ("gap=%6.3f" % gap) if gap > 0 else "overlapped ",
                                                      short(r["Kernel_Name"]), r["LDS_Block_Size"], r["Grid_Size_X"]))
