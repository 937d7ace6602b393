"""Alignment QC on one MI355X (csrc/qc.hip): what an add costs through the lane-per-cycle kernel, through the plain kernel alone,
and beside the pileup and depth adds on the same bytes.

The input is tools/pileup_rate.py's: coordinate-sorted records of 150M with random bases, qualities of 30 and either strand, at
--coverage (default 30) over one reference of --mbp (default 50) million bases; 267 bytes a record.  They go to bwams_qc_add_records,
whose kernels the library times between events (bwams_qc_info: ms_check, ms_add), once to warm up and --reps times (default 7),
first on the default path and then under BWAMS_QC_LANES=0; the upload before the kernels is outside the events.  In the same process
bwams_pileup_add_records (tiled, its own events) and bwams_depth_add_records (no events: the host clock around the call, with the
upload in it, next to the same clock around the QC add) take the same bytes.  One JSON line per measurement on stdout; the last line
holds the two comparisons of DESIGN 3.20: the default QC add against the tiled pileup add and against the plain kernel, each true
only when the faster one's slowest repetition is below the other's fastest.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bwams import capi  # noqa: E402
from pileup_rate import HBM_PEAK_GBS, records, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=50.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    l_ref = int(a.mbp * 1e6)
    n = int(l_ref * a.coverage / 150)
    rec = records(n, l_ref, 11)
    n_bytes = rec.nbytes
    ptr = rec.ctypes.data_as(C.c_void_p)
    L = capi.lib()
    print(json.dumps({"records": n, "bytes": n_bytes, "positions": l_ref, "coverage": a.coverage}), flush=True)
    total, qc_wall = {}, []
    for lanes in (1, 0):
        os.environ["BWAMS_QC_LANES"] = str(lanes)
        capi.debug_reload()
        q = capi.Qc()
        cnt = C.c_int64(0)
        check, add, wall = [], [], []
        for rep in range(a.reps + 1):                                                       # the first is the warm-up
            t = time.perf_counter()
            capi._chk(L.bwams_qc_add_records(q.h, ptr, n_bytes, C.byref(cnt)), "bwams_qc_add_records")
            w = (time.perf_counter() - t) * 1e3
            i = q.info()
            if rep:
                check.append(i["ms_check"]); add.append(i["ms_add"]); wall.append(w)
        _, scalars = q.summary()
        q.close()
        tag = "lanes" if lanes else "plain"
        total[tag] = [x + y for x, y in zip(check, add)]
        if lanes:
            qc_wall = wall
        med = float(np.median(total[tag]))
        print(json.dumps({"qc": tag, "counted": cnt.value, "check_ms": stats(check), "add_ms": stats(add), "kernels_ms": stats(total[tag]),
                          "call_ms": stats(wall), "records_per_s": round(n / med * 1e3), "record_gb_per_s": round(n_bytes / med / 1e6, 1),
                          "of_hbm_peak_pct": round(100 * n_bytes / med / 1e6 / HBM_PEAK_GBS, 2),
                          "qual_bases_per_add": int(scalars[8]) // (a.reps + 1)}), flush=True)
    del os.environ["BWAMS_QC_LANES"]
    capi.debug_reload()
    p = capi.Pileup([l_ref])                                                                # unchanged code: the tiled pileup add
    check, add = [], []
    for rep in range(a.reps + 1):
        capi._chk(L.bwams_pileup_add_records(p.h, ptr, n_bytes, None), "bwams_pileup_add_records")
        i = p.info()
        if rep:
            check.append(i["ms_check"]); add.append(i["ms_add"])
    p.close()
    total["pileup"] = [x + y for x, y in zip(check, add)]
    print(json.dumps({"pileup": "tiled", "check_ms": stats(check), "add_ms": stats(add), "kernels_ms": stats(total["pileup"])}), flush=True)
    d = capi.Depth([l_ref])
    wall = []
    for rep in range(a.reps + 1):
        t = time.perf_counter()
        capi._chk(L.bwams_depth_add_records(d.h, ptr, n_bytes, None), "bwams_depth_add_records")
        if rep:
            wall.append((time.perf_counter() - t) * 1e3)
    d.close()
    print(json.dumps({"depth": True, "call_ms": stats(wall), "qc_call_ms": stats(qc_wall)}), flush=True)
    med = {k: float(np.median(v)) for k, v in total.items()}
    print(json.dumps({"qc_over_pileup": round(med["lanes"] / med["pileup"], 3), "qc_below_pileup": max(total["lanes"]) < min(total["pileup"]),
                      "lanes_over_plain": round(med["lanes"] / med["plain"], 3),
                      "lanes_not_slower_than_plain": not max(total["plain"]) < min(total["lanes"])}), flush=True)


if __name__ == "__main__":
    main()
