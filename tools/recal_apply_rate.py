"""Applying base recalibration on one MI355X (csrc/recal_apply.hip): what an apply costs beside the counting add (csrc/recal.hip) on
the same bytes.

The input is that of tools/recal_rate.py: coordinate-sorted records of 150M on either strand at --coverage (default 30) over one
random reference of --mbp (default 50) million bases, 267 bytes a record, no read groups (every record is in the one row), mismatches
planted at --mismatch (default 0.01); here the QUAL bytes are drawn from 12, 20, 30, 37 and 41.  The tables are counted from these
bytes, the model is made from the tables, and bwams_recal_apply_records takes a fresh copy of the same bytes every time (it rewrites
its input), once to warm up and --reps times (default 7).  The library times its kernels between events (bwams_recal_apply_info:
ms_check, ms_apply; bwams_recal_info: ms_check, ms_add); the copies to and from the device are outside the events.  One JSON line per
measurement on stdout; the last line holds the comparison of DESIGN 3.22: the apply is "not slower" than the counting add unless the
add's slowest repetition is below the apply's fastest.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bwams import capi  # noqa: E402
from pileup_rate import HBM_PEAK_GBS, stats  # noqa: E402
from recal_rate import records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=50.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mismatch", type=float, default=0.01)
    a = ap.parse_args()
    l_ref = int(a.mbp * 1e6)
    n = int(l_ref * a.coverage / 150)
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 4, l_ref, dtype=np.uint8)
    rec, planted = records(n, ref, a.mismatch, 11)
    for k in range(0, n, 1 << 18):
        m = min(n, k + (1 << 18)) - k
        rec[k:k + m, 117:267] = rng.choice(np.array([12, 20, 30, 37, 41], np.uint8), (m, 150))
    n_bytes = rec.nbytes
    work = np.empty_like(rec)
    L = capi.lib()
    print(json.dumps({"records": n, "bytes": n_bytes, "positions": l_ref, "coverage": a.coverage, "mismatches_planted": planted}), flush=True)
    r = capi.Recal([l_ref], max_cycle=150)
    r.set_ref(0, ref)
    check, add = [], []
    for rep in range(a.reps + 1):                                                           # the first is the warm-up
        r.reset()
        capi._chk(L.bwams_recal_add_records(r.h, rec.ctypes.data_as(C.c_void_p), n_bytes, None), "bwams_recal_add_records")
        i = r.info()
        if rep:
            check.append(i["ms_check"]); add.append(i["ms_add"])
    count = [x + y for x, y in zip(check, add)]
    print(json.dumps({"recal_add": "lds" if i["lds"] else "plain", "bases_per_add": i["n_bases"], "check_ms": stats(check),
                      "add_ms": stats(add), "kernels_ms": stats(count)}), flush=True)
    model = capi.RecalModel.of(r)
    r.close()
    h = capi.RecalApply(model)
    model.close()
    cnt = C.c_int64(0)
    check, app = [], []
    for rep in range(a.reps + 1):
        np.copyto(work, rec)
        capi._chk(L.bwams_recal_apply_records(h.h, work.ctypes.data_as(C.c_void_p), n_bytes, C.byref(cnt)), "bwams_recal_apply_records")
        i = h.info()
        if rep:
            check.append(i["ms_check"]); app.append(i["ms_apply"])
    h.close()
    assert np.array_equal(work[:, :117], rec[:, :117])                                       # nothing but QUAL bytes changes
    total = [x + y for x, y in zip(check, app)]
    med = float(np.median(total))
    print(json.dumps({"recal_apply": "records", "rewritten": cnt.value, "bytes_changed": int((work[:, 117:] != rec[:, 117:]).sum()),
                      "model_bytes": i["model_bytes"], "check_ms": stats(check), "apply_ms": stats(app), "kernels_ms": stats(total),
                      "records_per_s": round(n / med * 1e3), "record_gb_per_s": round(n_bytes / med / 1e6, 1),
                      "of_hbm_peak_pct": round(100 * n_bytes / med / 1e6 / HBM_PEAK_GBS, 2)}), flush=True)
    print(json.dumps({"apply_over_count": round(med / float(np.median(count)), 3), "apply_not_slower_than_count": not max(count) < min(total)}),
          flush=True)


if __name__ == "__main__":
    main()
