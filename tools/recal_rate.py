"""Base recalibration tables on one MI355X (csrc/recal.hip): what an add costs through the LDS kernel, through the plain kernel
alone, and beside the tiled pileup add on the same bytes.

The input has the shape of tools/pileup_rate.py's: coordinate-sorted records of 150M, qualities of 30 and either strand, at
--coverage (default 30) over one reference of --mbp (default 50) million bases, 267 bytes a record.  Here the reference is random
and the reads are copies of it with mismatches planted at --mismatch (default 0.01); known sites are single positions at about one
in --known-every (default 1000).  The records go to bwams_recal_add_records, whose kernels the library times between events
(bwams_recal_info: ms_check, ms_add), once to warm up and --reps times (default 7), first on the default path and then under
BWAMS_RECAL_LDS=0; the upload before the kernels is outside the events.  In the same process bwams_pileup_add_records (tiled, its own
events) takes the same bytes.  One JSON line per measurement on stdout; the last line holds the two comparisons of DESIGN 3.21: the
default add against the tiled pileup add and against the plain kernel, each true only when the faster one's slowest repetition is
below the other's fastest.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bwams import capi  # noqa: E402
from pileup_rate import HBM_PEAK_GBS, stats  # noqa: E402


def records(n: int, ref: np.ndarray, mismatch: float, seed: int):
    """n records of 150M at sorted random positions: uint8[n, 267] (name "r", SEQ the reference but for planted mismatches, QUAL 30),
    and the number of mismatches planted"""
    rng = np.random.default_rng(seed)
    l_ref = len(ref)
    rec = np.zeros((n, 267), np.uint8)
    head = struct.pack("<IiiBBHHHiiii", 263, 0, 0, 2, 60, 4681, 1, 0, 150, -1, -1, 0) + b"r\0" + struct.pack("<I", 150 << 4)
    rec[:, :42] = np.frombuffer(head, np.uint8)
    pos = np.sort(rng.integers(0, l_ref - 150, n)).astype("<i4")
    rec[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    rec[:, 18] = 16 * rng.integers(0, 2, n, dtype=np.uint8)                                 # FLAG: either strand
    code = np.array([1, 2, 4, 8], np.uint8)
    planted = 0
    for k in range(0, n, 1 << 18):                                                          # in pieces: 150 bytes a record
        m = min(n, k + (1 << 18)) - k
        b = ref[pos[k:k + m, None].astype(np.int64) + np.arange(150)]
        hit = rng.random((m, 150), dtype=np.float32) < mismatch
        b = np.where(hit, (b + rng.integers(1, 4, (m, 150), dtype=np.uint8)) & 3, b)
        planted += int(hit.sum())
        c = code[b]
        rec[k:k + m, 42:117] = c[:, 0::2] << 4 | c[:, 1::2]
    rec[:, 117:267] = 30
    return rec, planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=50.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mismatch", type=float, default=0.01)
    ap.add_argument("--known-every", type=int, default=1000)
    a = ap.parse_args()
    l_ref = int(a.mbp * 1e6)
    n = int(l_ref * a.coverage / 150)
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 4, l_ref, dtype=np.uint8)
    known = np.zeros(l_ref // a.known_every, capi.RECAL_SITE_DTYPE)
    known["beg"] = np.sort(rng.choice(l_ref, len(known), replace=False))
    known["end"] = known["beg"] + 1
    rec, planted = records(n, ref, a.mismatch, 11)
    n_bytes = rec.nbytes
    ptr = rec.ctypes.data_as(C.c_void_p)
    L = capi.lib()
    print(json.dumps({"records": n, "bytes": n_bytes, "positions": l_ref, "coverage": a.coverage, "mismatches_planted": planted,
                      "known_sites": len(known)}), flush=True)
    total = {}
    for lds in (1, 0):
        os.environ["BWAMS_RECAL_LDS"] = str(lds)
        capi.debug_reload()
        r = capi.Recal([l_ref])
        r.set_ref(0, ref)
        capi._chk(L.bwams_recal_add_known(r.h, known.ctypes.data_as(C.c_void_p), len(known)), "bwams_recal_add_known")
        cnt = C.c_int64(0)
        check, add = [], []
        for rep in range(a.reps + 1):                                                       # the first is the warm-up
            capi._chk(L.bwams_recal_add_records(r.h, ptr, n_bytes, C.byref(cnt)), "bwams_recal_add_records")
            i = r.info()
            assert i["lds"] == lds
            if rep:
                check.append(i["ms_check"]); add.append(i["ms_add"])
        rg = r.table(0)[0]
        store = i["store_bytes"]
        r.close()
        tag = "lds" if lds else "plain"
        total[tag] = [x + y for x, y in zip(check, add)]
        med = float(np.median(total[tag]))
        print(json.dumps({"recal": tag, "counted": cnt.value, "bases_per_add": i["n_bases"], "observations": int(rg[0]), "errors": int(rg[1]),
                          "store_bytes": store, "check_ms": stats(check), "add_ms": stats(add), "kernels_ms": stats(total[tag]),
                          "records_per_s": round(n / med * 1e3), "record_gb_per_s": round(n_bytes / med / 1e6, 1),
                          "of_hbm_peak_pct": round(100 * n_bytes / med / 1e6 / HBM_PEAK_GBS, 2)}), flush=True)
    del os.environ["BWAMS_RECAL_LDS"]
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
    med = {k: float(np.median(v)) for k, v in total.items()}
    print(json.dumps({"recal_over_pileup": round(med["lds"] / med["pileup"], 3),
                      "recal_not_slower_than_pileup": not max(total["pileup"]) < min(total["lds"]),
                      "lds_over_plain": round(med["lds"] / med["plain"], 3), "lds_below_plain": max(total["lds"]) < min(total["plain"])}),
          flush=True)


if __name__ == "__main__":
    main()
