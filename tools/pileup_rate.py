"""Pileup on one MI355X (csrc/pileup.hip): what an add costs through the tiled path, through the direct kernel alone, and beside
the depth add on the same bytes.

The input is built on the host: coordinate-sorted records of 150M with random bases, qualities of 30 and either strand, at
--coverage (default 30) over one reference of --mbp (default 50) million bases; 267 bytes a record.  They go to
bwams_pileup_add_records, whose kernels the library times between events (bwams_pileup_info: ms_check, ms_add), once to warm up and
--reps times (default 7), tiled and then under BWAMS_PILEUP_TILED=0; the upload before the kernels is outside the events.
bwams_depth_add_records takes the same bytes; it has no events, so its row is the host clock around the call with the upload in it,
next to the same clock around the pileup add: the kernels of the depth add come from a `rocprofv3 --kernel-trace --stats` run of
this tool (--reps 2 is enough for that).  One JSON line per measurement on stdout.

--quality: the same adds with the quality plane on (bwams_pileup_set_quality: four additions per counted base, both planes of a
tile in LDS), tiled and direct, and then, in place of the depth add, bwams_pileup_calls over all the slots against a random
reference: the host clock around the call that counts and the call that fetches.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import capi  # noqa: E402

HBM_PEAK_GBS = 8000.0                                 # MI355X: 8 TB/s


def stats(xs):
    return {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3), "max": round(max(xs), 3)}


def records(n: int, l_ref: int, seed: int) -> np.ndarray:
    """n records of 150M at sorted random positions: uint8[n, 267] (name "r", SEQ random over ACGT, QUAL 30)"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 267), np.uint8)
    head = struct.pack("<IiiBBHHHiiii", 263, 0, 0, 2, 60, 4681, 1, 0, 150, -1, -1, 0) + b"r\0" + struct.pack("<I", 150 << 4)
    rec[:, :42] = np.frombuffer(head, np.uint8)
    pos = np.sort(rng.integers(0, l_ref - 150, n)).astype("<i4")
    rec[:, 8:12] = pos.view(np.uint8).reshape(n, 4)
    rec[:, 18] = 16 * rng.integers(0, 2, n, dtype=np.uint8)                                 # FLAG: either strand
    code = np.array([1, 2, 4, 8], np.uint8)
    for k in range(0, n, 1 << 20):                                                          # in pieces: the random draws are 150 bytes a record
        m = min(n, k + (1 << 20)) - k
        b = code[rng.integers(0, 4, (m, 150), dtype=np.uint8)]
        rec[k:k + m, 42:117] = b[:, 0::2] << 4 | b[:, 1::2]
    rec[:, 117:267] = 30
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=50.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    l_ref = int(a.mbp * 1e6)
    n = int(l_ref * a.coverage / 150)
    rec = records(n, l_ref, 11)
    n_bytes = rec.nbytes
    ptr = rec.ctypes.data_as(C.c_void_p)
    L = capi.lib()
    print(json.dumps({"records": n, "bytes": n_bytes, "positions": l_ref, "coverage": a.coverage}), flush=True)
    out = {}
    for tiled in (1, 0):
        os.environ["BWAMS_PILEUP_TILED"] = str(tiled)
        capi.debug_reload()
        p = capi.Pileup([l_ref])
        if a.quality:
            p.set_quality()
        cnt = C.c_int64(0)
        check, add, wall = [], [], []
        for rep in range(a.reps + 1):                                                       # the first is the warm-up
            t = time.perf_counter()
            capi._chk(L.bwams_pileup_add_records(p.h, ptr, n_bytes, C.byref(cnt)), "bwams_pileup_add_records")
            w = (time.perf_counter() - t) * 1e3
            i = p.info()
            if rep:
                check.append(i["ms_check"]); add.append(i["ms_add"]); wall.append(w)
        total = [x + y for x, y in zip(check, add)]
        depth_at = int(p.fetch(0, l_ref // 2, l_ref // 2 + 1)[0, :8].sum())
        if a.quality and not tiled:                                                         # the calls, once: the planes are the same either way
            p.reset()
            capi._chk(L.bwams_pileup_add_records(p.h, ptr, n_bytes, C.byref(cnt)), "bwams_pileup_add_records")
            p.set_ref(0, np.random.default_rng(12).integers(0, 4, l_ref, dtype=np.uint8))
            count, fetch = [], []
            for rep in range(a.reps + 1):
                t = time.perf_counter()
                n_calls = C.c_int64(0)
                capi._chk(L.bwams_pileup_calls(p.h, -1, -1, None, 0, C.byref(n_calls)), "bwams_pileup_calls")
                t1 = time.perf_counter()
                got = p.calls(cap=n_calls.value)
                t2 = time.perf_counter()
                if rep:
                    count.append((t1 - t) * 1e3); fetch.append((t2 - t1) * 1e3)
            print(json.dumps({"calls": len(got), "slots": l_ref, "count_ms": stats(count), "count_and_fetch_ms": stats(fetch),
                              "slots_per_s": round(l_ref / float(np.median(count)) * 1e3)}), flush=True)
        p.close()
        tag = ("quality_" if a.quality else "") + ("tiled" if tiled else "direct")
        out[tag] = float(np.median(total))
        print(json.dumps({"pileup": tag, "counted": cnt.value, "entries": i["n_entries"], "routed_direct": i["n_direct"],
                          "check_ms": stats(check), "add_ms": stats(add), "kernels_ms": stats(total), "call_ms": stats(wall),
                          "records_per_s": round(n / out[tag] * 1e3), "record_gb_per_s": round(n_bytes / out[tag] / 1e6, 1),
                          "of_hbm_peak_pct": round(100 * n_bytes / out[tag] / 1e6 / HBM_PEAK_GBS, 2),
                          "depth_mid": depth_at // (a.reps + 1)}), flush=True)
    del os.environ["BWAMS_PILEUP_TILED"]
    capi.debug_reload()
    if a.quality:
        print(json.dumps({"tiled_over_direct": round(out["quality_direct"] / out["quality_tiled"], 2)}), flush=True)
        return
    d = capi.Depth([l_ref])
    wall = []
    for rep in range(a.reps + 1):
        t = time.perf_counter()
        capi._chk(L.bwams_depth_add_records(d.h, ptr, n_bytes, None), "bwams_depth_add_records")
        if rep:
            wall.append((time.perf_counter() - t) * 1e3)
    d.close()
    print(json.dumps({"depth": True, "call_ms": stats(wall), "tiled_over_direct": round(out["direct"] / out["tiled"], 2)}), flush=True)


if __name__ == "__main__":
    main()
