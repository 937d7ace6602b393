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

--indels: the same input with --indel-share of the records (default 0.1) carrying one I or D of one base in the middle (75M1I74M or
75M1D75M, 275 bytes a record), added to a handle with the indel store (bwams_pileup_set_indels): beside the rows above, the device
time of the indel kernels alone (bwams_pileup_indel_info: ms_indel, the count pass and the event pass) and the events they append;
then, three times after a reset and an add, the host clock around the first bwams_pileup_fetch_span (the scan of the span sums), the
first bwams_pileup_indel_alleles that counts (the sort and the reduction of the events) and the bwams_pileup_indel_calls that counts
(rule 16 over the groups), each of which finds the work of the one before it cached.
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


def with_indels(rec: np.ndarray, share: float, seed: int) -> np.ndarray:
    """the records back to back, `share` of them with 75M1I74M or 75M1D75M in place of 150M (three CIGAR words: 8 bytes more)"""
    rng = np.random.default_rng(seed)
    n = len(rec)
    kind, ins = rng.random(n) < share, rng.random(n) < 0.5
    off = np.concatenate([[0], np.cumsum(np.where(kind, 275, 267))])
    out = np.zeros(int(off[-1]), np.uint8)
    cig_i = np.frombuffer(struct.pack("<III", 75 << 4, 1 << 4 | 1, 74 << 4), np.uint8)
    cig_d = np.frombuffer(struct.pack("<III", 75 << 4, 1 << 4 | 2, 75 << 4), np.uint8)
    for k in range(0, n, 1 << 18):                                                          # in pieces: the scatter indices are 8 bytes a byte
        m = min(n, k + (1 << 18))
        plain, ind = np.flatnonzero(~kind[k:m]) + k, np.flatnonzero(kind[k:m]) + k
        out[(off[plain, None] + np.arange(267)).ravel()] = rec[plain].ravel()
        wide = np.zeros((len(ind), 275), np.uint8)
        wide[:, :38] = rec[ind, :38]
        wide[:, 0:4] = np.frombuffer(struct.pack("<I", 271), np.uint8)
        wide[:, 16] = 3
        wide[:, 38:50] = np.where(ins[ind, None], cig_i, cig_d)
        wide[:, 50:] = rec[ind, 42:]
        out[(off[ind, None] + np.arange(275)).ravel()] = wide.ravel()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=50.0)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--indels", action="store_true")
    ap.add_argument("--indel-share", type=float, default=0.1)
    a = ap.parse_args()
    l_ref = int(a.mbp * 1e6)
    n = int(l_ref * a.coverage / 150)
    rec = records(n, l_ref, 11)
    if a.indels:
        rec = with_indels(rec, a.indel_share, 13)
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
        if a.indels:
            p.set_indels()
        cnt = C.c_int64(0)
        check, add, wall, indel = [], [], [], []
        for rep in range(a.reps + 1):                                                       # the first is the warm-up
            t = time.perf_counter()
            capi._chk(L.bwams_pileup_add_records(p.h, ptr, n_bytes, C.byref(cnt)), "bwams_pileup_add_records")
            w = (time.perf_counter() - t) * 1e3
            i = p.info()
            if rep:
                check.append(i["ms_check"]); add.append(i["ms_add"]); wall.append(w)
                if a.indels:
                    indel.append(p.indel_info()["ms_indel"])
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
        if a.indels:
            ii = p.indel_info()
            print(json.dumps({"indel_kernels_ms": stats(indel), "events_appended": ii["n_appended"], "events_held": ii["n_events"],
                              "event_capacity": ii["cap_events"]}), flush=True)
        if a.indels and not tiled:                                                          # the queries: the store is the same either way
            p.set_ref(0, np.random.default_rng(12).integers(0, 4, l_ref, dtype=np.uint8))
            scan, groups, calls = [], [], []
            n_out = C.c_int64(0)
            one = np.zeros(4, np.uint32)
            for rep in range(3):
                p.reset()
                capi._chk(L.bwams_pileup_add_records(p.h, ptr, n_bytes, C.byref(cnt)), "bwams_pileup_add_records")
                t = time.perf_counter()
                capi._chk(L.bwams_pileup_fetch_span(p.h, 0, 0, 1, one.ctypes.data_as(C.c_void_p)), "bwams_pileup_fetch_span")
                t1 = time.perf_counter()
                capi._chk(L.bwams_pileup_indel_alleles(p.h, None, 0, C.byref(n_out)), "bwams_pileup_indel_alleles")
                t2 = time.perf_counter()
                n_groups = n_out.value
                capi._chk(L.bwams_pileup_indel_calls(p.h, -1, -1, None, 0, C.byref(n_out)), "bwams_pileup_indel_calls")
                t3 = time.perf_counter()
                scan.append((t1 - t) * 1e3); groups.append((t2 - t1) * 1e3); calls.append((t3 - t2) * 1e3)
            print(json.dumps({"indel_calls": n_out.value, "groups": n_groups, "events": p.indel_info()["n_events"], "slots": l_ref,
                              "scan_ms": stats(scan), "sort_and_reduce_ms": stats(groups), "call_count_ms": stats(calls)}), flush=True)
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
