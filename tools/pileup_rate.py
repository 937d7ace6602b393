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

--tracts (with --indels): the reference has a tract of 8 to 40 bases in every 256 positions, homopolymers and 2-mers by turns, and every
record with an event is moved so that the event lies at a random place inside one: one base in a homopolymer, two in a 2-mer, an
insertion repeating the tract.  The reference is set before the adds.  --leftalign (implies --tracts): the handle left-aligns
(bwams_pileup_set_indel_leftalign), so ms_indel holds the event pass that notes the runs and the align kernel too; the two switches
on the same input are the cost of rule 18.  The indel row also gives ms_indel as a share of all the add's kernels.
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


TRACT_EVERY, TRACT_AT = 256, 64                       # --tracts: a tract in every 256 positions of the reference, from the 64th on


def tract_reference(l_ref: int, seed: int):
    """reference codes uint8[l_ref], random but for a tract of 8 to 40 bases in every block of TRACT_EVERY positions: a homopolymer in
    the even blocks, a 2-mer in the odd ones -> (codes, the tracts' lengths, their two unit codes)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, l_ref, dtype=np.uint8)
    nb = l_ref // TRACT_EVERY
    length = rng.integers(8, 41, nb)
    u0 = rng.integers(0, 4, nb, dtype=np.uint8)
    u1 = np.where(np.arange(nb) % 2 == 0, u0, (u0 + rng.integers(1, 4, nb, dtype=np.uint8)) % 4).astype(np.uint8)
    for j in range(40):
        m = np.flatnonzero(length > j)
        ref[TRACT_EVERY * m + TRACT_AT + j] = (u1 if j % 2 else u0)[m]
    return ref, length, np.stack([u0, u1], 1)


def with_indels(rec: np.ndarray, share: float, seed: int, tracts=None) -> np.ndarray:
    """the records back to back, `share` of them with 75M1I74M or 75M1D75M in place of 150M (three CIGAR words: 8 bytes more).
    tracts (what tract_reference returns): each such record is moved so that its event lies at a random place inside the tract of
    its block, one base in a homopolymer, two in a 2-mer, an insertion repeating the tract in phase: events that rule 18 can move"""
    rng = np.random.default_rng(seed)
    n = len(rec)
    kind, ins = rng.random(n) < share, rng.random(n) < 0.5
    off = np.concatenate([[0], np.cumsum(np.where(kind, 275, 267))])
    out = np.zeros(int(off[-1]), np.uint8)
    cig = {(1, 1): (75, 1, 74), (0, 1): (75, 1, 75), (1, 2): (75, 2, 73), (0, 2): (75, 2, 75)}      # (insertion, length): the three ops
    cig = {k: np.frombuffer(struct.pack("<III", a << 4, b << 4 | (1 if k[0] else 2), c << 4), np.uint8) for k, (a, b, c) in cig.items()}
    for k in range(0, n, 1 << 18):                                                          # in pieces: the scatter indices are 8 bytes a byte
        m = min(n, k + (1 << 18))
        plain, ind = np.flatnonzero(~kind[k:m]) + k, np.flatnonzero(kind[k:m]) + k
        out[(off[plain, None] + np.arange(267)).ravel()] = rec[plain].ravel()
        wide = np.zeros((len(ind), 275), np.uint8)
        wide[:, :38] = rec[ind, :38]
        wide[:, 0:4] = np.frombuffer(struct.pack("<I", 271), np.uint8)
        wide[:, 16] = 3
        wide[:, 38:50] = np.where(ins[ind, None], cig[1, 1], cig[0, 1])
        wide[:, 50:] = rec[ind, 42:]
        if tracts is not None:
            _, length, unit = tracts
            pos = np.ascontiguousarray(wide[:, 8:12]).view("<i4")[:, 0]
            blk = np.clip((pos + 74) // TRACT_EVERY, 1, len(length) - 2)
            two = blk % 2 == 1
            n_ev = np.where(two, 2, 1)
            at = (rng.random(len(ind)) * (length[blk] - n_ev)).astype(np.int64)             # the anchor's place in the tract; the event ends inside it
            wide[:, 8:12] = (TRACT_EVERY * blk + TRACT_AT + at - 74).astype("<i4").view(np.uint8).reshape(-1, 4)
            wide[:, 38:50] = np.where(two[:, None], np.where(ins[ind, None], cig[1, 2], cig[0, 2]), wide[:, 38:50])
            b0, b1 = unit[blk, (at + 1) % 2], unit[blk, (at + 2) % 2]                       # the tract's bases behind the anchor
            i1, i2 = ins[ind], ins[ind] & two
            wide[i1, 50 + 37] = (wide[i1, 50 + 37] & 0xF0) | (1 << b0[i1])                 # query base 75: the low nibble of SEQ byte 37
            wide[i2, 50 + 38] = (wide[i2, 50 + 38] & 0x0F) | (16 << b1[i2])                # query base 76: the high nibble of byte 38
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
    ap.add_argument("--tracts", action="store_true")
    ap.add_argument("--leftalign", action="store_true")
    a = ap.parse_args()
    if (a.tracts or a.leftalign) and not a.indels:
        ap.error("--tracts and --leftalign go with --indels")
    l_ref = int(a.mbp * 1e6)
    n = int(l_ref * a.coverage / 150)
    rec = records(n, l_ref, 11)
    tracts = tract_reference(l_ref, 12) if a.tracts or a.leftalign else None
    if a.indels:
        rec = with_indels(rec, a.indel_share, 13, tracts)
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
        if a.leftalign:
            p.set_indel_leftalign()
        if tracts is not None:                                                              # rule 18 wants the reference before the records
            p.set_ref(0, tracts[0])
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
                              "event_capacity": ii["cap_events"], "leftalign": bool(a.leftalign),
                              "of_the_add_s_kernels_pct": round(100 * float(np.median(indel)) / (float(np.median(indel)) + float(np.median(total))), 1)}),
                  flush=True)
        if a.indels and not tiled:                                                          # the queries: the store is the same either way
            if tracts is None:
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
