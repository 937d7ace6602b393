"""A sorted BAM file read back on one MI355X (bwams_bam_file_*): what the whole file into bwams_depth_add_file costs beside the
route a caller had without it, and what a 1 Mb region query reads and keeps.

The file: --records (default 10^6) mapped records of 150M with names, bases and qualities, all of one size, spread over four
references of --ref-mb (default 25) each, uploaded in chunks (bwams_bam_upload), sorted (bwams_bam_sort) and written with its
index by the sorted writer (bwams_sorter_put_batch, bwams_sorter_close).  Warm, --reps times, alternating, host clock around
calls that end in a synchronise, both routes in this process on this file, the file in the page cache:
  new   bwams_bam_file_query of the whole file, bwams_bam_file_next and bwams_depth_add_file per piece (--piece-mb, default 0: the library's);
        the stages' times from bwams_bam_file_info
  old   the file read, bwams_inflater_run to host memory in calls of 32 MiB of members, bwams_depth_add_records on the whole
        records of each call (its host chain walk, its upload).  The caller's cut at a record boundary is free here because the
        records are of one size; a real caller hops along block_size for it, so this route's time is a lower bound.
Both must count the same records and give the same per-reference sums.  Then the region: 1 Mb in the middle of the second reference,
fetched to the host: the bytes read, inflated and kept, the records seen and kept, and the time.
One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import bam, capi, simulate  # noqa: E402


def stats(xs):
    return {"min": round(min(xs), 2), "median": round(float(np.median(xs)), 2), "max": round(max(xs), 2)}


def records_150m(ref: np.ndarray, pos: np.ndarray, first: int, rng) -> bytes:
    """one mapped record of 150M per (ref, pos): a name of ten digits, random bases and qualities; 276 bytes each"""
    n = len(pos)
    size = 36 + 11 + 4 + 75 + 150
    rec = np.zeros((n, size), np.uint8)
    head = struct.pack("<IiiBBHHHiiii", size - 4, 0, 0, 11, 60, 4681, 1, 0, 150, -1, -1, 0)
    rec[:, :36] = np.frombuffer(head, np.uint8)
    rec[:, 4:8] = ref.astype("<i4").view(np.uint8).reshape(n, 4)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    idx = np.arange(first, first + n, dtype=np.int64)
    rec[:, 36:46] = (idx[:, None] // 10 ** np.arange(9, -1, -1)) % 10 + 48
    rec[:, 47:51] = np.frombuffer(struct.pack("<I", 150 << 4), np.uint8)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n, 150))]
    rec[:, 51:126] = codes[:, 0::2] << 4 | codes[:, 1::2]
    rec[:, 126:276] = rng.integers(2, 42, (n, 150), dtype=np.uint8)
    return rec.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ref-mb", type=float, default=25.0)
    ap.add_argument("--chunk", type=int, default=250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--piece-mb", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    names = [b"seq%d" % k for k in range(4)]
    l_ref = [int(a.ref_mb * 1e6)] * 4
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", names, l_ref)
    tmp = tempfile.mkdtemp(prefix="bam_query_rate.")
    path = os.path.join(tmp, "sorted.bam")
    ix = capi.Index.build(simulate.make_genome(3000, seed=3, repeat_frac=0.0), 0)
    try:
        s = capi.Sorter(path, 0, hdr, mem_bytes=8 << 30)
        size = 0
        for c, first in enumerate(range(0, a.records, a.chunk)):
            n = min(a.chunk, a.records - first)
            recs = records_150m(rng.integers(0, 4, n), rng.integers(0, l_ref[0] - 150, n), first, rng)
            size = len(recs) // n
            b = capi.Batch(ix, 16, 1000)
            b.bam_upload(recs)
            b.bam_sort()
            s.put_batch(c, b)
            b.close()
        st = s.close()
        gz = np.fromfile(path, np.uint8)
        print(json.dumps({"file": True, "records": st.records, "record_bytes": size, "file_bytes": len(gz),
                          "inflated_bytes": len(hdr) + a.records * size}), flush=True)

        f = capi.BamFile(path, piece_bytes=a.piece_mb << 20)
        inf = capi.Inflater(0, 32 << 20, 64 << 20)
        host = np.zeros((64 << 20) + size, np.uint8)
        L = capi.lib()

        def new_route():
            d = capi.Depth(l_ref)
            f.query(())
            n = sum(d.add_file(p) for p in f.pieces())
            return d, n, f.info()

        def old_route():
            d = capi.Depth(l_ref)
            at, have, start, total = 0, 0, len(hdr), 0
            cnt = C.c_int64(0)
            while at < len(gz):
                rc, used, n_out, _ = inf.run_raw((gz.ctypes.data + at, min(32 << 20, len(gz) - at)), host.ctypes.data + have, 64 << 20, False)
                if rc or not used:
                    raise RuntimeError("bwams_inflater_run: %d" % rc)
                at += used
                have += n_out
                whole = start + (have - start) // size * size
                rc = L.bwams_depth_add_records(d.h, C.c_void_p(host.ctypes.data + start), whole - start, C.byref(cnt))
                if rc:
                    raise RuntimeError("bwams_depth_add_records: %d" % rc)
                total += cnt.value
                host[:have - whole] = host[whole:have]
                have, start = have - whole, 0
            return d, total, None

        sums = []
        for route in (new_route, old_route):                 # warm-up, and the two results against each other
            d, n, _ = route()
            sums.append((n, d.finish().summary()["bases"].tolist()))
            d.close()
        times = {"new": [], "old": []}
        info = None
        for _ in range(a.reps):
            for tag, route in (("new", new_route), ("old", old_route)):
                t = time.perf_counter()
                d, n, i = route()
                times[tag].append((time.perf_counter() - t) * 1e3)
                info = i or info
                d.close()
        stages = {k: round(v, 2) for k, v in info.items() if k.startswith("ms_")}
        print(json.dumps({"whole_file": True, "records": sums[0][0], "same_result": sums[0] == sums[1], "new_ms": stats(times["new"]),
                          "old_ms": stats(times["old"]), "new_slowest_below_old_fastest": max(times["new"]) < min(times["old"]),
                          "pieces": info["pieces"], "carried": info["carried"], "candidates": info["candidates"], "stages_ms": stages}), flush=True)

        region = [(1, l_ref[1] // 2, l_ref[1] // 2 + 1_000_000)]
        f.read(region)
        ms = []
        for _ in range(a.reps):
            t = time.perf_counter()
            recs, _ = f.read(region)
            ms.append((time.perf_counter() - t) * 1e3)
        i = f.info()
        print(json.dumps({"region_1mb": True, "ms": stats(ms), "intervals": i["intervals"], "compressed_bytes": i["compressed_bytes"],
                          "inflated_bytes": i["inflated_bytes"], "kept_bytes": len(recs), "records_seen": i["records_seen"],
                          "records_kept": i["records_kept"], "stages_ms": {k: round(v, 2) for k, v in i.items() if k.startswith("ms_")}}),
              flush=True)
        f.close()
        inf.close()
    finally:
        ix.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
