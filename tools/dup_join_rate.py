"""Duplicate marking of a coordinate-sorted BAM file on one MI355X (bwams_dupjoin_t): what pass 1, bwams_dupjoin_finish and pass 2
cost beside a plain read of the same file into a depth handle.

The file is tools/bam_query_rate.py's: --records (default 10^6) mapped single-end records of 150M with names of their own, all of
one size, spread over four references of --ref-mb (default 25) each, written with its index by the sorted writer.  Warm, --reps
times, alternating in this process, host clock around calls that end in a synchronise, the file in the page cache:
  pass1   bwams_bam_file_query of the whole file, bwams_bam_file_next and bwams_dupjoin_add_file per piece
  finish  bwams_dupjoin_finish; its phases from bwams_dupjoin_info (the three sorts, head flags to the selects, md_decide and counts)
  pass2   the query again, bwams_bam_file_next and bwams_dupjoin_apply_file per piece
  plain   the query, bwams_bam_file_next and bwams_depth_add_file per piece: what any consumer of the file pays
--once runs one unmeasured round of the three phases and stops: the run to put under a kernel trace.
One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bwams import bam, capi, simulate  # noqa: E402
from bam_query_rate import records_150m, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ref-mb", type=float, default=25.0)
    ap.add_argument("--chunk", type=int, default=250_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--piece-mb", type=int, default=0)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    names = [b"seq%d" % k for k in range(4)]
    l_ref = [int(a.ref_mb * 1e6)] * 4
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", names, l_ref)
    tmp = tempfile.mkdtemp(prefix="dup_join_rate.")
    path = os.path.join(tmp, "sorted.bam")
    ix = capi.Index.build(simulate.make_genome(3000, seed=3, repeat_frac=0.0), 0)
    try:
        s = capi.Sorter(path, 0, hdr, mem_bytes=8 << 30)
        for c, first in enumerate(range(0, a.records, a.chunk)):
            n = min(a.chunk, a.records - first)
            b = capi.Batch(ix, 16, 1000)
            b.bam_upload(records_150m(rng.integers(0, 4, n), rng.integers(0, l_ref[0] - 150, n), first, rng))
            b.bam_sort()
            s.put_batch(c, b)
            b.close()
        st = s.close()
        print(json.dumps({"file": True, "records": st.records, "file_bytes": os.path.getsize(path)}), flush=True)

        f = capi.BamFile(path, piece_bytes=a.piece_mb << 20)
        j = capi.DupJoin()

        def round_of():
            """-> (ms of pass 1, finish, pass 2, the handle's info, the stats, the file's stage times of pass 1)"""
            j.reset()
            t0 = time.perf_counter()
            f.query(())
            n = sum(j.add_file(p) for p in f.pieces())
            t1 = time.perf_counter()
            file_info = f.info()
            t1b = time.perf_counter()
            dst, _ = j.finish()
            t2 = time.perf_counter()
            f.query(())
            marked = sum(j.apply_file(p) for p in f.pieces())
            t3 = time.perf_counter()
            assert n == st.records and marked == dst.records_marked
            return (t1 - t0) * 1e3, (t2 - t1b) * 1e3, (t3 - t2) * 1e3, j.info(), dst, file_info

        def plain():
            d = capi.Depth(l_ref)
            t = time.perf_counter()
            f.query(())
            n = sum(d.add_file(p) for p in f.pieces())
            ms = (time.perf_counter() - t) * 1e3
            d.close()
            assert n <= st.records
            return ms

        _, _, _, info, dst, file_info = round_of()              # warm-up
        if a.once:
            return
        plain()
        t = {"pass1": [], "finish": [], "pass2": [], "plain": []}
        for _ in range(a.reps):
            p1, fin, p2, info, dst, file_info = round_of()
            t["pass1"].append(p1)
            t["finish"].append(fin)
            t["pass2"].append(p2)
            t["plain"].append(plain())
        print(json.dumps({"dup_join": True, "records": info["records"], "templates": info["templates"], "ends": info["ends"],
                          "records_marked": dst.records_marked, "pieces": file_info["pieces"],
                          **{k + "_ms": stats(v) for k, v in t.items()},
                          "finish_phases_ms": {k: round(info[k], 2) for k in ("ms_sort", "ms_ends", "ms_decide")},
                          "kernels_ms": {"add": round(info["ms_add"], 2), "apply": round(info["ms_apply"], 2)},
                          "file_stages_ms_pass1": {k: round(v, 2) for k, v in file_info.items() if k.startswith("ms_")},
                          "entry_bytes": info["entry_bytes"], "hbm_bytes_after_finish": info["hbm_bytes"]}), flush=True)
        j.close()
        f.close()
    finally:
        ix.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
