"""Several sorted BAM files merged on one MI355X (bwams_bam_file_open_merge): what the merged stream into bwams_depth_add_file costs
beside the same files read one after another, which is what a caller had without it.

The files: tools/bam_query_rate.py's records (--records, default 10^6, mapped, 150M, 276 bytes each, over four references of
--ref-mb each) in coordinate order, dealt round-robin into --files (default 4) files, each written with its index by the sorted
writer (bwams_sorter_put, one run).  Warm, --reps times, alternating, host clock around calls that end in a synchronise, both
routes in this process, the files in the page cache:
  A   the merged handle (--piece-mb, default 0: the library's 128 MiB, so child_bytes = piece / files): bwams_bam_file_query of the
      whole file, bwams_bam_file_next and bwams_depth_add_file per piece; the stages from bwams_bam_merge_info and the children's
      sums from bwams_bam_file_info
  B   the yardstick: a plain handle per file with piece_bytes = child_bytes, one file after another, into the same kind of depth handle
Both must count the same records and give the same per-reference sums.  A does strictly more device work than B (check, rank,
scan, a second gather); what it saves is the first refill, where the children's first pieces are inflated concurrently.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bwams import bam, capi  # noqa: E402
from bam_query_rate import records_150m, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ref-mb", type=float, default=25.0)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--piece-mb", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    names = [b"seq%d" % k for k in range(4)]
    l_ref = [int(a.ref_mb * 1e6)] * 4
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", names, l_ref)
    tmp = tempfile.mkdtemp(prefix="bam_merge_rate.")
    try:
        ref, pos = rng.integers(0, 4, a.records), rng.integers(0, l_ref[0] - 150, a.records)
        order = np.lexsort((pos, ref))
        ref, pos = ref[order], pos[order]
        paths = []
        for k in range(a.files):                             # record i of the sorted stream goes to file i mod files
            r, p = ref[k::a.files], pos[k::a.files]
            recs = records_150m(r, p, k * a.records, rng)
            coords = np.zeros(len(r), capi.BAM_COORD_DTYPE)
            coords["key"] = (r.astype(np.uint64) << np.uint64(32)) | ((p.astype(np.uint64) + np.uint64(1)) << np.uint64(1))
            coords["end"] = p + 150
            coords["size"] = len(recs) // len(r)
            paths.append(os.path.join(tmp, "lane%d.bam" % k))
            s = capi.Sorter(paths[-1], 0, hdr, mem_bytes=8 << 30)
            s.put(0, recs, coords)
            s.close()
        print(json.dumps({"files": a.files, "records": a.records, "file_bytes": [os.path.getsize(p) for p in paths]}), flush=True)

        m = capi.BamFile.merge(paths, piece_bytes=a.piece_mb << 20)
        child = m.merge_info()["child_bytes"]
        plain = [capi.BamFile(p, piece_bytes=child) for p in paths]

        def route_a():
            d = capi.Depth(l_ref)
            m.query(())
            n = sum(d.add_file(p) for p in m.pieces())
            return d, n, (m.merge_info(), m.info())

        def route_b():
            d = capi.Depth(l_ref)
            n, ms_inflate = 0, 0.0
            for f in plain:
                f.query(())
                n += sum(d.add_file(p) for p in f.pieces())
                ms_inflate += f.info()["ms_inflate"]
            return d, n, ms_inflate

        sums = []
        for route in (route_a, route_b):                     # warm-up, and the two results against each other
            d, n, _ = route()
            sums.append((n, d.finish().summary()["bases"].tolist()))
            d.close()
        times = {"A": [], "B": []}
        seen = {}
        for _ in range(a.reps):
            for tag, route in (("A", route_a), ("B", route_b)):
                t = time.perf_counter()
                d, n, i = route()
                times[tag].append((time.perf_counter() - t) * 1e3)
                seen[tag] = i
                d.close()
        mi, fi = seen["A"]
        print(json.dumps({"whole_file": True, "files": a.files, "child_bytes": child, "records": sums[0][0], "same_result": sums[0] == sums[1],
                          "A_ms": stats(times["A"]), "B_ms": stats(times["B"]),
                          "A_over_B_median": round(float(np.median(times["A"]) / np.median(times["B"])), 3),
                          "rounds": mi["rounds"], "refills": mi["refills"], "max_piece_records": mi["max_piece_records"],
                          "max_window_left": mi["max_window_left"],
                          "merge_stages_ms": {k: round(v, 2) for k, v in mi.items() if k.startswith("ms_")},
                          "children_ms": {k: round(v, 2) for k, v in fi.items() if k.startswith("ms_")},
                          "B_ms_inflate": round(seen["B"], 2)}), flush=True)
        m.close()
        for f in plain:
            f.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
