"""BAM records viewed as SAM text on one MI355X (bwams_samview_t): what the two passes cost per million records, what a whole add
costs from host records and from a BAM file's pieces, and bwams_bam_run on the same records' text beside it.

--records (default 10^6) mapped paired records of 150M, all of one size (276 bytes, tools/collate_rate.py's input), in coordinate
order on one reference of --ref-mb (default 100).  Warm, --reps times:
  add_records_ms  host clock around one bwams_samview_add_records of all of them: the host's chain walk and the upload included
  count_ms, write_ms  device time between events of that add, from bwams_samview_info: the counting pass with its scan, the writing pass
  add_file_ms     host clock around bwams_bam_file_query and, piece by piece, bwams_bam_file_next + bwams_samview_add_file over the
                  same records written by the sorted writer; view_in_file_ms is the two passes' device time inside it
The first 2000 lines are compared with bwams/samview.py.
For context, the inverse: --pairs (default 100000) simulated 150 bp pairs on a --genome-mb (default 20) genome go through
bwams_process_chunk; then, warm,
  bam_run_ms      host clock around bwams_bam_run (line ends, bam_count_kernel, a scan, bam_write_kernel; its kernels by name come
                  from a kernel trace of this tool, profiles/samview.md)
  view_batch      count_ms and write_ms of bwams_samview_add_batch on the records bam_run made: the same records, the other way
--once runs every path once, unmeasured, and stops: the run to put under a kernel trace.  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bwams import bam, capi, samview, simulate  # noqa: E402
from bam_query_rate import stats  # noqa: E402
from bam_rate import fastq  # noqa: E402
from collate_rate import sorted_pairs  # noqa: E402


def med(xs) -> float:
    return round(float(np.median(xs)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ref-mb", type=float, default=100.0)
    ap.add_argument("--chunk", type=int, default=250_000)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--genome-mb", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    reps = 1 if a.once else a.reps
    l_ref = int(a.ref_mb * 1e6)
    names = [b"seq0"]
    hdr = bam.header_block(b"@HD\tVN:1.6\tSO:coordinate\n", names, [l_ref])
    rec = sorted_pairs(a.records, l_ref, 0.02, 7)
    data = rec.tobytes()
    per_m = 1e6 / len(rec)
    v = capi.SamView(hdr)
    res = {"samview": True, "records": len(rec), "record_bytes": 276}

    def delta(fn):
        """fn(), and what it added to the two passes' device time"""
        i0 = v.info()
        t = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t) * 1e3
        i1 = v.info()
        return ms, i1["ms_count"] - i0["ms_count"], i1["ms_write"] - i0["ms_write"]

    # host records, one add
    assert v.add_records(data[:2000 * 276]) == 2000
    assert v.fetch()[0] == samview.view(data[:2000 * 276], names)[0]
    v.add_records(data)                                      # warm-up
    res["text_bytes"] = v.out().n_bytes
    runs = [delta(lambda: v.add_records(data)) for _ in range(reps)]
    res["add_records_ms"] = stats([r[0] for r in runs])
    res["count_ms"], res["write_ms"] = med([r[1] for r in runs]), med([r[2] for r in runs])
    res["passes_ms_per_million"] = round((res["count_ms"] + res["write_ms"]) * per_m, 3)
    res["write_GB_per_s"] = round(res["text_bytes"] / max(res["write_ms"], 1e-6) / 1e6, 1)

    # the same records from a sorted file, piece by piece
    tmp = tempfile.mkdtemp(prefix="samview_rate.")
    path = os.path.join(tmp, "sorted.bam")
    ix = capi.Index.build(simulate.make_genome(3000, seed=3, repeat_frac=0.0), 0)
    s = capi.Sorter(path, 0, hdr, mem_bytes=8 << 30)
    for c, first in enumerate(range(0, len(rec), a.chunk)):
        b = capi.Batch(ix, 16, 1000)
        b.bam_upload(rec[first:first + a.chunk].tobytes())
        b.bam_sort()
        s.put_batch(c, b)
        b.close()
    s.close()
    ix.close()
    f = capi.BamFile(path)
    lines = [0]

    def file_round():
        f.query(())
        lines[0] = sum(v.add_file(p) for p in f.pieces())

    file_round()                                             # warm-up
    assert lines[0] == len(rec)
    runs = [delta(file_round) for _ in range(reps)]
    res["add_file_ms"] = stats([r[0] for r in runs])
    res["view_in_file_ms"] = med([r[1] + r[2] for r in runs])
    res["pieces"] = f.info()["pieces"]
    f.close()
    v.close()
    os.remove(path)
    if os.path.exists(path + ".bai"):
        os.remove(path + ".bai")
    os.rmdir(tmp)

    # the inverse on the same records: bwams_bam_run, then the view of what it made
    g = simulate.make_genome(int(a.genome_mb * 1e6), seed=5)
    fa = b">chr1\n" + np.frombuffer(b"ACGT", np.uint8)[g].tobytes() + b"\n"
    ix = capi.Index.from_fasta(fa, 0)
    reads = simulate.make_read_pairs_bulk(g, a.pairs, seed=7)[:2 * a.pairs]
    b = capi.Batch(ix, len(reads), len(reads) * reads.shape[1])
    sam_bytes = b.process_chunk(fastq(reads, 9, True), paired=True, fetch=False)
    nb, nr = b.bam_run()                                     # warm-up
    v = capi.SamView(ix.bam_header(b"@HD\tVN:1.6\n"))
    assert v.add_batch(b) == nr and v.out().n_bytes == sam_bytes
    bam_ms = []
    for _ in range(reps):
        t = time.perf_counter()
        b.bam_run()
        bam_ms.append((time.perf_counter() - t) * 1e3)
    runs = [delta(lambda: v.add_batch(b)) for _ in range(reps)]
    m = 1e6 / nr
    view_ms = med([r[1] for r in runs]) + med([r[2] for r in runs])
    res["batch"] = {"records": nr, "sam_bytes": sam_bytes, "bam_bytes": nb, "text_over_bam": round(sam_bytes / nb, 3),
                    "bam_run_ms": stats(bam_ms), "bam_run_ms_per_million": round(float(np.median(bam_ms)) * m, 3),
                    "view_count_ms": med([r[1] for r in runs]), "view_write_ms": med([r[2] for r in runs]),
                    "view_passes_ms_per_million": round(view_ms * m, 3),
                    "view_over_bam_run": round(view_ms / float(np.median(bam_ms)), 3)}
    v.close()
    b.close()
    ix.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
