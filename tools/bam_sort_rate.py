"""Coordinate-sorted BAM and its index on one MI355X (csrc/bam_sort.hip, host/bam_sort.cpp): the GPU sort's rate and the sorter's.

A simulated genome (--genome-mb, default 100) split into 24 sequences is indexed with Index.from_fasta; --chunks (default 4)
single-end chunks of --reads (default 10^6) reads of 150 bp run through bwams_process_chunk and bwams_bam_run.  Per chunk, warm, --reps
times, host clock around calls that end in a synchronise:
  sort_ms          bwams_bam_sort alone (a bwams_bam_run in front of every repetition, untimed, so that it sorts)
  sorted_fetch_ms  bwams_bam_sorted_fetch of the records and coords to host memory
min / median / max of each, and the alignment (process_chunk) for comparison.  Then every chunk goes to one bwams_sorter
(bwams_sorter_put_batch, BWAMS_SORT_BAI) and the sorter is closed: the put rate, close's merge / deflate / write milliseconds, and
records/s and output MB/s end to end (puts + close).  One JSON line per chunk and one for the sorter on stdout.
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
from bam_rate import fastq, timed  # noqa: E402
from bwams import capi, simulate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=100.0)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mem-bytes", type=int, default=16 << 30)
    a = ap.parse_args()
    g = simulate.make_genome(int(a.genome_mb * 1e6), seed=5)
    cut = np.linspace(0, len(g), 25).astype(np.int64)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    fa = b"".join(b">seq%02d\n" % i + acgt[g[cut[i]:cut[i + 1]]].tobytes() + b"\n" for i in range(24))
    ix = capi.Index.from_fasta(fa, 0)
    hdr = ix.bam_header(ix.sam_header(None, b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n"))
    tmp = tempfile.mkdtemp(prefix="bam_sort_rate.")
    b = capi.Batch(ix, a.reads, a.reads * 150)
    s = capi.Sorter(os.path.join(tmp, "out.bam"), 0, hdr, mem_bytes=a.mem_bytes)
    put_s, recs, bam_bytes = 0.0, 0, 0
    try:
        for c in range(a.chunks):
            reads = simulate.make_read_pairs_bulk(g, (a.reads + 1) // 2, seed=7 + c)[:a.reads]
            text = fastq(reads, 9 + c, False)
            t = time.perf_counter()
            b.process_chunk(text, fetch=False, n_processed=c * a.reads)
            align_ms = (time.perf_counter() - t) * 1e3
            nb, nr = b.bam_run()
            b.bam_sort()
            b.bam_sorted_fetch()                                                 # warm-up of both paths
            sort = []
            for _ in range(a.reps):
                b.bam_run()
                t = time.perf_counter()
                b.bam_sort()
                sort.append((time.perf_counter() - t) * 1e3)
            res = {"chunk": c, "reads": len(reads), "records": nr, "bam_bytes": nb, "align_ms": round(align_ms, 1),
                   "sort_ms": {"min": round(min(sort), 3), "median": round(float(np.median(sort)), 3), "max": round(max(sort), 3)},
                   "sorted_fetch_ms": timed(b.bam_sorted_fetch, a.reps)}
            t = time.perf_counter()
            s.put_batch(c, b)
            dt = time.perf_counter() - t
            put_s += dt
            recs += nr
            bam_bytes += nb
            res["put_batch_ms"] = round(dt * 1e3, 1)
            print(json.dumps(res), flush=True)
        t = time.perf_counter()
        st = s.close()
        close_s = time.perf_counter() - t
        out = {"sorter": True, "chunks": a.chunks, "records": st.records, "bam_bytes": bam_bytes, "out_bytes": st.out_bytes,
               "bai_bytes": os.path.getsize(os.path.join(tmp, "out.bam.bai")), "spilled_runs": st.spilled_runs,
               "put_records_per_s": round(recs / put_s), "put_mb_per_s": round(bam_bytes / put_s / 1e6, 1),
               "close_ms": round(close_s * 1e3, 1), "merge_ms": round(st.ms_merge, 1), "deflate_ms": round(st.ms_deflate, 1),
               "write_ms": round(st.ms_write, 1), "records_per_s": round(recs / (put_s + close_s)),
               "out_mb_per_s": round(st.out_bytes / (put_s + close_s) / 1e6, 1)}
        print(json.dumps(out), flush=True)
    finally:
        s.close()
        b.close()
        ix.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
