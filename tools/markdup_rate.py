"""Duplicate marking on one MI355X (csrc/markdup.hip, host/bam_sort.cpp's BWAMS_SORT_MARKDUP): the batch passes' rates and what
marking adds to the sorter's close.

A simulated genome (--genome-mb, default 100) split into 24 sequences is indexed with Index.from_fasta; --chunks (default 4)
paired-end chunks of --reads (default 10^6) reads of 150 bp run through bwams_process_chunk and bwams_bam_run, each chunk in a batch of
its own.  Per chunk, warm, --reps times, host clock around calls that end in a synchronise (a bwams_bam_run in front of every
repetition, untimed, so that the templates are computed afresh):
  templates_ms  bwams_bam_templates alone
  markdup_ms    bwams_bam_markdup (templates, decision, marking of the unsorted records)
min / median / max of each.  Then every chunk goes to a bwams_sorter (bwams_sorter_put_batch, BWAMS_SORT_BAI), --close-reps times with
and without BWAMS_SORT_MARKDUP, alternating, and close is timed: close_ms of each, their difference, and the marking's ms_decide and
counts.  One JSON line per chunk and one for the sorter on stdout.
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
from bam_rate import fastq  # noqa: E402
from bwams import capi, simulate  # noqa: E402


def stats(xs):
    return {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=100.0)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--close-reps", type=int, default=2)
    ap.add_argument("--mem-bytes", type=int, default=16 << 30)
    a = ap.parse_args()
    g = simulate.make_genome(int(a.genome_mb * 1e6), seed=5)
    cut = np.linspace(0, len(g), 25).astype(np.int64)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    fa = b"".join(b">seq%02d\n" % i + acgt[g[cut[i]:cut[i + 1]]].tobytes() + b"\n" for i in range(24))
    ix = capi.Index.from_fasta(fa, 0)
    hdr = ix.bam_header(ix.sam_header(None, b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n"))
    tmp = tempfile.mkdtemp(prefix="markdup_rate.")
    bs = []
    try:
        for c in range(a.chunks):
            b = capi.Batch(ix, a.reads, a.reads * 150)
            bs.append(b)
            reads = simulate.make_read_pairs_bulk(g, (a.reads + 1) // 2, seed=7 + c)[:a.reads]
            b.process_chunk(fastq(reads, 9 + c, True), paired=True, fetch=False, n_processed=c * a.reads)
            nb, nr = b.bam_run()
            b.bam_templates()
            b.bam_markdup()                                                      # warm-up of both paths
            tm, md = [], []
            for _ in range(a.reps):
                b.bam_run()
                t = time.perf_counter()
                n_t, n_e = b.bam_templates()
                tm.append((time.perf_counter() - t) * 1e3)
                b.bam_run()
                t = time.perf_counter()
                st = b.bam_markdup()
                md.append((time.perf_counter() - t) * 1e3)
            b.bam_run()
            print(json.dumps({"chunk": c, "reads": len(reads), "records": nr, "bam_bytes": nb, "templates": n_t, "ends": n_e,
                              "templates_ms": stats(tm), "markdup_ms": stats(md), "ms_decide": round(st.ms_decide, 3),
                              "records_marked": st.records_marked}), flush=True)
        close = {False: [], True: []}
        last = None
        for rep in range(a.close_reps):
            for flag in (False, True):
                s = capi.Sorter(os.path.join(tmp, "out_%d.bam" % flag), 0, hdr, mem_bytes=a.mem_bytes, markdup=flag)
                for c, b in enumerate(bs):
                    s.put_batch(c, b)
                t = time.perf_counter()
                st = s.close()
                close[flag].append((time.perf_counter() - t) * 1e3)
                if flag:
                    last = st
        plain, marked = float(np.median(close[False])), float(np.median(close[True]))
        d = last.dup
        print(json.dumps({"sorter": True, "chunks": a.chunks, "records": last.records, "close_ms": stats(close[False]),
                          "close_markdup_ms": stats(close[True]), "added_ms": round(marked - plain, 1),
                          "added_pct": round(100 * (marked - plain) / plain, 2), "ms_decide": round(d.ms_decide, 1),
                          "templates": d.templates, "pairs_examined": d.pairs_examined, "pair_duplicates": d.pair_duplicates,
                          "unpaired_examined": d.unpaired_examined, "unpaired_duplicates": d.unpaired_duplicates,
                          "records_marked": d.records_marked}), flush=True)
    finally:
        for b in bs:
            b.close()
        ix.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
