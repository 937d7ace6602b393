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

Then (unless --no-libs) the leg of rules 9-15: the same genome, --chunks chunks of --reads reads with Illumina-style 7-field names
(M:1:FC:<lane>:<tile>:<x>:<y>), 5 % of the pairs copies of the pair before them at x and y offsets within +-150, chunk c aligned with
-R's read group lane<c % 2 + 1>; the table has the two read groups in one library, and d = 100.  Per chunk, as above, on the same
records: the calls of rules 1-8 (templates_ms, markdup_ms) and beside them templates2_ms (bwams_bam_templates2 with the table) and
markdup2_ms (bwams_bam_markdup2: table, d, per-library rows).  Then the sorter's close, alternating BWAMS_SORT_MARKDUP alone (close2_ms)
with bwams_sorter_set_markdup + bwams_sorter_close3 (close3_ms), the rows' counts and the metrics text's size.  JSON lines with
"leg": "libs".
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


HEADER_RG = "@RG\tID:lane1\tLB:lib1\tSM:s\n@RG\tID:lane2\tLB:lib1\tSM:s\n"
DIST = 100


def fastq7(reads: np.ndarray, seed: int, lane: int) -> bytes:
    """fastq() with names M:1:FC:<lane>:<tile>:<x>:<y> (fixed width, pairs sharing a name); every 20th pair is a copy of the pair
    before it, on its tile, at x and y offsets within +-150"""
    n, L = reads.shape
    rng = np.random.default_rng(seed)
    reads = reads.copy()
    pid = np.arange(n // 2)
    tile, x, y = 1101 + pid % 4, 10000 + (pid * 7919) % 80000, 10000 + (pid // 4) % 80000
    cp = pid[19::20]
    reads[2 * cp], reads[2 * cp + 1] = reads[2 * cp - 2], reads[2 * cp - 1]
    tile[cp] = tile[cp - 1]
    dx, dy = rng.integers(-150, 151, len(cp)), rng.integers(-150, 151, len(cp))
    dx[(dx == 0) & (dy == 0)] = 1                                               # never the name of the pair before it
    x[cp], y[cp] = x[cp - 1] + dx, y[cp - 1] + dy
    digits = lambda v, w: (np.repeat(v, 2)[:, None] // 10 ** np.arange(w - 1, -1, -1)[None, :]) % 10 + ord("0")   # noqa: E731
    head = b"@M:1:FC:%d:" % lane
    h = len(head)
    rec = np.empty((n, h + 17 + L + 3 + L + 1), np.uint8)
    rec[:, 0:h] = np.frombuffer(head, np.uint8)
    rec[:, h:h + 4] = digits(tile, 4)
    rec[:, h + 4] = ord(":")
    rec[:, h + 5:h + 10] = digits(x, 5)
    rec[:, h + 10] = ord(":")
    rec[:, h + 11:h + 16] = digits(y, 5)
    rec[:, h + 16] = ord("\n")
    o = h + 17
    rec[:, o:o + L] = np.frombuffer(b"ACGTN", np.uint8)[reads]
    rec[:, o + L:o + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, o + L + 3:o + 2 * L + 3] = np.frombuffer(b"F:,#", np.uint8)[rng.choice(4, (n, L), p=[0.85, 0.10, 0.04, 0.01])]
    rec[:, -1] = ord("\n")
    return rec.tobytes()


def timed(prepare, call, reps):
    out, last = [], None
    for _ in range(reps):
        prepare()
        t = time.perf_counter()
        last = call()
        out.append((time.perf_counter() - t) * 1e3)
    return out, last


def libs_leg(a, g, ix, tmp):
    hdr = ix.bam_header(ix.sam_header(HEADER_RG.encode().rstrip(b"\n"), b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n"))
    table = capi.DupGroups(HEADER_RG)
    bs = []
    try:
        for c in range(a.chunks):
            b = capi.Batch(ix, a.reads, a.reads * 150)
            bs.append(b)
            n = a.reads - a.reads % 2
            reads = simulate.make_read_pairs_bulk(g, n // 2, seed=107 + c)[:n]
            lane = c % 2 + 1
            b.process_chunk(fastq7(reads, 109 + c, lane), paired=True, fetch=False, n_processed=c * a.reads,
                            sopt=capi.default_sam_opt(0, b"lane%d" % lane))
            nb, nr = b.bam_run()
            b.bam_markdup()
            b.bam_markdup2(table, DIST)                                          # warm-up of both paths
            tm, (n_t, n_e) = timed(b.bam_run, b.bam_templates, a.reps)
            md, st = timed(b.bam_run, b.bam_markdup, a.reps)
            tm2, _ = timed(b.bam_run, lambda: b.bam_templates2(table), a.reps)
            md2, (st2, rows) = timed(b.bam_run, lambda: b.bam_markdup2(table, DIST), a.reps)
            b.bam_run()
            row = capi.lib_rows(rows)[0]
            print(json.dumps({"leg": "libs", "chunk": c, "reads": len(reads), "records": nr, "bam_bytes": nb, "templates": n_t,
                              "ends": n_e, "templates_ms": stats(tm), "markdup_ms": stats(md), "templates2_ms": stats(tm2),
                              "markdup2_ms": stats(md2), "ms_decide": round(st.ms_decide, 3), "ms_decide2": round(st2.ms_decide, 3),
                              "pair_duplicates": row["pair_duplicates"], "pair_optical_duplicates": row["pair_optical_duplicates"],
                              "records_marked": st2.records_marked}), flush=True)
        close = {False: [], True: []}
        last = None
        for rep in range(a.close_reps):
            for new in (False, True):
                s = capi.Sorter(os.path.join(tmp, "libs_%d.bam" % new), 0, hdr, mem_bytes=a.mem_bytes, markdup=True)
                if new:
                    s.set_markdup(table, DIST)
                for c, b in enumerate(bs):
                    s.put_batch(c, b)
                t = time.perf_counter()
                st = s.close3() if new else s.close()
                close[new].append((time.perf_counter() - t) * 1e3)
                if new:
                    last = st
        old, new = float(np.median(close[False])), float(np.median(close[True]))
        row = capi.lib_rows(last.lib)[0]
        text = capi.dup_metrics_text(table, last.lib, "tools/markdup_rate.py")
        print(json.dumps({"leg": "libs", "sorter": True, "chunks": a.chunks, "records": last.records, "close2_ms": stats(close[False]),
                          "close3_ms": stats(close[True]), "added_ms": round(new - old, 1), "added_pct": round(100 * (new - old) / old, 2),
                          "ms_decide": round(last.dup.ms_decide, 1), "row": row, "metrics_bytes": len(text)}), flush=True)
    finally:
        for b in bs:
            b.close()
        table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=100.0)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--close-reps", type=int, default=2)
    ap.add_argument("--mem-bytes", type=int, default=16 << 30)
    ap.add_argument("--no-libs", action="store_true", help="skip the leg of rules 9-15")
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
        for b in bs:
            b.close()
        bs = []
        if not a.no_libs:
            libs_leg(a, g, ix, tmp)
    finally:
        for b in bs:
            b.close()
        ix.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
