"""SAM text to BAM on one MI355X (csrc/bam.hip): the conversion's rate next to the BGZF of the text it replaces.

A simulated genome (--genome-mb, default 100) is indexed with Index.from_fasta; one single-end chunk (--se-reads, default 10^6 x 150 bp)
and one paired-end chunk (--pairs, default 5 x 10^5) run through bwams_process_chunk.  Then, warm, --reps times each, host clock
around calls that end in a synchronise:
  bam_ms        bwams_bam_run + bwams_bam_fetch (records to host memory)
  bam_run_ms    bwams_bam_run alone (records stay in HBM)
  bam_bgzf_ms   bwams_bam_fetch_bgzf after one bwams_bam_run (BGZF members of the records to host memory)
  sam_bgzf_ms   bwams_sam_fetch_bgzf (BGZF of the SAM text, for comparison)
min / median / max of each, and the sizes: SAM text, BAM records, and both as BGZF.  One JSON line per chunk on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import capi, simulate  # noqa: E402


def fastq(reads: np.ndarray, seed: int, pair_names: bool) -> bytes:
    """fixed-width FASTQ records of uint8[n, L] reads, built with numpy (names r%09d, pairs sharing a name)"""
    n, L = reads.shape
    rng = np.random.default_rng(seed)
    ids = np.arange(n) // 2 if pair_names else np.arange(n)
    digits = (ids[:, None] // 10 ** np.arange(8, -1, -1)[None, :]) % 10 + ord("0")
    rec = np.empty((n, 12 + L + 3 + L + 1), np.uint8)
    rec[:, 0:2] = np.frombuffer(b"@r", np.uint8)
    rec[:, 2:11] = digits
    rec[:, 11] = ord("\n")
    rec[:, 12:12 + L] = np.frombuffer(b"ACGTN", np.uint8)[reads]
    rec[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 15 + L:15 + 2 * L] = np.frombuffer(b"F:,#", np.uint8)[rng.choice(4, (n, L), p=[0.85, 0.10, 0.04, 0.01])]
    rec[:, -1] = ord("\n")
    return rec.tobytes()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"min": round(min(out), 3), "median": round(statistics.median(out), 3), "max": round(max(out), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=100.0)
    ap.add_argument("--se-reads", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    g = simulate.make_genome(int(a.genome_mb * 1e6), seed=5)
    fa = b">chr1\n" + np.frombuffer(b"ACGT", np.uint8)[g].tobytes() + b"\n"
    ix = capi.Index.from_fasta(fa, 0)
    d = capi.Deflater(0, 64 << 20)
    for name, paired, n in (("se", False, a.se_reads), ("pe", True, a.pairs)):
        reads = simulate.make_read_pairs_bulk(g, (n + 1) // 2 if not paired else n, seed=7)[: n if not paired else 2 * n]
        text = fastq(reads, 9, paired)
        b = capi.Batch(ix, len(reads), len(reads) * reads.shape[1])
        sam_bytes = b.process_chunk(text, paired=paired, fetch=False)
        nb, nr = b.bam_run()
        b.bam_fetch()
        bam_gz, sam_gz = b.bam_fetch_bgzf(d), b.sam_fetch_bgzf(d)            # warm-up of every path
        res = {"chunk": name, "reads": len(reads), "records": nr, "sam_bytes": sam_bytes, "bam_bytes": nb,
               "sam_bgzf_bytes": len(sam_gz), "bam_bgzf_bytes": len(bam_gz)}
        res["bam_ms"] = timed(lambda: (b.bam_run(), b.bam_fetch()), a.reps)
        res["bam_run_ms"] = timed(b.bam_run, a.reps)
        res["bam_bgzf_ms"] = timed(lambda: b.bam_fetch_bgzf(d), a.reps)
        res["sam_bgzf_ms"] = timed(lambda: b.sam_fetch_bgzf(d), a.reps)
        print(json.dumps(res), flush=True)
        b.close()
    d.close()
    ix.close()


if __name__ == "__main__":
    main()
