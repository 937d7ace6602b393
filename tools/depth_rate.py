"""Depth of coverage on one MI355X (csrc/depth.hip, host/bam_sort.cpp's bwams_sorter_set_depth): what the add, the finish, the
queries and the sorter's close cost.

The workload of tools/markdup_rate.py: a simulated genome (--genome-mb, default 100) split into 24 sequences, indexed with
Index.from_fasta; --chunks (default 4) paired-end chunks of --reads (default 10^6) reads of 150 bp through bwams_process_chunk and
bwams_bam_run, each chunk in a batch of its own.  Warm, --reps times, host clock around calls that end in a synchronise:
  add_batch_ms   bwams_depth_add_batch per chunk, beside templates_ms, bwams_bam_templates on the same records (a bwams_bam_run in
                 front of every repetition of the latter, untimed, so that it computes afresh): a pass of similar shape
  finish_ms and each query once (summary, histogram of all references and of one, windows of 1000, runs of the first sequence,
                 the three texts), after all chunks were added
  close_ms       the sorter's close (BWAMS_SORT_BAI) over all chunks without and with bwams_sorter_set_depth, --close-reps times,
                 alternating
  one locus      --reads records of 150M at one place of the first sequence, uploaded, and the same spread over it: add_batch_ms
                 with the folding of equal slots inside a wave and, BWAMS_DEPTH_COMBINE=0, without
--only-add ends after the first chunk's adds (for a profiler run of its own).  One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bam_rate import fastq  # noqa: E402
from bwams import capi, simulate  # noqa: E402


def stats(xs):
    return {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3), "max": round(max(xs), 3)}


def timed(call, reps, prepare=None):
    out, last = [], None
    for _ in range(reps):
        if prepare:
            prepare()
        t = time.perf_counter()
        last = call()
        out.append((time.perf_counter() - t) * 1e3)
    return out, last


def once(call):
    t = time.perf_counter()
    r = call()
    return round((time.perf_counter() - t) * 1e3, 3), r


def records_150m(pos: np.ndarray) -> bytes:
    """one mapped record of 150M per position of the first sequence: no name, no sequence, 41 bytes each"""
    n = len(pos)
    rec = np.zeros((n, 41), np.uint8)
    head = struct.pack("<IiiBBHHHiiii", 37, 0, 0, 1, 60, 4681, 1, 0, 0, -1, -1, 0) + b"\0" + struct.pack("<I", 150 << 4)
    rec[:] = np.frombuffer(head, np.uint8)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    return rec.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=100.0)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--close-reps", type=int, default=2)
    ap.add_argument("--mem-bytes", type=int, default=16 << 30)
    ap.add_argument("--only-add", action="store_true")
    a = ap.parse_args()
    g = simulate.make_genome(int(a.genome_mb * 1e6), seed=5)
    cut = np.linspace(0, len(g), 25).astype(np.int64)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    names = [b"seq%02d" % i for i in range(24)]
    fa = b"".join(b">" + names[i] + b"\n" + acgt[g[cut[i]:cut[i + 1]]].tobytes() + b"\n" for i in range(24))
    ix = capi.Index.from_fasta(fa, 0)
    hdr = ix.bam_header(ix.sam_header(None, b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n"))
    l_ref = np.diff(cut).astype(np.int32)
    tmp = tempfile.mkdtemp(prefix="depth_rate.")
    bs = []
    d = capi.Depth(l_ref)
    try:
        for c in range(1 if a.only_add else a.chunks):
            b = capi.Batch(ix, a.reads, a.reads * 150)
            bs.append(b)
            reads = simulate.make_read_pairs_bulk(g, (a.reads + 1) // 2, seed=7 + c)[:a.reads]
            b.process_chunk(fastq(reads, 9 + c, True), paired=True, fetch=False, n_processed=c * a.reads)
            nb, nr = b.bam_run()
            b.bam_templates()
            n_counted = d.add_batch(b)                                           # warm-up of both paths, and the chunk's one add that stays
            scratch = capi.Depth(l_ref)
            add, _ = timed(lambda: scratch.add_batch(b), a.reps)
            scratch.close()
            tm, _ = timed(b.bam_templates, a.reps, prepare=b.bam_run)
            b.bam_run()
            print(json.dumps({"chunk": c, "reads": len(reads), "records": nr, "bam_bytes": nb, "counted": n_counted,
                              "add_batch_ms": stats(add), "templates_ms": stats(tm)}), flush=True)
        if a.only_add:
            return
        q = {}
        q["finish_ms"], _ = once(d.finish)
        q["summary_ms"], rows = once(d.summary)
        q["hist_all_1024_ms"], h = once(lambda: d.hist(-1, 1024))
        q["hist_one_1024_ms"], _ = once(lambda: d.hist(0, 1024))
        q["windows_1000_ms"], w = once(lambda: d.windows(1000))
        q["runs_seq00_ms"], (rs, _) = once(lambda: d.runs(0, 0, int(l_ref[0])))
        q["text_summary_ms"], t0 = once(lambda: d.text(names, 0))
        q["text_dist_ms"], t1 = once(lambda: d.text(names, 1))
        q["text_windows_1000_ms"], t2 = once(lambda: d.text(names, 2, 1000))
        q.update(positions=int(l_ref.sum()), bases=int(rows["bases"].sum()), max_depth=int(rows["max"].max()), windows=len(w),
                 runs_seq00=len(rs), text_bytes=[len(t0), len(t1), len(t2)], mode_depth=int(np.argmax(h)))
        print(json.dumps({"queries": q}), flush=True)
        close = {False: [], True: []}
        last = None
        for rep in range(a.close_reps):
            for with_depth in (False, True):
                s = capi.Sorter(os.path.join(tmp, "out_%d.bam" % with_depth), 0, hdr, mem_bytes=a.mem_bytes)
                dd = capi.Depth(l_ref) if with_depth else None
                if dd is not None:
                    s.set_depth(dd)
                for c, b in enumerate(bs):
                    s.put_batch(c, b)
                t = time.perf_counter()
                st = s.close()
                close[with_depth].append((time.perf_counter() - t) * 1e3)
                if dd is not None:
                    last = (st, int(dd.finish().summary()["bases"].sum()))
                    dd.close()
        plain, withd = float(np.median(close[False])), float(np.median(close[True]))
        print(json.dumps({"sorter": True, "chunks": a.chunks, "records": last[0].records, "close_ms": stats(close[False]),
                          "close_depth_ms": stats(close[True]), "added_ms": round(withd - plain, 1),
                          "added_pct": round(100 * (withd - plain) / plain, 2), "bases": last[1],
                          "same_bases_as_batches": last[1] == q["bases"]}), flush=True)
        for b in bs[1:]:
            b.close()
        b, bs = bs[0], bs[:1]
        rng = np.random.default_rng(3)
        for tag, pos in (("one_locus", np.full(a.reads, 1000)), ("spread_sorted", np.sort(rng.integers(0, int(l_ref[0]) - 150, a.reads))),
                         ("spread_shuffled", rng.integers(0, int(l_ref[0]) - 150, a.reads))):
            b.bam_upload(records_150m(pos))
            out = {"worst_case": tag, "records": a.reads}
            for combine in (1, 0):
                os.environ["BWAMS_DEPTH_COMBINE"] = str(combine)
                capi.debug_reload()
                scratch = capi.Depth(l_ref)
                scratch.add_batch(b)
                ms, _ = timed(lambda: scratch.add_batch(b), a.reps)
                scratch.close()
                out["add_batch_ms" if combine else "add_batch_no_combine_ms"] = stats(ms)
            del os.environ["BWAMS_DEPTH_COMBINE"]
            capi.debug_reload()
            print(json.dumps(out), flush=True)
    finally:
        d.close()
        for b in bs:
            b.close()
        ix.close()
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
