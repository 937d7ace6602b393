"""BAM records to reads on one MI355X (csrc/bam_reads.hip) next to FASTQ text to reads (csrc/fastq.hip), and the BAM reader next to
the BGZF FASTQ reader.

--reads (default 10^6) reads of --len (default 150) bases, half of them reverse, one in 20 records secondary, every record with an
RG:Z and an NM:C field, are built as BAM records with numpy; to_fastq of them is the FASTQ text of the same reads.  Both lie in
device memory.  Warm, --reps (default 5) times each:
  bam_ms          bwams_bam_reads_decode, device time, split into discover_ms (filter, ranks, successors, lifting) and emit_ms
                  (measure, scans, emit); candidates = offsets that passed the filter
  bam_tags_ms     the same with tags "RGNM" (comments made)
  fastq_ms        bwams_fastq_decode of the FASTQ text, device time (the yardstick: unchanged by this tool's subject)
Then both as files at BGZF level 6, drained through bwams_reader_open_bam and bwams_reader_open_device with --chunk-bases per
chunk, --reps times after a first pass: chunks per second, inflated MB per second.  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import bam, bam_reads, bgzf, capi  # noqa: E402


def records(n: int, L: int, seed: int) -> bytes:
    """n fixed-width BAM records (names r%09d, l_seq L, no CIGAR, RG:Z:grp1 and NM:C) as one numpy array"""
    rng = np.random.default_rng(seed)
    aux = b"RGZgrp1\0NMC\0"
    body = 32 + 11 + (L + 1) // 2 + L + len(aux)
    rec = np.zeros((n, 4 + body), np.uint8)
    rec[:, 0:4] = np.frombuffer(np.uint32(body).tobytes(), np.uint8)
    rec[:, 4:12] = 0xFF                                                        # refID, POS = -1
    rec[:, 12] = 11                                                            # l_read_name
    rec[:, 14:16] = np.frombuffer(np.uint16(4680).tobytes(), np.uint8)
    flag = (4 | np.where(rng.random(n) < 0.5, 0x10, 0) | np.where(rng.random(n) < 0.05, 0x100, 0)).astype(np.uint16)
    rec[:, 18:20] = flag.view(np.uint8).reshape(n, 2)
    rec[:, 20:24] = np.frombuffer(np.int32(L).tobytes(), np.uint8)
    rec[:, 24:32] = 0xFF
    rec[:, 36] = ord("r")
    rec[:, 37:46] = (np.arange(n)[:, None] // 10 ** np.arange(8, -1, -1)[None, :]) % 10 + ord("0")
    nib = rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), (n, (L + 1) // 2 * 2), p=[0.2475, 0.2475, 0.2475, 0.2475, 0.01])
    if L & 1:
        nib[:, -1] = 0
    s = 47
    rec[:, s:s + (L + 1) // 2] = nib[:, 0::2] << 4 | nib[:, 1::2]
    s += (L + 1) // 2
    rec[:, s:s + L] = np.array([37, 25, 11, 2], np.uint8)[rng.choice(4, (n, L), p=[0.85, 0.10, 0.04, 0.01])]
    s += L
    rec[:, s:s + len(aux)] = np.frombuffer(aux, np.uint8)
    rec[:, s + len(aux) - 1] = rng.integers(0, 12, n)
    return rec.tobytes()


def stat(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def drain(r):
    t = time.perf_counter()
    chunks = capi.reader_chunks(r)
    dt = time.perf_counter() - t
    nb = sum(len(c[0]) for c in chunks)
    return {"chunks": len(chunks), "reads": sum(c[1] for c in chunks), "s": round(dt, 3), "chunks_per_s": round(len(chunks) / dt, 2),
            "inflated_MB_per_s": round(nb / dt / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-bases", type=int, default=10_000_000)
    ap.add_argument("--no-reader", action="store_true")
    a = ap.parse_args()
    recs = records(a.reads, a.len, 1)
    text = bam_reads.to_fastq(recs[:(len(recs) // a.reads) * 1000])            # the restatement on the first 1000 records, for a check
    d_bam = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to("cuda:0")
    f = capi.bam_reads_decode(0, d_bam.data_ptr(), n_bytes=len(recs))
    got = f.fetch()
    f.close()
    assert capi.Fastq(text).fetch()["names"] == got["names"][:len(text.split(b"\n")) // 4]
    # the FASTQ text of all reads, from the decoded arrays (to_fastq in Python would take minutes)
    n, L = got["n"], a.len
    fq = np.empty((n, 12 + L + 3 + L + 1), np.uint8)
    fq[:, 0] = ord("@")
    fq[:, 1:11] = np.frombuffer(b"".join(got["names"]), np.uint8).reshape(n, 10)
    fq[:, 11] = ord("\n")
    fq[:, 12:12 + L] = np.frombuffer(b"ACGTN", np.uint8)[got["enc"].reshape(n, L)]
    fq[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", np.uint8)
    fq[:, 15 + L:15 + 2 * L] = got["quals"].reshape(n, L)
    fq[:, -1] = ord("\n")
    text = fq.tobytes()
    d_fq = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    res = {"records": a.reads, "reads": n, "len": L, "bam_bytes": len(recs), "fastq_bytes": len(text)}
    for key, tags in (("bam", b""), ("bam_tags", b"RGNM")):
        tot, dis, emi = [], [], []
        for rep in range(a.reps + 1):
            f = capi.bam_reads_decode(0, d_bam.data_ptr(), tags, n_bytes=len(recs))
            i = capi.bam_reads_info(f)
            f.close()
            if rep:                                                           # the first run is the warm-up
                dis.append(i["ms_discover"]); emi.append(i["ms_emit"]); tot.append(i["ms_discover"] + i["ms_emit"])
        res[key + "_ms"], res[key + "_discover_ms"], res[key + "_emit_ms"] = stat(tot), stat(dis), stat(emi)
        res["candidates"] = i["n_candidates"]
    ms = []
    for rep in range(a.reps + 1):
        f = capi.Fastq(d_fq.data_ptr(), 0, len(text))
        if rep:
            ms.append(f.info()["ms"])
        f.close()
    res["fastq_ms"] = stat(ms)
    if not a.no_reader:
        with tempfile.TemporaryDirectory() as d:
            hdr = bam.header_block(b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:grp1\n", [], [])
            with open(os.path.join(d, "in.bam"), "wb") as fp:
                fp.write(bgzf.compress(hdr + recs, 6))
            with open(os.path.join(d, "in.fq.gz"), "wb") as fp:
                fp.write(bgzf.compress(text, 6))
            res["bam_file_bytes"], res["fastq_file_bytes"] = os.path.getsize(os.path.join(d, "in.bam")), os.path.getsize(os.path.join(d, "in.fq.gz"))
            runs = {"reader_bam": [], "reader_fastq": []}
            for rep in range(a.reps + 1):                                     # the first pass warms the page cache
                b_ = drain(capi.reader_open_bam(os.path.join(d, "in.bam"), 0, a.chunk_bases, False, 0, 2))
                f_ = drain(capi.reader_open_device(os.path.join(d, "in.fq.gz"), 0, a.chunk_bases, False, 0, 2))
                if rep:
                    runs["reader_bam"].append(b_); runs["reader_fastq"].append(f_)
            for k, v in runs.items():
                res[k] = {"chunks": v[0]["chunks"], "reads": v[0]["reads"], "chunks_per_s": stat([x["chunks_per_s"] for x in v]),
                          "inflated_MB_per_s": stat([x["inflated_MB_per_s"] for x in v])}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
