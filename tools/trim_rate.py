"""Read trimming on one MI355X (csrc/trim.hip) next to the FASTQ decode in front of it (csrc/fastq.hip).

--reads (default 10^6) paired reads of --len (default 150) bases, the ends interleaved: inserts drawn from a normal distribution
(mean 250, sd 80, at least 40) so that about a tenth are shorter than a read and run into the adapters, 0.5 % substitutions, quality
37 falling over the last bases of some reads.  The FASTQ text lies in device memory.  Warm, --reps (default 5) times each:
  decode_ms    bwams_fastq_decode of the text, device time (the yardstick: unchanged by this tool's subject)
  trim_ms      bwams_fastq_trim of the decoded chunk with the default options, device time (`ms` of the new chunk: T1 to T7, the
               scans and the gather) and trim_wall_ms, the whole call (offsets up, the report back, host offset arrays, stats);
               decode_wall_ms is the decode's whole call, for the same comparison
  trim_all_ms  the same with every step on and both adapters given
  text_ms      bwams_fastq_text of the trimmed chunk, the whole call
The first 2000 reads are also trimmed by bwams/trim.py and compared.  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import capi, trim  # noqa: E402

ADAPTERS = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")


def fastq_text(n_pairs: int, L: int, seed: int) -> bytes:
    """the interleaved FASTQ text of n_pairs simulated pairs, built with numpy as fixed-width records"""
    rng = np.random.default_rng(seed)
    I = np.clip(rng.normal(250, 80, n_pairs).astype(np.int64), 40, None)
    G = rng.integers(0, 4, (n_pairs, 2 * L), dtype=np.uint8)              # the insert's first 2 L bases: beyond that the ends cannot meet
    R = rng.integers(0, 4, (n_pairs, L), dtype=np.uint8)
    k = np.arange(L)[None, :]
    rc2 = 3 - np.take_along_axis(G, np.clip(I[:, None] - 1 - k, 0, 2 * L - 1), axis=1)      # the reverse complement of the insert's last bases
    ends = []
    for e, src in enumerate((G[:, :L], np.where(I[:, None] <= 2 * L, rc2, R))):
        fill = np.concatenate([np.frombuffer(bytes(b"ACGT".index(c) for c in ADAPTERS[e]), np.uint8), rng.integers(0, 4, L, dtype=np.uint8)])
        x = np.where(k < I[:, None], src, fill[np.clip(k - I[:, None], 0, len(fill) - 1)])
        err = rng.random((n_pairs, L)) < 0.005
        x = np.where(err, (x + 1 + rng.integers(0, 3, (n_pairs, L))) % 4, x).astype(np.uint8)
        q = np.full((n_pairs, L), 37, np.uint8)
        bad = rng.integers(0, 30, n_pairs) * (rng.random(n_pairs) < 0.3)
        q[k >= L - bad[:, None]] = 8
        ends.append((x, q))
    n = 2 * n_pairs
    fq = np.empty((n, 12 + L + 3 + L + 1), np.uint8)
    fq[:, 0] = ord("@")
    fq[:, 1] = ord("p")
    fq[:, 2:11] = (np.repeat(np.arange(n_pairs), 2)[:, None] // 10 ** np.arange(8, -1, -1)[None, :]) % 10 + ord("0")
    fq[:, 11] = ord("\n")
    for e in range(2):
        fq[e::2, 12:12 + L] = np.frombuffer(b"ACGT", np.uint8)[ends[e][0]]
        fq[e::2, 15 + L:15 + 2 * L] = ends[e][1] + 33
    fq[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", np.uint8)
    fq[:, -1] = ord("\n")
    return fq.tobytes()


def stat(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    text = fastq_text(a.reads // 2, a.len, 1)
    # the restatement on the first 2000 reads
    head = text[:2000 * (len(text) // (a.reads // 2 * 2))]
    all_on = dict(cut_front=1, adapter1=ADAPTERS[0], adapter2=ADAPTERS[1])
    for kw in ({}, all_on):
        f = capi.Fastq(head)
        t, rep, st = f.trim(capi.trim_opt(**kw), True)
        _, wrep, wst = trim.trim(trim.from_fetch(f.fetch()), trim.Opt(**kw), True)
        assert st == wst and all(np.array_equal(rep[x], wrep[x]) for x in trim.READ_DTYPE.names)
        f.close(); t.close()
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    res = {"reads": a.reads, "len": a.len, "fastq_bytes": len(text)}
    dec, runs = [], {"trim": ([], []), "trim_all": ([], [])}
    txt, dec_wall = [], []
    for rep in range(a.reps + 1):                                          # the first run is the warm-up
        t0 = time.perf_counter()
        f = capi.Fastq(d_text.data_ptr(), 0, len(text))
        if rep:
            dec.append(f.info()["ms"]); dec_wall.append((time.perf_counter() - t0) * 1e3)
        for key, kw in (("trim", {}), ("trim_all", all_on)):
            o = capi.trim_opt(**kw)
            t0 = time.perf_counter()
            t, _, st = f.trim(o, True, report=False)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                runs[key][0].append(t.info()["ms"]); runs[key][1].append(wall)
            res[key + "_stats"] = st
            if key == "trim":
                t0 = time.perf_counter()
                t.text(fetch=False)
                if rep:
                    txt.append((time.perf_counter() - t0) * 1e3)
            t.close()
        f.close()
    res["decode_ms"], res["decode_wall_ms"] = stat(dec), stat(dec_wall)
    for key, (ms, wall) in runs.items():
        res[key + "_ms"], res[key + "_wall_ms"] = stat(ms), stat(wall)
    res["text_ms"] = stat(txt)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
