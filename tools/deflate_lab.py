"""BGZF deflate on one MI355X against one zlib level-1 thread (csrc/deflate.hip).

Inputs: SAM-like text (150 bp reads from a random 50 Mbp genome, binned qualities, the usual fields; --sam-mb), simulated FASTQ
(--reads) and the SAM text of bwams_process_chunk over simulated reads (--chunk-reads).  Per input, warm, median of --reps runs:
  kernel_gbs   text bytes / kernel time (the device events around the deflate launches; input and output in HBM)
  copy_gbs     text bytes / wall time of bwams_deflater_run from host memory to host memory (upload, kernels, download)
  zlib1_gbs    text bytes / wall time of one thread writing the same members with zlib level 1
  ratio        text bytes / BGZF bytes, for the device and for zlib level 1
One JSON line per input on stdout.  --quick: 4 MB inputs, 2 runs (for a profiler run).
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
from bwams import bgzf, capi, simulate  # noqa: E402


def sam_like(n_bytes, seed=0, genome_len=50_000_000):
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, genome_len, dtype=np.uint8)]
    n = n_bytes // 370 + 1
    pos = rng.integers(0, genome_len - 150, n)
    quals = np.frombuffer(b"F:,#", np.uint8)[rng.choice(4, (n, 150), p=[0.85, 0.10, 0.04, 0.01])]
    flags, chrs, nm = rng.choice([0, 16], n), rng.integers(1, 23, n), rng.integers(0, 4, n)
    return b"".join(b"r%09d\t%d\tchr%d\t%d\t60\t150M\t*\t0\t0\t%s\t%s\tNM:i:%d\tMD:Z:150\tAS:i:%d\tXS:i:0\n"
                    % (i, flags[i], chrs[i], pos[i] + 1, genome[pos[i]:pos[i] + 150].tobytes(), quals[i].tobytes(), nm[i],
                       150 - 5 * nm[i]) for i in range(n))[:n_bytes]


def fastq_text(n, seed=0, read_len=150):
    rng = np.random.default_rng(seed)
    name = np.frombuffer(b"".join(b"@r%09d\n" % i for i in range(n)), np.uint8).reshape(n, 12)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len), dtype=np.uint8)]
    qual = (rng.integers(0, 41, (n, read_len), dtype=np.uint8) + 33).astype(np.uint8)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0)
    return np.concatenate([name, seq, nl, plus, qual, nl], axis=1).tobytes()


def chunk_sam(n_reads, seed=3):
    """SAM text of bwams_process_chunk over simulated reads of a 2 Mbp genome (several chunks of 20 k reads)."""
    g = simulate.make_genome(2_000_000, seed=seed)
    ix = capi.Index.build(g, 0)
    ix.set_contig_names([b"chr1"])
    rng = np.random.default_rng(seed)
    per = 20_000
    b = capi.Batch(ix, per, per * 160)
    out = []
    for a in range(0, n_reads, per):
        reads, _, _ = simulate.make_reads(g, min(per, n_reads - a), seed=seed + a)
        q = (rng.integers(0, 41, reads.shape) + 33).astype(np.uint8)
        text = b"".join(b"@s%d\n%s\n+\n%s\n" % (a + i, bytes(b"ACGTN"[c] for c in r), q[i].tobytes()) for i, r in enumerate(reads))
        out.append(b.process_chunk(text, n_processed=a)[0])
    b.close()
    ix.close()
    return b"".join(out)


def measure(d, text, reps):
    import torch
    dev_in = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    cap = capi.deflate_bound(len(text))
    dev_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    host_out = capi.pinned_array(cap)
    kern, wall = [], []
    d.run_raw((dev_in.data_ptr(), len(text)), dev_out.data_ptr(), cap, True, True)       # warm
    for _ in range(reps):
        rc, n, st = d.run_raw((dev_in.data_ptr(), len(text)), dev_out.data_ptr(), cap, True, True)
        capi._chk(rc, "bwams_deflater_run")
        kern.append(st.ms_kernel)
        t = time.perf_counter()
        rc, n_h, _ = d.run_raw(text, host_out.ctypes.data, cap)
        wall.append(time.perf_counter() - t)
        capi._chk(rc, "bwams_deflater_run")
    capi.pinned_free(host_out)
    t = time.perf_counter()
    z = bgzf.compress(text, level=1)
    zt = time.perf_counter() - t
    gb = len(text) / 1e9
    return {"bytes": len(text), "members": st.members, "kernel_ms": round(statistics.median(kern), 3),
            "kernel_gbs": round(gb / (statistics.median(kern) / 1e3), 3), "copy_gbs": round(gb / statistics.median(wall), 3),
            "zlib1_gbs": round(gb / zt, 3), "ratio": round(len(text) / n, 3), "zlib1_ratio": round(len(text) / len(z), 3),
            "size_vs_zlib1": round(n / len(z), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sam-mb", type=int, default=256)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunk-reads", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.sam_mb, a.reads, a.chunk_reads, a.reps = 4, 12_000, 20_000, 2
    import torch
    torch.cuda.init()
    d = capi.Deflater(0, 64 << 20)
    for name, make in (("sam_like", lambda: sam_like(a.sam_mb << 20, seed=11)), ("fastq", lambda: fastq_text(a.reads, seed=2)),
                       ("process_chunk_sam", lambda: chunk_sam(a.chunk_reads))):
        r = measure(d, make(), a.reps)
        print(json.dumps({"input": name, **r}), flush=True)
    d.close()


if __name__ == "__main__":
    main()
