"""BGZF inflate on one MI355X against one zlib thread (csrc/inflate.hip).

Inputs: 1 M x 150 bp simulated reads as FASTQ (~330 MB) and a synthetic FASTA (--fasta-gb, default 1.0 GB of text), each bgzipped
at levels 1, 6 and 9 (members written by zlib on --threads threads).  Per file, warm, median of --reps runs:
  kernel_gbs   text bytes / summed kernel time (device output: the text stays in HBM)
  copy_gbs     text bytes / wall time of bwams_inflater_run into page-locked host memory (upload, kernel, download, host walk)
  zlib_gbs     text bytes / wall time of one thread inflating the same file (Python's gzip.decompress: zlib's inflate per member)
  reader_*     chunks/s and GB/s of text of bwams_reader_open (zlib) and bwams_reader_open_device on the FASTQ files
One JSON line per file on stdout.  --quick: 100 k reads, 64 MB of FASTA, level 6 only, 2 runs (for a profiler run).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import bgzf, capi  # noqa: E402


def fastq_text(n, seed=0, read_len=150):
    rng = np.random.default_rng(seed)
    name = np.frombuffer(b"".join(b"@r%09d\n" % i for i in range(n)), np.uint8).reshape(n, 12)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len), dtype=np.uint8)]
    qual = (rng.integers(0, 41, (n, read_len), dtype=np.uint8) + 33).astype(np.uint8)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0)
    return np.concatenate([name, seq, nl, plus, qual, nl], axis=1).tobytes()


def fasta_text(n_bytes, seed=1, width=60):
    rng = np.random.default_rng(seed)
    rows = n_bytes // (width + 1)
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (rows, width), dtype=np.uint8)]
    a[rng.random((rows, width), dtype=np.float32) < 0.001] = ord("N")
    return b">chr1 synthetic\n" + np.concatenate([a, np.full((rows, 1), 10, np.uint8)], axis=1).tobytes()


def bgzip(data, level, threads):
    blocks = [data[a:a + bgzf.BLOCK] for a in range(0, len(data), bgzf.BLOCK)]
    with ThreadPoolExecutor(threads) as ex:                   # zlib releases the GIL while it compresses
        parts = list(ex.map(lambda d: bgzf.member(d, level), blocks))
    return b"".join(parts) + bgzf.EOF_MEMBER


class Pinned:
    def __init__(self, n):
        self.p = C.c_void_p()
        capi._chk(capi.lib().bwams_host_alloc(C.c_size_t(n), C.byref(self.p)), "bwams_host_alloc")
        self.n = n

    def close(self):
        capi.lib().bwams_host_free(self.p)


def inflate_all(f, zp, nz, out, cap, on_device):
    """every member of the file (zp: page-locked, nz bytes) through f in calls of max_in bytes: (text bytes, summed kernel ms)"""
    at, n_out, ms_k = 0, 0, 0.0
    while at < nz:
        rc, used, n, st = f.run_raw((zp + at, min(nz - at, MAX_IN)), out + (n_out if on_device else 0), cap - (n_out if on_device else 0),
                                    on_device)
        capi._chk(rc, "bwams_inflater_run")
        assert used > 0
        at += used
        n_out += n
        ms_k += st.ms_kernel
    return n_out, ms_k


def reader_rate(open_fn, path, chunk_bases):
    L = capi.lib()
    t0 = time.perf_counter()
    r = open_fn(path, chunk_bases)
    n, nbytes = 0, 0
    while True:
        tp, nb, nr, nbs = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = L.bwams_reader_next(r, C.byref(tp), C.byref(nb), C.byref(nr), C.byref(nbs))
        if rc == 1:
            break
        capi._chk(rc, "bwams_reader_next")
        n += 1
        nbytes += nb.value
        L.bwams_reader_release(r, tp)
    L.bwams_reader_close(r)
    dt = time.perf_counter() - t0
    return n / dt, nbytes / dt / 1e9


MAX_IN = 32 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--fasta-gb", type=float, default=1.0)
    ap.add_argument("--levels", default="1,6,9")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(32, os.cpu_count() or 1))
    ap.add_argument("--chunk-bases", type=int, default=10_000_000)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.reads, a.fasta_gb, a.levels, a.reps = 100_000, 0.064, "6", 2
    import torch
    torch.cuda.init()
    capi.lib()
    texts = {"fastq": fastq_text(a.reads), "fasta": fasta_text(int(a.fasta_gb * 1e9))}
    tmp = tempfile.mkdtemp(prefix="inflate_lab_")
    f = capi.Inflater(0, MAX_IN, 64 << 20)
    for kind, text in texts.items():
        dev = torch.empty(len(text), dtype=torch.uint8, device="cuda:0")
        host = Pinned(64 << 20)
        for level in (int(x) for x in a.levels.split(",")):
            t0 = time.perf_counter()
            z = bgzip(text, level, a.threads)
            t_comp = time.perf_counter() - t0
            zp = Pinned(len(z))
            C.memmove(zp.p, z, len(z))
            res = dict(file=kind, level=level, text_bytes=len(text), bgzf_bytes=len(z), members=-(-len(text) // bgzf.BLOCK) + 1,
                       compress_s=round(t_comp, 2))
            kern, dev_wall, copy_wall = [], [], []
            for rep in range(a.reps + 1):                       # the first run is the warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n, ms_k = inflate_all(f, zp.p.value, len(z), dev.data_ptr(), len(text), True)
                t1 = time.perf_counter()
                assert n == len(text)
                # host output: into a 64 MiB page-locked buffer, call after call
                at, m = 0, 0
                t2 = time.perf_counter()
                while at < len(z):
                    rc, used, nn, _ = f.run_raw((zp.p.value + at, min(len(z) - at, MAX_IN)), host.p.value, host.n, False)
                    capi._chk(rc, "bwams_inflater_run")
                    at += used
                    m += nn
                t3 = time.perf_counter()
                assert m == len(text)
                if rep:
                    kern.append(ms_k / 1e3)
                    dev_wall.append(t1 - t0)
                    copy_wall.append(t3 - t2)
            if level == 6 or a.quick:                            # the device output is the text, byte for byte
                assert bytes(dev[:1 << 20].cpu().numpy()) == text[:1 << 20] and bytes(dev[-(1 << 20):].cpu().numpy()) == text[-(1 << 20):]
            zl = []
            for rep in range(min(a.reps, 3)):
                t0 = time.perf_counter()
                assert len(gzip.decompress(z)) == len(text)
                zl.append(time.perf_counter() - t0)
            med = statistics.median
            res.update(kernel_gbs=round(len(text) / med(kern) / 1e9, 2), device_out_wall_gbs=round(len(text) / med(dev_wall) / 1e9, 2),
                       copy_gbs=round(len(text) / med(copy_wall) / 1e9, 2), zlib_gbs=round(len(text) / med(zl) / 1e9, 3),
                       kernel_s=[round(x, 4) for x in kern], copy_s=[round(x, 4) for x in copy_wall], zlib_s=[round(x, 3) for x in zl])
            if kind == "fastq":
                path = os.path.join(tmp, f"reads.{level}.fq.bgz")
                open(path, "wb").write(z)
                hr = [reader_rate(lambda p, cb: _host_open(p, cb), path, a.chunk_bases) for _ in range(min(a.reps, 3))]
                dr = [reader_rate(lambda p, cb: capi.reader_open_device(p, 0, cb, False, 0, 2), path, a.chunk_bases)
                      for _ in range(min(a.reps, 3))]
                res.update(chunk_bases=a.chunk_bases, reader_host_chunks_s=round(med([x[0] for x in hr]), 2),
                           reader_host_gbs=round(med([x[1] for x in hr]), 3), reader_device_chunks_s=round(med([x[0] for x in dr]), 2),
                           reader_device_gbs=round(med([x[1] for x in dr]), 3))
                os.remove(path)
            zp.close()
            print(json.dumps(res), flush=True)
        host.close()
        del dev
    f.close()


def _host_open(path, chunk_bases):
    r = C.c_void_p()
    capi._chk(capi.lib().bwams_reader_open(path.encode(), C.c_int64(chunk_bases), 0, C.c_int64(0), 2, C.byref(r)), "bwams_reader_open")
    return r


if __name__ == "__main__":
    main()
