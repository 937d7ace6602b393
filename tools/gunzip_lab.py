"""Plain gzip inflated on one MI355X against one zlib thread (csrc/gunzip.hip).

Inputs: --reads x 150 bp simulated reads as FASTQ (1 M: ~316 MB) and a synthetic FASTA (--fasta-gb of text), each one gzip member at
--level (zlib, as `gzip -6` writes it).  Per file, warm, median of --reps runs:
  gbs_*            text bytes / summed time of each kernel (find, count, decode, window, resolve), and of all five
  call_gbs         text bytes / wall time of bwams_gunzip_run into page-locked host memory, calls of --call-mib of gzip
  zlib_gbs         text bytes / ms_inflate of bwams_reader_open on the same file: the one zlib thread this replaces
  bgzf_kernel_gbs  text bytes / kernel time of bwams_inflater_run on the BGZF of the same text: the ceiling the decoder shares
  reader_*         GB/s of text of bwams_reader_open_device2 without and with BWAMS_READER_GUNZIP (FASTQ only)
One JSON line per file on stdout.  --quick: 100 k reads, 64 MB of FASTA, 2 runs (for a profiler run:
rocprofv3 --kernel-trace --stats -- python tools/gunzip_lab.py --quick gives the split between the five kernels).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bwams import capi  # noqa: E402
from inflate_lab import Pinned, bgzip, fasta_text, fastq_text, reader_rate  # noqa: E402

KERNELS = ("find", "count", "decode", "window", "resolve")


def gunzip_all(g_args, zp, nz, out, cap, on_device, call):
    """the whole file (zp: page-locked, nz bytes) through a fresh handle: (text bytes, summed ms per kernel, pieces, dropped)"""
    g = capi.Gunzipper(*g_args)
    pos, end, n_out, ms, pieces, dropped = 0, 0, 0, dict.fromkeys(KERNELS, 0.0), 0, 0
    while pos < nz:
        end = min(max(end, pos) + call, nz)
        rc, used, n, st = g.run_raw((zp + pos, end - pos), end == nz, out + (n_out if on_device else 0),
                                    cap - (n_out if on_device else 0), on_device)
        capi._chk(rc, "bwams_gunzip_run")
        pos += used
        n_out += n
        pieces += st.pieces
        dropped += st.pieces_dropped
        for k in KERNELS:
            ms[k] += getattr(st, "ms_" + k)
    g.close()
    return n_out, ms, pieces, dropped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--fasta-gb", type=float, default=0.25)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--call-mib", type=int, default=32)
    ap.add_argument("--piece-kib", type=int, default=32)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--chunk-bases", type=int, default=10_000_000)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.reads, a.fasta_gb, a.reps = 100_000, 0.064, 2
    import torch
    torch.cuda.init()
    capi.lib()
    med = statistics.median
    call = a.call_mib << 20
    g_args = (0, 2 * call, 256 << 20, a.piece_kib << 10)
    tmp = tempfile.mkdtemp(prefix="gunzip_lab_")
    for kind, text in (("fastq", fastq_text(a.reads)), ("fasta", fasta_text(int(a.fasta_gb * 1e9)))):
        c = zlib.compressobj(a.level, zlib.DEFLATED, 31)
        t0 = time.perf_counter()
        z = c.compress(text) + c.flush()
        res = dict(file=kind, level=a.level, text_bytes=len(text), gz_bytes=len(z), compress_s=round(time.perf_counter() - t0, 2),
                   piece_kib=a.piece_kib, call_mib=a.call_mib)
        zp = Pinned(len(z))
        C.memmove(zp.p, z, len(z))
        dev = torch.empty(len(text), dtype=torch.uint8, device="cuda:0")
        host = Pinned(256 << 20)
        per, wall = {k: [] for k in KERNELS}, []
        for rep in range(a.reps + 1):                           # the first run is the warm-up
            n, ms, pieces, dropped = gunzip_all(g_args, zp.p.value, len(z), dev.data_ptr(), len(text), True, call)
            assert n == len(text)
            g = capi.Gunzipper(*g_args)                         # host output: call after call into the page-locked buffer
            pos, end, m = 0, 0, 0
            t0 = time.perf_counter()
            while pos < len(z):
                end = min(max(end, pos) + call, len(z))
                rc, used, nn, _ = g.run_raw((zp.p.value + pos, end - pos), end == len(z), host.p.value, host.n, False)
                capi._chk(rc, "bwams_gunzip_run")
                pos += used
                m += nn
            t1 = time.perf_counter()
            g.close()
            assert m == len(text)
            if rep:
                wall.append(t1 - t0)
                for k in KERNELS:
                    per[k].append(ms[k] / 1e3)
        assert bytes(dev[:1 << 20].cpu().numpy()) == text[:1 << 20] and bytes(dev[-(1 << 20):].cpu().numpy()) == text[-(1 << 20):]
        res.update(pieces=pieces, pieces_dropped=dropped, call_gbs=round(len(text) / med(wall) / 1e9, 3),
                   gbs_all=round(len(text) / sum(med(per[k]) for k in KERNELS) / 1e9, 3),
                   **{"gbs_" + k: round(len(text) / max(med(per[k]), 1e-9) / 1e9, 3) for k in KERNELS})
        path = os.path.join(tmp, f"{kind}.gz")
        open(path, "wb").write(z)
        r = C.c_void_p()                                        # one zlib thread: the reader's own ms_inflate
        capi._chk(capi.lib().bwams_reader_open(path.encode(), C.c_int64(a.chunk_bases), 0, C.c_int64(0), 2, C.byref(r)), "bwams_reader_open")
        while True:
            tp, nb, nr, nbs = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
            if capi.lib().bwams_reader_next(r, C.byref(tp), C.byref(nb), C.byref(nr), C.byref(nbs)):
                break
            capi.lib().bwams_reader_release(r, tp)
        info = capi.reader_info(r)
        capi.lib().bwams_reader_close(r)
        res.update(zlib_gbs=round(info.out_bytes / (info.ms_inflate / 1e3) / 1e9, 3))
        bz = bgzip(text, a.level, a.threads)                    # the BGZF inflater on the same text
        bp = Pinned(len(bz))
        C.memmove(bp.p, bz, len(bz))
        f = capi.Inflater(0, 32 << 20, 64 << 20)
        ks = []
        for rep in range(min(a.reps, 3) + 1):
            at, done, ms_k = 0, 0, 0.0
            while at < len(bz):
                rc, used, n, st = f.run_raw((bp.p.value + at, min(len(bz) - at, 32 << 20)), dev.data_ptr() + done, len(text) - done, True)
                capi._chk(rc, "bwams_inflater_run")
                at += used
                done += n
                ms_k += st.ms_kernel
            if rep:
                ks.append(ms_k / 1e3)
        f.close()
        bp.close()
        res.update(bgzf_kernel_gbs=round(len(text) / med(ks) / 1e9, 3))
        if kind == "fastq":
            for name, flags in (("reader_zlib_gbs", 0), ("reader_gunzip_gbs", capi.READER_GUNZIP)):
                rates = [reader_rate(lambda p, cb: capi.reader_open_device2(p, 0, cb, False, 0, 2, flags), path, a.chunk_bases)
                         for _ in range(min(a.reps, 3))]
                res[name] = round(med([x[1] for x in rates]), 3)
        os.remove(path)
        zp.close()
        host.close()
        del dev
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
