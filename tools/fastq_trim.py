"""Adapter and quality trimming of FASTQ files on one GPU, in front of the mapper (what `fastp` does with its defaults; the rules are
T1 to T9 above bwams_fastq_trim in include/bwams.h): the reader cuts the input into chunks, each chunk is decoded, trimmed and
written back as FASTQ text on the device (bwams_fastq_decode, bwams_fastq_trim, bwams_fastq_text), and the deflater compresses it.

usage: fastq_trim.py [options] -o out.fq[.gz] in.fq[.gz]                         single-end
       fastq_trim.py [options] --interleaved -o out.fq[.gz] in.fq[.gz]           pairs, the ends interleaved in one file
       fastq_trim.py [options] -o out1.fq[.gz] -O out2.fq[.gz] in1.fq[.gz] in2.fq[.gz]

An output whose name ends in .gz is written as BGZF (which gunzip reads), any other as plain text.  Every field of bwams_trim_opt_t
is an option (--cut-front 1, --adapter1 AGATCGGAAGAGC, ...); the defaults are bwams_trim_opt_default's.  The stats of the whole run
go to stdout (or --json FILE) as one JSON object.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import capi  # noqa: E402


def chunks(path: str, chunk_bases: int, paired: bool):
    """the texts of a file's chunks (whole records; an even number of them with paired)"""
    L = capi.lib()
    r = capi.reader_open(path, chunk_bases, paired)
    try:
        while True:
            text, nb, n, bases = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
            rc = L.bwams_reader_next(r, C.byref(text), C.byref(nb), C.byref(n), C.byref(bases))
            if rc == 1:
                return
            if rc:
                raise capi.BwamsError(rc, "bwams_reader_next", L.bwams_reader_error(r).decode())
            data = C.string_at(text, nb.value)
            L.bwams_reader_release(r, text)
            yield data
    finally:
        L.bwams_reader_close(r)


def records(path: str, chunk_bases: int):
    """the four-line records of a file, chunk by chunk, as lists"""
    for text in chunks(path, chunk_bases, False):
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        if len(lines) % 4:
            raise SystemExit(f"fastq_trim: {path}: records of four lines are required when two files are read")
        yield [b"\n".join(lines[k:k + 4]) + b"\n" for k in range(0, len(lines), 4)]


def interleaved(path1: str, path2: str, chunk_bases: int):
    """record k of the first file, record k of the second, as chunk texts"""
    g1, g2 = records(path1, chunk_bases), records(path2, chunk_bases)
    b1, b2 = [], []
    while True:
        if not b1:
            b1 = next(g1, None)
        if not b2:
            b2 = next(g2, None)
        if b1 is None or b2 is None:
            if b1 or b2:
                raise SystemExit("fastq_trim: the two files hold different numbers of records")
            return
        n = min(len(b1), len(b2))
        yield b"".join(x + y for x, y in zip(b1[:n], b2[:n]))
        b1, b2 = b1[n:], b2[n:]


class Out:
    """a FASTQ output: BGZF through the GPU deflater when the name ends in .gz"""

    PIECE = 32 << 20                  # the deflater's input limit: a chunk's text goes through it in pieces, each whole BGZF members

    def __init__(self, path: str, device: int):
        self.f = open(path, "wb")
        self.d = capi.Deflater(device, self.PIECE) if path.endswith(".gz") else None

    def put(self, data):
        """data: bytes, or (device address, n_bytes)"""
        if self.d is not None:
            n = data[1] if isinstance(data, tuple) else len(data)
            for at in range(0, n, self.PIECE):
                m = min(self.PIECE, n - at)
                self.f.write(self.d.run((data[0] + at, m) if isinstance(data, tuple) else data[at:at + m])[0])
        elif isinstance(data, tuple):
            raise ValueError("plain output takes host bytes")
        else:
            self.f.write(data)

    def close(self):
        if self.d is not None:
            self.f.write(self.d.run(b"", eof=True)[0])
            self.d.close()
        self.f.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(usage=__doc__.split("usage: ")[1].split("\n\n")[0])
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("-o", dest="out1", required=True)
    ap.add_argument("-O", dest="out2")
    ap.add_argument("--interleaved", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--chunk-bases", type=int, default=8_000_000)
    ap.add_argument("--json")
    ints = [n for n, t in capi.TrimOpt._fields_ if t is C.c_int32]
    for n in ints:
        ap.add_argument("--" + n.replace("_", "-"), type=int)
    ap.add_argument("--adapter1")
    ap.add_argument("--adapter2")
    a = ap.parse_args(argv)
    if len(a.inputs) > 2 or (len(a.inputs) == 2) != bool(a.out2) or (a.interleaved and len(a.inputs) == 2):
        ap.error("one input and -o, one interleaved input and -o, or two inputs with -o and -O")
    paired = a.interleaved or len(a.inputs) == 2
    kw = {n: getattr(a, n) for n in ints if getattr(a, n) is not None}
    kw.update({n: getattr(a, n).encode() for n in ("adapter1", "adapter2") if getattr(a, n)})
    opt = capi.trim_opt(**kw)
    src = interleaved(a.inputs[0], a.inputs[1], a.chunk_bases) if len(a.inputs) == 2 else chunks(a.inputs[0], a.chunk_bases, paired)
    outs = [Out(a.out1, a.device)] + ([Out(a.out2, a.device)] if a.out2 else [])
    total: dict = {}
    try:
        for text in src:
            fq = capi.Fastq(text, a.device)
            t, _, st = fq.trim(opt, paired, report=False)
            fq.close()
            for k, v in st.items():
                if isinstance(v, list):
                    total[k] = [x + y for x, y in zip(total.get(k, [0] * len(v)), v)]
                else:
                    total[k] = total.get(k, 0) + v
            if len(outs) == 1:
                outs[0].put(t.text(fetch=False) if outs[0].d is not None else t.text())
            else:                                         # the two ends back to their files
                lines = t.text().split(b"\n")
                per = 4 if capi.lib().bwams_fastq_has_qual(t.h) else 2
                recs = [b"\n".join(lines[k:k + per]) + b"\n" for k in range(0, len(lines) - 1, per)]
                outs[0].put(b"".join(recs[0::2])); outs[1].put(b"".join(recs[1::2]))
            t.close()
    finally:
        for o in outs:
            o.close()
    text = json.dumps(total)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    else:
        print(text, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
