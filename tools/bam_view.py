"""`samtools view` for a coordinate-sorted BAM with its .bai, on one GPU: the records are selected by region on the device
(bwams_bam_file_t) and printed as SAM lines there (bwams_samview_t); only the text comes to the host.

usage: bam_view.py [-h] [-f N] [-F N] [-q N] file.bam [ref:beg-end ...]

  -h     write the header text first (as in samtools view; --help is the usage)
  -f N   only records with every bit of N set in FLAG
  -F N   only records with no bit of N set in FLAG
  -q N   only records with MAPQ >= N
A region is ref, ref:beg or ref:beg-end with 1-based inclusive positions and the reference by name; none: the whole file.  N may be
decimal, hex (0x...) or octal (0...).  The lines go to stdout in file order, each record once.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import capi, samview  # noqa: E402


def region(text: str, names, lengths) -> tuple:
    """ref[:beg[-end]] -> (ref, beg, end), 0-based and half-open"""
    name, _, span = text.rpartition(":") if ":" in text and text.encode() not in names else (text, "", "")
    if name.encode() not in names:
        raise SystemExit(f"bam_view: unknown reference in region {text!r}")
    ref = names.index(name.encode())
    beg, end = 1, int(lengths[ref])
    if span:
        a, _, b = span.replace(",", "").partition("-")
        beg = int(a)
        end = int(b) if b else end
    return ref, max(beg - 1, 0), end


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(add_help=False, usage="bam_view.py [-h] [-f N] [-F N] [-q N] file.bam [ref:beg-end ...]")
    ap.add_argument("--help", action="help")
    ap.add_argument("-h", dest="header", action="store_true")
    ap.add_argument("-f", dest="require", type=lambda s: int(s, 0), default=0)
    ap.add_argument("-F", dest="exclude", type=lambda s: int(s, 0), default=0)
    ap.add_argument("-q", dest="min_mapq", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("bam")
    ap.add_argument("regions", nargs="*")
    a = ap.parse_args(argv)
    out = sys.stdout.buffer
    f = capi.BamFile(a.bam, device=a.device)
    v = capi.SamView(f.header_block(), a.device, a.require, a.exclude, a.min_mapq)
    try:
        if a.header:
            out.write(f.header()[0])
        names = samview.header_names(f.header_block())
        f.query([region(r, names, f.refs()) for r in a.regions])
        for piece in f.pieces():
            v.add_file(piece)
            out.write(v.fetch()[0])
        out.flush()
    finally:
        v.close()
        f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
