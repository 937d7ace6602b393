"""`samtools merge` for coordinate-sorted BAM files on one GPU: the files are merged on the device (bwams_bam_file_open_merge, the
rules M1 to M9 of include/bwams.h) and written with an index by the sorted writer.

  bam_merge.py IN1.bam IN2.bam ... -o OUT.bam [--markdup] [--regions ref:beg-end ...] [--piece-mb N] [--device D]

The merged pieces go to bwams_sorter_put as runs, seq = the piece's ordinal; OUT.bam and OUT.bam.bai are written by
bwams_sorter_close.  (The sorter's host merge over runs that are already in order is redundant work; a writer that takes an
ordered stream directly is the follow-up.)  --markdup: duplicates are marked across the files first, in two passes through
bwams_dupjoin_t over the same pieces (rule M8 makes the second query's pieces those of the first); the read groups' libraries
come from the merged header.  --regions: only the records that overlap them, ref[:beg[-end]] 1-based inclusive as bam_view.py
takes them; every input then needs its .bai.  With --markdup the marks hold for the records of the regions only (rule J7).
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bwams import capi, samview  # noqa: E402
from bam_view import region  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(usage="bam_merge.py IN1.bam IN2.bam ... -o OUT.bam [--markdup] [--regions ref:beg-end ...]")
    ap.add_argument("inputs", nargs="+")
    ap.add_argument("-o", dest="out", required=True)
    ap.add_argument("--markdup", action="store_true")
    ap.add_argument("--regions", nargs="*", default=[])
    ap.add_argument("--piece-mb", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    f = capi.BamFile.merge(a.inputs, device=a.device, piece_bytes=a.piece_mb << 20)
    j = groups = None
    try:
        names = samview.header_names(f.header_block())
        regions = [region(r, names, f.refs()) for r in a.regions]
        if a.markdup:
            groups = capi.DupGroups(f.header()[0])
            j = capi.DupJoin(groups, a.device)
            f.query(regions)
            for piece in f.pieces():
                j.add_file(piece)
            st, _ = j.finish()
            print("bam_merge: %d records of %d templates marked as duplicates" % (st.counts()["records_marked"], st.counts()["templates"]),
                  file=sys.stderr)
        s = capi.Sorter(a.out, a.device, f.header_block(), bai=True)
        f.query(regions)
        for k, piece in enumerate(f.pieces()):
            if j is not None:
                j.apply_file(piece)
            s.put(k, *piece.fetch())
        st = s.close()
        i = f.merge_info()
        print("bam_merge: %d files, %d records in %d pieces -> %s (%d bytes)" % (i["n_files"], st.records, i["rounds"], a.out, st.out_bytes),
              file=sys.stderr)
    finally:
        if j is not None:
            j.close()
        if groups is not None:
            groups.close()
        f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
