"""Coordinate-sorted BAM files merged as one record stream, restated in Python (include/bwams.h, above bwams_bam_file_open_merge,
rules M1 to M9): the order of the merged stream (merge_records, M4), the merged header (merge_header, M2 and M3) and the rounds
that cut the stream into pieces (rounds, M7).  Nothing here touches a device: the GPU tests compare the library with these, and the
frontier rule can be tested where there is no GPU."""
from __future__ import annotations

import heapq
import struct

from . import bam

ERR_ARG, ERR_UNSUPPORTED = -3, -6
MAX_FILES = 64


class MergeRefusal(ValueError):
    """What the library returns as an error code: .code is that BWAMS_ERR_* value"""

    def __init__(self, code: int, text: str):
        super().__init__(text)
        self.code = code


def _key(rec) -> int:
    """a record's key: bam.coord_key of BAM bytes, else the first element of a tuple"""
    return bam.coord_key(rec) if isinstance(rec, (bytes, bytearray)) else rec[0]


def merge_records(files, key=_key) -> list:
    """M4: every record of every file once, ordered by (key, file index, ordinal within the file).  files: a list of records per
    file, each sorted by key (what bwams_sorter_close gives when file k is put as the run with seq = k)."""
    runs = [[(key(r), k, i, r) for i, r in enumerate(f)] for k, f in enumerate(files)]
    return [t[3] for t in heapq.merge(*runs, key=lambda t: t[:3])]


def rounds(files_as_piece_lists, key=_key, log=None) -> list:
    """M7, literally: files_as_piece_lists[j] is the list of pieces of child j, a piece being a list of records.  Returns the merged
    pieces.  A child is open while it has pieces to come.  log, when a list, receives a row per round: (the children that were open,
    each child's window size before the round, each child's emitted count)."""
    K = len(files_as_piece_lists)
    nxt = [0] * K                                    # the next piece of each child
    win = [[] for _ in range(K)]                     # the windows
    out = []
    while True:
        is_open = [nxt[j] < len(files_as_piece_lists[j]) for j in range(K)]
        for j in range(K):                           # every open child with an empty window is advanced, while pieces come back empty
            while is_open[j] and not win[j]:
                win[j] = list(files_as_piece_lists[j][nxt[j]])
                nxt[j] += 1
                is_open[j] = nxt[j] < len(files_as_piece_lists[j])
        before = [len(w) for w in win]
        if not any(is_open):                         # every window whole: the last piece
            emit = before
        else:
            last = {j: key(win[j][-1]) for j in range(K) if is_open[j]}     # an open child's window is not empty here
            F = min(last.values())
            i_star = min(j for j, v in last.items() if v == F)
            emit = [sum(1 for r in win[j] if key(r) < F or (key(r) == F and j <= i_star)) for j in range(K)]
        taken = [win[j][:emit[j]] for j in range(K)]
        win = [win[j][emit[j]:] for j in range(K)]
        out.append(merge_records(taken, key))
        if log is not None:
            log.append((is_open, before, emit))
        if not any(is_open):
            return out


# ---- the header (M2, M3) ----

def parse_header_block(block: bytes):
    """-> (text, [(name with its NUL, l_ref), ...]) of a BAM header block; MergeRefusal(ERR_ARG) when it is cut off or not one"""
    block = bytes(block)

    def need(p, n):
        if p + n > len(block):
            raise MergeRefusal(ERR_ARG, "the header block is cut off")
    need(0, 8)
    if block[:4] != b"BAM\1":
        raise MergeRefusal(ERR_ARG, "the header block does not start with the BAM magic")
    (l_text,) = struct.unpack_from("<i", block, 4)
    if l_text < 0:
        raise MergeRefusal(ERR_ARG, "the header block is cut off")
    need(8, l_text + 4)
    text = block[8:8 + l_text]
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", block, p)
    p += 4
    if n_ref < 0:
        raise MergeRefusal(ERR_ARG, "the header block is cut off")
    refs = []
    for _ in range(n_ref):
        need(p, 4)
        (l_name,) = struct.unpack_from("<i", block, p)
        if l_name < 0:
            raise MergeRefusal(ERR_ARG, "the header block is cut off")
        need(p + 4, l_name + 4)
        refs.append((block[p + 4:p + 4 + l_name], struct.unpack_from("<i", block, p + 4 + l_name)[0]))
        p += 8 + l_name
    return text, refs


def _lines(text: bytes) -> list:
    """the text's lines without their newlines: NUL padding behind the text and empty lines are no lines"""
    return [ln for ln in text.rstrip(b"\0").split(b"\n") if ln]


def _id_of(line: bytes):
    for f in line.split(b"\t")[1:]:
        if f[:3] == b"ID:":
            return f[3:]
    return None


def merge_header(blocks):
    """M2 and M3: -> (the merged header block, the @PG lines dropped).  MergeRefusal(ERR_UNSUPPORTED) for reference lists that
    differ and for an @RG ID taken with other bytes."""
    if not 1 <= len(blocks) <= MAX_FILES:
        raise MergeRefusal(ERR_ARG, "1 to 64 header blocks are required")
    parsed = [parse_header_block(b) for b in blocks]
    refs0 = parsed[0][1]
    for k, (_, refs) in enumerate(parsed):
        if len(refs) != len(refs0):
            raise MergeRefusal(ERR_UNSUPPORTED, "file %d has %d references, file 0 has %d" % (k, len(refs), len(refs0)))
        for r, (a, b) in enumerate(zip(refs, refs0)):
            if a[0] != b[0]:
                raise MergeRefusal(ERR_UNSUPPORTED, "file %d: reference %d: its name differs from file 0's" % (k, r))
            if a[1] != b[1]:
                raise MergeRefusal(ERR_UNSUPPORTED, "file %d: reference %d: its length %d differs from file 0's %d" % (k, r, a[1], b[1]))
    first = _lines(parsed[0][0])
    out = [ln for ln in first if ln[:3] == b"@HD"][:1] + [ln for ln in first if ln[:3] == b"@SQ"]
    taken = set(out)
    ids = {b"@RG": {}, b"@PG": {}}                   # ID -> (the file that gave it, its line)
    dropped = 0
    for k, (text, _) in enumerate(parsed):
        for ln in _lines(text):
            kind = ln[:3]
            if kind in (b"@HD", b"@SQ") or ln in taken:
                continue
            if kind in ids and _id_of(ln) is not None:
                i = _id_of(ln)
                if i in ids[kind]:
                    if kind == b"@PG":
                        dropped += 1
                        continue
                    raise MergeRefusal(ERR_UNSUPPORTED, "file %d: @RG ID %s is file %d's with other bytes" %
                                       (k, i.decode("latin-1"), ids[kind][i][0]))
                ids[kind][i] = (k, ln)
            taken.add(ln)
            out.append(ln)
    text = b"".join(ln + b"\n" for ln in out)
    block = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs0))
    for name, l_ref in refs0:
        block += struct.pack("<i", len(name)) + name + struct.pack("<i", l_ref)
    return block, dropped


def child_bytes_of(piece_bytes: int, n_files: int, child_bytes: int = 0) -> int:
    """M1: a child's piece size"""
    if child_bytes:
        return child_bytes
    return ((piece_bytes or (128 << 20)) // n_files) & ~0xFFFF
