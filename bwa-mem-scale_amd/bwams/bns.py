"""numpy restatement of bns_fasta2bntseq (reference src/bntseq.cpp:269-372, for_only = 1): FASTA text -> base codes, .ann,
.amb and .pac bytes.  The checker of the device path (csrc/fasta_ref.hip); tests pin it to the reference's own bytes
(tests/golden/bns_cases.npz) and its generator to glibc's srand48 / lrand48.

kseq_read (src/kseq.h:358-400, OPT_RW) on a FASTA text, record by record:
  - bytes before the first '>' or '@' are skipped, even in mid-line; a line starting with '>' or '@' begins the next record;
  - the name runs to the first isspace() byte; unless that byte is '\\n', the rest of the line is the comment;
  - sequence lines are concatenated, empty lines skipped; a line starting with '+' makes the record FASTQ (refused here);
  - a trailing '\\r' goes only when the accumulated string is then longer than one byte, and not from a last line that is a
    lone '\\r' without '\\n' (the append returns at EOF before its test).
add1: nst_nt4_table codes; every code >= 4 takes lrand48() & 3 after srand48(11), in global base order; a hole is a run of one
ambiguous byte value inside one contig (`lasts` starts at 0 per contig).
"""
from __future__ import annotations

import numpy as np

SEED = 11
LCG_A, LCG_C, MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1
X0 = (SEED << 16) | 0x330E                      # srand48(11)

NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = NT4[_c + 32] = _i
NT4[ord("-")] = 5


class FastaError(ValueError):
    pass


def lrand48_draws(first: int, count: int) -> np.ndarray:
    """lrand48() of draws first+1 .. first+count after srand48(11) (draw k uses state X_k), by jump-ahead."""
    r = np.arange(first, first + count, dtype=np.uint64)
    x = np.full(count, X0, dtype=np.uint64)
    a, c = LCG_A, LCG_C
    m = np.uint64(MASK)
    for i in range(48):                          # apply the 2^i-step map where bit i of the rank is set
        sel = ((r >> np.uint64(i)) & np.uint64(1)).astype(bool)
        if sel.any():
            x[sel] = (np.uint64(a) * x[sel] + np.uint64(c)) & m
        c = (a * c + c) & MASK
        a = (a * a) & MASK
        if (first + count) >> (i + 1) == 0:
            break
    x = (np.uint64(LCG_A) * x + np.uint64(LCG_C)) & m    # one more step: draw r + 1
    return (x >> np.uint64(17)).astype(np.int64)


def _is_space(b: int) -> bool:
    return b == 32 or 9 <= b <= 13


def parse(text: bytes):
    """kseq_read's records: list of (name, comment, sequence bytes)."""
    p = min([i for i in (text.find(b">"), text.find(b"@")) if i >= 0], default=-1)
    if p < 0:
        raise FastaError("no '>' header")
    recs = []
    lines = text[p:].split(b"\n")
    ends_nl = [True] * (len(lines) - 1) + [False]
    if lines and lines[-1] == b"":                # the text ended with '\n'
        lines.pop(); ends_nl.pop()
    cur = None
    for line, nl in zip(lines, ends_nl):
        if cur is None or (line and line[0] in b">@"):
            if len(line) == 1 and not nl:         # a lone '>' at EOF starts no record
                break
            q = 1
            while q < len(line) and not _is_space(line[q]):
                q += 1
            name, comment = line[1:q], b""
            if q < len(line):
                comment = line[q + 1:]
                if len(comment) > 1 and comment.endswith(b"\r"):
                    comment = comment[:-1]
            cur = [name, comment, bytearray()]
            recs.append(cur)
            continue
        if not line:
            continue
        if line[0] == ord("+"):
            raise FastaError("a line starts with '+' (FASTQ)")
        s = cur[2]
        s += line
        if line.endswith(b"\r") and len(s) > 1 and (len(line) > 1 or nl):
            del s[-1]
    return [(r[0], r[1], bytes(r[2])) for r in recs]


def fasta2bntseq(text: bytes) -> dict:
    """codes (uint8 0..3), contigs (offset, len, n_ambs), names, comments, holes, and the .ann / .amb / .pac bytes."""
    recs = parse(text)
    raw = np.frombuffer(b"".join(r[2] for r in recs), np.uint8)
    l_pac = len(raw)
    lens = np.array([len(r[2]) for r in recs], np.int64)
    if (lens > 0x7FFFFFFF).any():
        raise FastaError("a sequence is longer than INT32_MAX")
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(recs) else np.zeros(0, np.int64)
    code = NT4[raw].copy()
    amb = code >= 4
    start = np.zeros(l_pac, bool)
    start[offs[lens > 0]] = True
    prev_diff = np.ones(l_pac, bool)
    prev_diff[1:] = raw[1:] != raw[:-1]
    hs = np.flatnonzero(amb & (start | prev_diff))
    nxt_end = np.zeros(l_pac, bool)
    if l_pac:
        nxt_end[-1] = True
        nxt_end[:-1] = start[1:] | (raw[1:] != raw[:-1])
    he = np.flatnonzero(amb & nxt_end) + 1
    n_amb = int(amb.sum())
    code[amb] = (lrand48_draws(0, n_amb) & 3).astype(np.uint8)
    n_ambs = np.searchsorted(hs, offs + lens) - np.searchsorted(hs, offs)
    ann = [b"%d %d %u\n" % (l_pac, len(recs), SEED)]
    for (name, comment, _), o, ln, na in zip(recs, offs, lens, n_ambs):
        ann.append(b"0 %s %s\n%d %d %d\n" % (name, comment if comment else b"(null)", o, ln, na))
    amb_txt = [b"%d %d %u\n" % (l_pac, len(recs), len(hs))]
    for b, e in zip(hs, he):
        amb_txt.append(b"%d %d %c\n" % (b, e - b, int(raw[b])))
    c4 = np.zeros((l_pac + 3) // 4 * 4, np.uint8)
    c4[:l_pac] = code
    c4 = c4.reshape(-1, 4)
    pac = (c4[:, 0] << 6 | c4[:, 1] << 4 | c4[:, 2] << 2 | c4[:, 3]).astype(np.uint8).tobytes()
    pac += (b"\0" if l_pac % 4 == 0 else b"") + bytes([l_pac % 4])
    return dict(codes=code, l_pac=l_pac, offsets=offs, lens=lens, n_ambs=n_ambs, names=[r[0] for r in recs],
                comments=[r[1] for r in recs], holes=(hs, he - hs, raw[hs] if len(hs) else np.zeros(0, np.uint8)),
                n_ambig=n_amb, ann=b"".join(ann), amb=b"".join(amb_txt), pac=pac)


def restored_annos(comments) -> list:
    """bntann1_t.anno as bns_restore reads the .ann back: the comment, or b"" for none (and for a literal "(null)")."""
    return [b"" if (not c or c == b"(null)") else c for c in comments]
