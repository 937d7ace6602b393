"""The parallel gzip decoder of csrc/gunzip.hip restated in pure Python, for the tests: no GPU, no zlib inside.

  walk / walk_gzip     every DEFLATE block of a stream: start bit, kind, final flag, output length
  is_candidate         the test gz_find_kernel applies at a bit offset: a non-final dynamic block header that parses
  first_candidates     the first candidate in each piece of piece_bytes, as the kernel reports them
  decode_piece         a piece decoded to 16-bit symbols: a byte, or 0x8000 | k = byte k of the 32 KiB in front of its start
  resolve              the symbols with their markers looked up in that window

The tests use it to prove that their inputs have the shapes they claim (pieces that hold a block start, false candidates, histories
that are mostly markers), and tests/test_gunzip.py checks it against zlib.
"""
from __future__ import annotations

import numpy as np

WIN = 32768
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Damaged(ValueError):
    pass


class _Bits:
    """LSB-first bits of buf from bit `pos`; bytes past the end read as 0 (the caller checks pos against the end)."""

    def __init__(self, buf: bytes, pos: int = 0):
        self.buf, self.pos, self.end = buf, pos, 8 * len(buf)

    def peek(self, n: int) -> int:
        p = self.pos >> 3
        return (int.from_bytes(self.buf[p:p + 8], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n: int) -> int:
        v = self.peek(n)
        self.pos += n
        return v


def _check(lens, cl: bool) -> None:
    """zlib's inflate_table rules: no over-subscribed code, no incomplete one except a single code of length 1 (never for `cl`)."""
    left, mx = 1, 0
    for ln in range(1, 16):
        c = sum(1 for x in lens if x == ln)
        left = 2 * left - c
        if left < 0:
            raise Damaged("over-subscribed code")
        if c:
            mx = ln
    if mx and left > 0 and (cl or mx != 1):
        raise Damaged("incomplete code")


def _table(lens):
    """(table, bits): table[next `bits` bits] = (symbol, length) or None."""
    mx = max(lens) if lens else 0
    if mx == 0:
        return [None], 0
    tab = [None] * (1 << mx)
    code = 0
    for ln in range(1, mx + 1):
        for s, x in enumerate(lens):
            if x == ln:
                rev = int(format(code, f"0{ln}b")[::-1], 2)
                tab[rev::1 << ln] = [(s, ln)] * (1 << (mx - ln))
                code += 1
        code <<= 1
    return tab, mx


def _sym(b: _Bits, tab, bits: int) -> int:
    e = tab[b.peek(bits)]
    if e is None:
        raise Damaged("no such code")
    b.pos += e[1]
    return e[0]


def _dynamic_header(b: _Bits):
    """The code lengths of a dynamic block behind its 3 header bits: (literal/length lengths, distance lengths)."""
    nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if nlen > 286 or ndist > 30:
        raise Damaged("too many symbols")
    cl = [0] * 19
    for i in range(ncode):
        cl[CL_ORDER[i]] = b.take(3)
    _check(cl, True)
    tab, bits = _table(cl)
    lens = []
    while len(lens) < nlen + ndist:
        if b.pos > b.end:
            raise Damaged("overrun")
        s = _sym(b, tab, bits)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Damaged("repeat with nothing before it")
            v, rep = lens[-1], 3 + b.take(2)
        elif s == 17:
            v, rep = 0, 3 + b.take(3)
        else:
            v, rep = 0, 11 + b.take(7)
        if len(lens) + rep > nlen + ndist:
            raise Damaged("repeat past the end")
        lens += [v] * rep
    if b.pos > b.end:
        raise Damaged("overrun")
    if lens[256] == 0:
        raise Damaged("no end-of-block code")
    _check(lens[:nlen], False)
    _check(lens[nlen:], False)
    return lens[:nlen], lens[nlen:]


_FIXED = ([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32)


def _block(b: _Bits, out, emit: bool) -> tuple:
    """One block at b: (kind, final, output length).  out: a list of symbols that grows (emit) or a one-element count."""
    final, kind = b.take(1), b.take(2)
    n0 = len(out) if emit else out[0]
    if kind == 0:
        b.pos = (b.pos + 7) & ~7
        ln, nln = b.take(16), b.take(16)
        if ln != (~nln & 0xffff) or b.pos + 8 * ln > b.end:
            raise Damaged("stored block")
        if emit:
            out.extend(b.buf[b.pos >> 3:(b.pos >> 3) + ln])
        else:
            out[0] += ln
        b.pos += 8 * ln
        return kind, final, ln
    if kind == 3:
        raise Damaged("block type 3")
    ll, dl = _FIXED if kind == 1 else _dynamic_header(b)
    lt, lb = _table(ll)
    dt, db = _table(dl)
    n = n0
    while True:
        if b.pos > b.end:
            raise Damaged("overrun")
        s = _sym(b, lt, lb)
        if s < 256:
            if emit:
                out.append(s)
            n += 1
            continue
        if s == 256:
            break
        s -= 257
        if s >= 29:
            raise Damaged("length symbol")
        ln = LEN_BASE[s] + b.take(LEN_EXTRA[s])
        d = _sym(b, dt, db)
        if d >= 30:
            raise Damaged("distance symbol")
        dist = DIST_BASE[d] + b.take(DIST_EXTRA[d])
        if emit:
            at = len(out) - dist
            if at >= 0 and dist >= ln:
                out.extend(out[at:at + ln])
            elif at >= 0 and dist == 1:
                out.extend(out[-1:] * ln)
            else:
                for _ in range(ln):
                    at = len(out) - dist
                    out.append(out[at] if at >= 0 else 0x8000 | (WIN + at))
        n += ln
    if not emit:
        out[0] = n
    if b.pos > b.end:
        raise Damaged("overrun")
    return kind, final, n - n0


def walk(raw: bytes, start_bit: int = 0):
    """Every block of the raw DEFLATE stream at start_bit: ([(start bit, kind, final, output length)], the bit behind the last)."""
    b, out, blocks = _Bits(raw, start_bit), [0], []
    while True:
        at = b.pos
        kind, final, n = _block(b, out, False)
        blocks.append((at, kind, final, n))
        if final:
            return blocks, b.pos


def header_len(gz: bytes, at: int = 0) -> int:
    """The bytes of the gzip member header at gz[at]."""
    if gz[at:at + 3] != b"\x1f\x8b\x08":
        raise Damaged("no gzip header")
    flg, p = gz[at + 3], at + 10
    if flg & 4:
        p += 2 + (gz[p] | gz[p + 1] << 8)
    for f in (8, 16):
        if flg & f:
            p = gz.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return p - at


def walk_gzip(gz: bytes):
    """Every block of every member of a gzip file, start bits counted in the file: ([blocks], [(header byte, trailer byte)])."""
    blocks, members, at = [], [], 0
    while at + 2 <= len(gz) and gz[at:at + 2] == b"\x1f\x8b":
        start = at + header_len(gz, at)
        bl, end = walk(gz, 8 * start)
        blocks += bl
        trailer = (end + 7) >> 3
        members.append((at, trailer))
        at = trailer + 8
    return blocks, members


def _bit_array(buf: bytes):
    return np.unpackbits(np.frombuffer(buf, np.uint8), bitorder="little")


def is_candidate(buf: bytes, bit: int) -> bool:
    """gz_find_kernel's test at one bit offset."""
    b = _Bits(buf, bit)
    if b.take(3) != 4:                                   # BFINAL = 0, BTYPE = 2
        return False
    try:
        _dynamic_header(b)
    except Damaged:
        return False
    return True


def candidates(buf: bytes, a: int, e: int, first_only: bool = False):
    """The candidate bit offsets in [a, e): the 17 header bits and the Kraft sum of the code lengths code for every offset at once
    (numpy), the full parse for the survivors."""
    e = min(e, 8 * len(buf))
    if a >= e:
        return []
    bits = _bit_array(buf[a >> 3:(e >> 3) + 16] + bytes(16)).astype(np.int64)
    off = np.arange(a & 7, (a & 7) + (e - a))
    f = lambda k, n: sum(bits[off + k + i] << i for i in range(n))
    ok = (f(0, 3) == 4) & (f(3, 5) <= 29) & (f(8, 5) <= 29)
    off = off[ok]
    ncode = f(13, 4) + 4
    kraft = np.zeros(len(off), np.int64)
    for i in range(19):
        ln = f(17 + 3 * i, 3)
        kraft += np.where((i < ncode) & (ln > 0), 128 >> ln, 0)
    out = []
    for o in off[kraft == 128]:
        bit = int(o) - (a & 7) + a
        if is_candidate(buf, bit):
            out.append(bit)
            if first_only:
                break
    return out


def first_candidates(buf: bytes, piece_bytes: int):
    """Per piece k >= 1 of piece_bytes: its first candidate bit offset, or None (index 0 is None: piece 0 starts where the stream is)."""
    n = (len(buf) + piece_bytes - 1) // piece_bytes
    out = [None]
    for k in range(1, n):
        c = candidates(buf, 8 * k * piece_bytes, 8 * (k + 1) * piece_bytes, first_only=True)
        out.append(c[0] if c else None)
    return out


def decode_piece(raw: bytes, start_bit: int, end_bit: int):
    """The blocks from start_bit up to the boundary end_bit (or the final block) as symbols with markers."""
    b, out, final = _Bits(raw, start_bit), [], 0
    while b.pos < end_bit:
        _, final, _ = _block(b, out, True)
        if final:
            break
    if b.pos != end_bit and not final:
        raise Damaged("no block boundary at end_bit")
    return out


def resolve(symbols, window: bytes) -> bytes:
    """The bytes of a piece: window = the 32 KiB in front of its start (shorter: the stream's first bytes, right-aligned)."""
    w = bytes(WIN - len(window)) + window
    return bytes(w[s & 0x7fff] if s & 0x8000 else s for s in symbols)


def next_window(symbols, window: bytes) -> bytes:
    """gz_window_kernel's step: the window behind a piece from the window in front of it."""
    return ((bytes(WIN - len(window)) + window) + resolve(symbols, window))[-WIN:]
