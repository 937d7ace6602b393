"""BAM records viewed as SAM text on the GPU (csrc/samview.hip, bwams_samview_t): every comparison is byte-exact against
bwams/samview.py (rules V1-V8, include/bwams.h above bwams_samview_open): the text, line_off, out() and the info() counts."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import bam_query_cases as Q
from bwams import bai, bam, bgzf, capi, samview, simulate
from samview_cases import LITERALS, NAMED_BITS, NAMED_FLOATS, N_REF, NAMES, OK, REFUSALS, canonical_texts, f32, float_bits, rec
from test_gpu_bam import _fq
from test_host_boundary import _setup

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -3, -4, -6
HEADER = bam.header_block(b"@HD\tVN:1.6\n", NAMES, [1 << 31 - 1, 5000, 70])
COUNTS = ("records", "lines", "filtered", "bytes", "adds")


def counts(v) -> tuple:
    i = v.info()
    return tuple(i[k] for k in COUNTS)


def check_add(v, recs, names=NAMES, require=0, exclude=0, min_mapq=0) -> bytes:
    """One add of recs (a list of records) on handle v, whose filter the keywords restate: the lines, fetch(), out() and the
    info() counts against the restatement; -> the text"""
    before = counts(v)
    want, woff = samview.view(recs, names, require, exclude, min_mapq)
    assert v.add_records(b"".join(recs)) == len(woff) - 1
    text, off = v.fetch()
    assert text == want
    assert off.dtype == np.int64 and np.array_equal(off, woff)
    o = v.out()
    assert (o.n_bytes, o.n_lines, o.n_records) == (len(want), len(woff) - 1, len(recs))
    assert bool(o.text) == bool(want) and o.line_off
    n_lines = len(woff) - 1
    assert counts(v) == (before[0] + len(recs), before[1] + n_lines, before[2] + len(recs) - n_lines, before[3] + len(want), before[4] + 1)
    return text


@pytest.fixture(scope="module")
def view():
    v = capi.SamView(HEADER)
    yield v
    v.close()


def test_literal_pairs_and_canonical_texts(view):
    assert view.fetch() == (b"", [0]) and counts(view) == (0, 0, 0, 0, 0)           # V1: empty before any add
    assert check_add(view, [r for _, r, _ in LITERALS]) == b"".join(ln for _, _, ln in LITERALS)
    for names, text in canonical_texts():
        v = capi.SamView(bam.header_block(b"", names, [1000000] * len(names)), opt=False)
        try:
            assert check_add(v, bam.split_records(bam.encode_records(text, names)), names) == text
        finally:
            v.close()


def _bases(rng, n: int) -> bytes:
    return bytes(np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)[rng.integers(0, 16, n)])


def _quals(rng, n: int) -> bytes:
    q = rng.integers(0, 94, n).astype(np.uint8)
    return bytes(q)


def _cigar(rng, n: int):
    return [(int(ln), int(o)) for ln, o in zip(rng.integers(1, 100000, n), rng.integers(0, 9, n))]


def limit_records():
    rng = np.random.default_rng(41)
    out = []
    for ln in (1, 15, 16, 17, 254):                                                  # names
        out.append(rec(b"n" * ln, 0, 0, 10 + ln, 3, [(ln, 0)], _bases(rng, ln), _quals(rng, ln)))
    for ls in (0, 1, 2, 15, 16, 17, 31, 32, 33, 70000):                              # SEQ and QUAL; every second QUAL absent
        out.append(rec(b"s%d" % ls, 16, 1, 7, 60, [(ls, 0)] if ls else [], _bases(rng, ls), _quals(rng, ls) if ls % 2 == 0 else None))
    for n in (0, 1, 16, 17, 65535):                                                  # CIGAR
        out.append(rec(b"c%d" % n, 0, 0, 100, 9, _cigar(rng, n), b"ACGT", _quals(rng, 4)))
    out.append(rec(b"cmax", 0, 0, 100, 9, [((1 << 28) - 1, 3), (1, 0), ((1 << 28) - 1, 8)], b"A", [0]))
    out.append(rec(b"lo", 0, -1, -1, 0, [], tlen=-(1 << 31), pnext=-1))              # the fixed fields' ends
    out.append(rec(b"hi", 65535, 0, (1 << 31) - 2, 255, [], nrefid=2, pnext=(1 << 31) - 2, tlen=(1 << 31) - 1))
    ints = b"".join(b"X%c%c" % (48 + k, t) + struct.pack(f, x) for k, (t, f, x) in enumerate(
        [(99, "<b", -128), (99, "<b", 127), (67, "<B", 0), (67, "<B", 255), (115, "<h", -32768), (115, "<h", 32767), (83, "<H", 0),
         (83, "<H", 65535), (105, "<i", -(1 << 31)), (105, "<i", (1 << 31) - 1), (73, "<I", 0), (73, "<I", (1 << 32) - 1)]))
    out.append(rec(b"ints", 4, aux=ints))
    out.append(rec(b"zh", 4, aux=b"Z0Z\0" + b"Z1Z" + b"a" * 16 + b"\0" + b"Z2Z" + b"b" * 17 + b"\0" + b"H0H00FFA1\0" + b"Z3Z" + b"c" * 300 + b"\0"))
    out.append(rec(b"many", 4, seq=b"ACG", qual=[1, 2, 3], aux=b"".join(
        [b"A%cC%c" % (65 + k % 26, k) for k in range(50)] + [b"Z%cZ%s\0" % (65 + k % 26, b"v" * k) for k in range(50)])))
    vals = {b"c": ("<b", -128, 128), b"C": ("<B", 0, 256), b"s": ("<h", -32768, 32768), b"S": ("<H", 0, 65536),
            b"i": ("<i", -(1 << 31), 1 << 31), b"I": ("<I", 0, 1 << 32)}
    bits = float_bits()
    for n in (0, 1, 16, 17, 1000):                                                   # B arrays
        aux = b""
        for sub, (f, lo, hi) in vals.items():
            x = rng.integers(lo, hi, n)
            if n > 1:
                x[0], x[-1] = lo, hi - 1
            aux += b"B" + sub + b"B" + sub + struct.pack("<I", n) + b"".join(struct.pack(f, int(v)) for v in x)
        aux += b"BfBf" + struct.pack("<I", n) + bits[rng.integers(0, len(bits), n)].astype("<u4").tobytes()
        out.append(rec(b"b%d" % n, 4, aux=aux))
    named = np.concatenate([np.array(NAMED_FLOATS, np.float32).view(np.uint32), np.array(NAMED_BITS, np.uint32), bits[::97]])
    for k in range(0, len(named), 40):                                               # f values, as fields of their own
        out.append(rec(b"f%d" % k, 4, aux=b"".join(b"f%cf" % (48 + j) + struct.pack("<I", int(b)) for j, b in enumerate(named[k:k + 40]))))
    out.append(rec(b"fB", 4, aux=b"FAf" + f32(0.5) + b"FBBf" + struct.pack("<I", len(bits)) + bits.astype("<u4").tobytes()))
    return out


def test_field_limits(view):
    recs = limit_records()
    text = check_add(view, recs)
    assert b"\t65535\tchr1\t2147483647\t255\t*\tchrUn_alt\t2147483647\t2147483647\t" in text
    assert b"lo\t0\t*\t0\t0\t*\t*\t0\t-2147483648\t*\t*\n" in text and b"\t268435455N1M268435455X\t" in text
    check_add(view, recs[::-1])                                                       # other alignments of every store


def _small(k: int) -> bytes:
    return rec(b"r%d" % k, (k * 37) & 0xFFF, k % 3, k * 11, k % 61, [(50 + k % 7, 0)], b"ACGTN"[:1 + k % 5] * 3, None if k % 4 == 0 else [k % 40] * (3 + 3 * (k % 5)),
               aux=b"NMC" + bytes([k % 200]) + (b"MDZ%d\0" % k if k % 2 else b""))


def test_record_counts(view):
    """adds that straddle a lane group, a wave, a block and the grid's stride; each add's output replaces the last"""
    last = None
    for n in (0, 1, 15, 16, 17, 4097, 17, 0):
        text = check_add(view, [_small(k) for k in range(n)])
        assert text.count(b"\n") == n and (n == 0 or text != last)
        last = text
    assert view.fetch() == (b"", [0])
    cycle = [_small(k) for k in range(7)]
    lines = [samview.format_record(r, NAMES) for r in cycle]
    n = 16 * 16 * 512 + 17                                                           # past one stride of the largest grid (16 blocks a CU)
    assert view.add_records(b"".join(cycle[k % 7] for k in range(n))) == n
    text, off = view.fetch()
    assert text == b"".join(lines[k % 7] for k in range(n)) and len(off) == n + 1 and off[-1] == len(text)


def test_filter():
    recs = [_small(k) for k in range(300)] + [r for _, r, _ in LITERALS]
    for req, exc, mq in ((0x10, 0, 0), (0, 0x4, 0), (0, 0, 30), (0x41, 0x804, 17), (0, 0, 255), (0xFFFF, 0xFFFF, 0)):
        v = capi.SamView(HEADER, require=req, exclude=exc, min_mapq=mq)
        try:
            check_add(v, recs, NAMES, req, exc, mq)
            i = v.info()
            assert i["filtered"] > 0 and i["lines"] + i["filtered"] == len(recs)
        finally:
            v.close()
    v = capi.SamView(HEADER, exclude=0, require=0, min_mapq=256)                     # everything is filtered
    try:
        assert check_add(v, recs, NAMES, 0, 0, 256) == b"" and v.fetch()[1].tolist() == [0] and not v.out().text
        with pytest.raises(capi.BwamsError) as e:                                     # a filtered record with a fault still refuses
            v.add_records(b"".join(recs[:20]) + REFUSALS[0][1])
        assert e.value.code == ERR_UNSUPPORTED and "record 20:" in str(e.value)
    finally:
        v.close()


def test_refusals(view):
    good = [_small(k) for k in range(40)]
    kept = check_add(view, good)
    before = counts(view)
    L = capi.lib()
    n = C.c_int64(-1)
    for what, r, why in REFUSALS:
        for at in (0, 17, 39):
            data = b"".join(good[:at]) + r + b"".join(good[at:])
            assert L.bwams_samview_add_records(view.h, data, len(data), C.byref(n)) == ERR_UNSUPPORTED, what
            assert L.bwams_last_error().decode() == "bwams_samview_add_records: record %d: %s" % (at, samview.REASONS[why]), what
            assert samview.check(data, N_REF) == (at, samview.REASONS[why])
    first = {w: r for _, r, w in reversed(REFUSALS)}
    for a, b, ia, ib in ((5, 1, 33, 2), (3, 4, 16, 15), (2, 5, 0, 39), (1, 3, 70, 69)):                # two faults: the smaller ordinal
        recs = good + good
        recs[ia], recs[ib] = first[a], first[b]
        data = b"".join(recs)
        k, why = (ia, a) if ia < ib else (ib, b)
        assert L.bwams_samview_add_records(view.h, data, len(data), C.byref(n)) == ERR_UNSUPPORTED
        assert L.bwams_last_error().decode() == "bwams_samview_add_records: record %d: %s" % (k, samview.REASONS[why])
    assert n.value == -1 and view.fetch()[0] == kept and counts(view) == before       # the handle as it was
    assert view.out().n_records == len(good)


def test_front_door(view):
    L = capi.lib()
    h = C.c_void_p()
    for blk in (HEADER[:-1], HEADER[:10], b"BAM\2" + HEADER[4:], b"", HEADER[:len(HEADER) - 9]):
        assert L.bwams_samview_open(0, blk, len(blk), None, C.byref(h)) == ERR_ARG and not h
    with pytest.raises(capi.BwamsError) as e:
        capi.SamView(HEADER, reserved=1)
    assert e.value.code == ERR_ARG
    with pytest.raises(capi.BwamsError) as e:
        capi.SamView(HEADER, device=1 << 20)
    assert L.bwams_samview_close(None) == 0
    kept = check_add(view, [_small(k) for k in range(9)])
    for data in (OK[:-1], OK + b"\x01\x02", struct.pack("<I", 8) + b"\0" * 8):        # malformed chains, as the other consumers refuse them
        with pytest.raises(capi.BwamsError) as e:
            view.add_records(data)
        assert e.value.code == ERR_ARG
    with pytest.raises(capi.BwamsError) as e:
        view.fetch(cap=len(kept) - 1)
    assert e.value.code == ERR_CAPACITY
    off = np.zeros(10, np.int64)
    assert L.bwams_samview_fetch(view.h, None, 0, capi._p(off)) == 0 and off[-1] == len(kept)      # either pointer NULL
    assert L.bwams_samview_fetch(view.h, None, 0, None) == 0
    assert view.fetch()[0] == kept


@pytest.fixture(scope="module", params=["plain", "alt"])
def toy(request):
    """three sequences; "alt": the last an ALT one, as tests/test_gpu_bam.py has it, so that hits on it carry bwa's pa:f:%.3f"""
    g, ix, contigs, names = _setup(seed=31)
    if request.param == "plain":
        contigs["is_alt"] = 0
        ix.set_contigs(contigs)
        ix.set_contig_names(names)
    yield g, ix, [n.encode() for n in names], request.param
    ix.close()


def _canonical_floats(text: bytes) -> bytes:
    """the text with every f field as "%g" prints its float: what is left of "%.3f" once the value has been a float in a record"""
    out = []
    for ln in text.split(b"\n"):
        out.append(b"\t".join(f[:5] + samview.fmt_g(float(f[5:])) if f[2:5] == b":f:" else f for f in ln.split(b"\t")))
    return b"\n".join(out)


def test_round_trip_through_the_pipeline(toy):
    """text -> bwams_bam_run -> view == text byte for byte (but for the digits "%.3f" prints and "%g" does not, where an ALT
    sequence brings pa:f fields), and the flags of bwams_bam_markdup show in the lines"""
    g, ix, names, kind = toy
    rng = np.random.default_rng(8)
    pairs = simulate.make_read_pairs(g, 300, seed=17, damaged_frac=0.2, discordant_frac=0.05)
    reads = list(pairs) + list(pairs[:80])                                            # forty pairs twice: duplicates
    rn = [b"p%d" % (i // 2) for i in range(len(pairs))] + [b"d%d" % (i // 2) for i in range(80)]
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    v = capi.SamView(ix.bam_header(b"@HD\tVN:1.6\n"))
    empty = capi.Batch(ix, 16, 16 * 160)
    try:
        with pytest.raises(capi.BwamsError) as e:                                     # a batch without BAM records
            v.add_batch(empty)
        assert e.value.code == ERR_ARG and "bwams_bam_run" in str(e.value)
        b.process_chunk(_fq(reads, rn, rng), paired=True)
        text, _, _ = b.sam_fetch()
        _, nr = b.bam_run()
        assert v.add_batch(b) == nr == text.count(b"\n")
        got, off = v.fetch()
        if kind == "plain":
            assert b":f:" not in text and got == text
        else:
            assert b"\tpa:f:" in text and got == _canonical_floats(text) == samview.view(b.bam_fetch()[0], names)[0]
        assert off[-1] == len(got) and len(off) == nr + 1
        st = b.bam_markdup()
        assert st.records_marked > 0
        rec_marked, _ = b.bam_fetch()
        assert v.add_batch(b) == nr
        marked, moff = v.fetch()
        want, woff = samview.view(rec_marked, names)
        assert marked == want and np.array_equal(moff, woff)
        flags = lambda t: [int(ln.split(b"\t")[1]) for ln in t.split(b"\n")[:-1]]
        assert sum(bool(f & 0x400) for f in flags(marked)) == st.records_marked and not any(f & 0x400 for f in flags(got))
        assert [f & ~0x400 for f in flags(marked)] == flags(got)
    finally:
        v.close(); b.close(); empty.close()


def test_file_pieces_regions_and_marks(tmp_path):
    rng = np.random.default_rng(29)
    lines = Q.named_lines(rng) + Q.background(rng, 3200, unplaced=30)
    dups = [Q.line(b"dup%d" % k, 1, 60000, b"80M", 0, rng) for k in range(6)]         # six fragments at one place: five duplicates
    records = Q.encode(lines + dups)
    p = tmp_path / "sorted.bam"
    p.write_bytes(Q.bam_file(records, 300))
    (tmp_path / "sorted.bam.bai").write_bytes(bai.build(p.read_bytes()))
    f = capi.BamFile(str(p), piece_bytes=65536)
    v = capi.SamView(f.header_block())
    j = capi.DupJoin()
    try:
        with pytest.raises(capi.BwamsError) as e:                                     # a file with no current piece
            v.add_file(f)
        assert e.value.code == ERR_ARG
        f.query()
        got, n_pieces = [], 0
        for piece in f.pieces():
            recs, _ = piece.fetch()
            want, woff = samview.view(recs, Q.NAMES)
            assert v.add_file(piece) == len(woff) - 1 == piece.n_records
            text, off = v.fetch()
            assert text == want and np.array_equal(off, woff)
            got.append(text)
            n_pieces += 1
        assert n_pieces >= 3
        assert b"".join(got) == samview.view(records, Q.NAMES)[0]
        regions = [Q.R_EDGE, (0, 100000, 160000)]
        f.query(regions)
        got = []
        for piece in f.pieces():
            recs, _ = piece.fetch()
            assert v.add_file(piece) == piece.n_records
            assert v.fetch()[0] == samview.view(recs, Q.NAMES)[0]
            got.append(v.fetch()[0])
        assert b"".join(got) == b"".join(samview.format_record(r, Q.NAMES) for r in Q.brute(records, regions)) != b""
        f.query()                                                                     # marks applied to a piece show in its lines
        for piece in f.pieces():
            j.add_file(piece)
        j.finish()
        f.query()
        n_marked = 0
        for piece in f.pieces():
            n = j.apply_file(piece)
            v.add_file(piece)
            text = v.fetch()[0]
            assert text == samview.view(piece.fetch()[0], Q.NAMES)[0]
            assert sum(bool(int(ln.split(b"\t")[1]) & 0x400) for ln in text.split(b"\n")[:-1]) == n
            n_marked += n
        assert n_marked >= 5
    finally:
        j.close(); v.close(); f.close()


def test_fetch_bgzf(view):
    d = capi.Deflater(0, 64 << 20)
    try:
        check_add(view, [_small(k) for k in range(3000)] + limit_records()[:12])
        text, _ = view.fetch()
        gz = view.fetch_bgzf(d, eof=True)
        assert gz.endswith(bgzf.EOF_MEMBER) and gz == d.run(text, eof=True)[0]       # the same deflater over the same bytes
        out, p = [], 0
        while p < len(gz):                                                            # member by member, with Python's zlib
            (bsize,) = struct.unpack_from("<H", gz, p + 16)
            out.append(zlib.decompress(gz[p + 18:p + bsize + 1 - 8], -15))
            p += bsize + 1
        assert b"".join(out) == text and len(out) > 3
        plain = view.fetch_bgzf(d)                                                    # without the EOF member
        assert gzip.decompress(plain) == text and plain + bgzf.EOF_MEMBER == gz
        check_add(view, [])
        assert view.fetch_bgzf(d, eof=True) == bgzf.EOF_MEMBER
        L = capi.lib()
        buf, n = C.create_string_buffer(64), C.c_int64(0)
        assert L.bwams_samview_fetch_bgzf(view.h, None, C.addressof(buf), 64, 0, C.byref(n)) == ERR_ARG
    finally:
        d.close()
