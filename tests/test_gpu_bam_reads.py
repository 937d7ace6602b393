"""BAM as read input on the GPU (csrc/bam_reads.hip, bwams_process_chunk_bam*, bwams_reader_open_bam) against bwams/bam_reads.py,
against bwams_fastq_decode of the equivalent FASTQ text, and round the project's own BAM.  All comparisons are exact."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from bwams import bam, bam_reads, bgzf, capi, simulate
from bam_reads_util import NT16, fetched, many_records, rand_qual, rand_seq, rec, same_reads
from test_gpu_inflate import _damaged
from test_host_boundary import _setup

pytestmark = pytest.mark.gpu

ERR_IO, ERR_ARG, ERR_UNSUPPORTED = -2, -3, -6
MEM_F_ALL = 0x8


def _same_handles(a: capi.Fastq, b: capi.Fastq):
    """two decoded chunks, array for array"""
    x, y = a.fetch(), b.fetch()
    assert x["n"] == y["n"] and a.info()["name_bytes"] == b.info()["name_bytes"] and a.info()["comment_bytes"] == b.info()["comment_bytes"]
    for k in ("enc", "cum"):
        assert np.array_equal(x[k], y[k]), k
    assert (x["quals"] is None) == (y["quals"] is None) and (x["quals"] is None or np.array_equal(x["quals"], y["quals"]))
    assert x["names"] == y["names"] and x["comments"] == y["comments"]


def _decode_checked(records: bytes, tags: bytes = b"", fastq: bool = True) -> capi.Fastq:
    """decode from host memory; == the restatement, == the same bytes from device memory, == bwams_fastq_decode of to_fastq"""
    want = bam_reads.reads(records, tags)
    f = capi.bam_reads_decode(0, records, tags)
    assert (f.n_records, f.n_reads, f.n_bases) == bam_reads.count(records)
    same_reads(fetched(f), want)
    dev = torch.empty(len(records) + 3, dtype=torch.uint8, device="cuda:0")
    for shift in (0, 3):                                       # an aligned and an odd device address
        dev[shift:shift + len(records)] = torch.frombuffer(bytearray(records), dtype=torch.uint8).to("cuda:0")
        g = capi.bam_reads_decode(0, dev.data_ptr() + shift, tags, n_bytes=len(records))
        _same_handles(f, g)
        g.close()
    if fastq:
        t = capi.Fastq(bam_reads.to_fastq(records, tags))
        _same_handles(f, t)
        t.close()
    return f


# ------------------------------------------------------------------------------------------------------------- 1. hand-built cases
def _decoy_record() -> bytes:
    """the bytes of a complete, well-formed little record whose bytes are all valid quality values (< 0xDE) and not 0xFF first"""
    body = struct.pack("<iiBBHHHiiii", 0, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0) + b"\x30\0" + b"\x10" + b"\x05" + b"\0" * 4
    return struct.pack("<I", len(body)) + body


def test_hand_built_cases():
    rng = np.random.default_rng(11)
    q16 = bytes(range(40, 56))
    aux = [b"BC:Z:ACGT", b"RG:Z:grp", b"XA:A:q", b"XH:H:1AE3", b"RG:Z:second"]
    ints = [b"X%d:i:%d" % (k, v) for k, v in enumerate([-128, 255, -32768, 65535, -(1 << 31), (1 << 32) - 1, 0, -1])]
    rs = [rec(b"skipped-first", 0x100, b"", None),
          rec(b"fwd", 0, b"ACGTN", b"!#5?I", aux), rec(b"rev", 0x10, b"AACGN", b"!#5?I", aux[::-1]),
          rec(b"n16", 0, NT16, q16), rec(b"r16", 0x10, NT16, q16, ints)]
    for l in (1, 2, 3, 151):
        for flag in (0, 0x10):
            rs.append(rec(b"len%d_%d" % (l, flag), flag, rand_seq(rng, l), rand_qual(rng, l), ints[l % 8:l % 8 + 2]))
    rs += [rec(b"run%d" % k, f, rand_seq(rng, 9), rand_qual(rng, 9)) for k, f in enumerate([0x100, 0x800, 0x900, 0x110])]
    rs += [rec(b"N", 0, rand_seq(rng, 33), rand_qual(rng, 33)), rec(b"L" * 254, 0x10, rand_seq(rng, 34), rand_qual(rng, 34), aux)]
    for n_cig in (0, 1, 300):
        rs.append(rec(b"cig%d" % n_cig, 0, rand_seq(rng, 300), rand_qual(rng, 300), [b"RG:Z:c%d" % n_cig], cigar=b"1M" * n_cig or b"*"))
    rs.append(rec(b"long", 0x10, rand_seq(rng, 10001), rand_qual(rng, 10001), [b"NM:i:77", b"XF:f:1.5"]))
    decoy = _decoy_record()
    arr = b"XBBC" + struct.pack("<I", len(decoy)) + decoy                  # a byte array that holds a whole record
    rs.append(rec(b"decoy-aux", 0, rand_seq(rng, 40), rand_qual(rng, 40), [b"RG:Z:d"], raw_aux=arr + b"NMC\x09"))
    qual = decoy + bytes(rng.integers(0, 42, 60 - len(decoy)).astype(np.uint8))
    rs.append(rec(b"decoy-qual", 0, rand_seq(rng, 60), bytes(v + 33 for v in qual)))
    rs.append(rec(b"skipped-last", 0x800, rand_seq(rng, 5), rand_qual(rng, 5)))
    records = b"".join(rs)
    assert bam_reads.record_offsets(records + decoy)[-1] == len(records)   # the decoy is a record in its own right
    for tags in (b"", b"RG", b"NMRGXAXHBC", b"".join(b"X%d" % k for k in range(8)) + b"ZZ"):
        f = _decode_checked(records, tags)
        i = capi.bam_reads_info(f)
        assert i["n_records"] == len(rs) and i["n_candidates"] >= len(rs) + 2   # both decoys pass the filter; the chain skips them
        f.close()
    # a Z value that holds a record's bytes up to its first NUL, aux not walked; and a lone record
    z = rec(b"decoy-z", 0, rand_seq(rng, 40), rand_qual(rng, 40), raw_aux=b"XZZ" + decoy + b"\0")
    _decode_checked(z + rs[1] + z).close()
    _decode_checked(rs[1], b"RG").close()


def test_no_qualities_anywhere():
    records = rec(b"a", 0, b"ACGTN", None) + rec(b"s", 0x100, b"AC", b"II") + rec(b"b", 0x10, b"AAC", None, [b"RG:Z:g"])
    f = _decode_checked(records, b"RG")                                    # to_fastq gives FASTA text: has_qual 0 on both sides
    assert f.fetch()["quals"] is None
    f.close()


# ------------------------------------------------------------------------------------------------------------------ 2. long chain
def test_long_chain():
    records, want = many_records(70000, 3)
    f = capi.bam_reads_decode(0, records, b"RGNM")
    got = f.fetch()
    i = capi.bam_reads_info(f)
    f.close()
    assert f.n_records == 70000 == i["n_records"] and f.n_reads == len(want) and i["n_candidates"] >= 70000
    rs = bam_reads.reads(records, b"RGNM")
    same_reads(rs, want)                                                   # the restatement and the builder agree
    assert np.array_equal(got["enc"], np.concatenate([r[1] for r in rs]))
    assert bytes(got["quals"]) == b"".join(r[2] for r in rs)
    assert np.array_equal(got["cum"], np.concatenate([[0], np.cumsum([len(r[1]) for r in rs])]))
    assert got["names"] == [r[0] for r in rs] and [c or b"" for c in got["comments"]] == [r[3] for r in rs]


# -------------------------------------------------------------------------------------------------------------------- 3. refusals
def _refused(records: bytes, tags: bytes, code: int, ordinal: int, offset: int):
    with pytest.raises(capi.BwamsError) as e:
        capi.bam_reads_decode(0, records, tags)
    assert e.value.code == code, str(e.value)
    assert "record %d at byte %d" % (ordinal, offset) in str(e.value), str(e.value)
    with pytest.raises((bam_reads.BadRecord, bam_reads.Unsupported)) as w:           # the restatement refuses the same record
        bam_reads.reads(records, tags)
    assert (w.value.ordinal, w.value.offset) == (ordinal, offset)
    assert isinstance(w.value, bam_reads.BadRecord) == (code == ERR_ARG)
    ok = capi.bam_reads_decode(0, rec(b"fine", 0, b"ACGT", b"IIII"))                 # the device is as good as before
    assert ok.n_reads == 1
    ok.close()


A = rec(b"a", 0, b"ACGTA", b"IIIII", [b"RG:Z:g"])
B = rec(b"b", 0x10, b"ACG", b"III")
WORSE = struct.pack("<I", 7) + B[4:]                                       # planted behind the record under test: "earliest" holds
REFUSALS = {
    "block_size_31": (A + struct.pack("<I", 31) + B[4:] + WORSE, b"", ERR_ARG, 1, len(A)),
    "overshoot_by_one": (A + B + struct.pack("<I", len(B) - 3) + B[4:], b"", ERR_ARG, 2, len(A) + len(B)),
    "truncated_last": (A + B[:-1], b"", ERR_ARG, 1, len(A)),
    "truncated_fixed_part": (A + B[:20], b"", ERR_ARG, 1, len(A)),
    "l_seq_max": (A + B[:20] + struct.pack("<i", (1 << 31) - 1) + B[24:] + WORSE, b"", ERR_ARG, 1, len(A)),
    "l_seq_negative": (A + B[:20] + struct.pack("<i", -1) + B[24:] + WORSE, b"", ERR_ARG, 1, len(A)),
    "l_read_name_0": (A + B[:12] + b"\0" + B[13:] + WORSE, b"", ERR_ARG, 1, len(A)),
    "name_without_nul": (A + B[:37] + b"x" + B[38:] + WORSE, b"", ERR_ARG, 1, len(A)),
    "first_record": (B[:37] + b"x" + B[38:] + A + WORSE, b"", ERR_ARG, 0, 0),
    "aux_past_the_record": (A + rec(b"c", 0, b"AC", b"II", raw_aux=b"RGZabc") + rec(b"d", 0, b"AC", b"II", raw_aux=b"RGZab"), b"RG",
                            ERR_ARG, 1, len(A)),
    "aux_unknown_type": (A + B + rec(b"c", 0, b"AC", b"II", raw_aux=b"XY?\1"), b"RG", ERR_ARG, 2, len(A) + len(B)),
    "listed_float": (A + rec(b"c", 0, b"AC", b"II", [b"XF:f:1.5"]) + rec(b"d", 0, b"", None), b"RGXF", ERR_UNSUPPORTED, 1, len(A)),
    "listed_array": (A + rec(b"c", 0, b"AC", b"II", raw_aux=b"XBBs" + struct.pack("<Ih", 1, 5)), b"XB", ERR_UNSUPPORTED, 1, len(A)),
    "mixed_qualities": (A + rec(b"s", 0x100, b"AC", None) + rec(b"c", 0, b"AC", None) + rec(b"d", 0, b"", None), b"", ERR_UNSUPPORTED, 2,
                        len(A) + len(rec(b"s", 0x100, b"AC", None))),
    "mixed_qualities_first_without": (rec(b"c", 0, b"AC", None) + B + A, b"", ERR_UNSUPPORTED, 1, len(rec(b"c", 0, b"AC", None))),
    "l_seq_0": (A + B + rec(b"c", 0, b"", None) + rec(b"d", 0, b"AC", None), b"", ERR_UNSUPPORTED, 2, len(A) + len(B)),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(case):
    _refused(*REFUSALS[case])


def test_tag_lists_and_inputs_without_reads():
    for tags in (b"RGB", b"AB" * 33):
        with pytest.raises(capi.BwamsError) as e:
            capi.bam_reads_decode(0, A, tags)
        assert e.value.code == ERR_ARG
    # rule 7: no read at all is what bwams_fastq_decode makes of a text without records — a handle without reads
    L = capi.lib()
    h, n, nb = C.c_void_p(), C.c_int64(-1), C.c_int64(-1)
    want = L.bwams_fastq_decode(0, b"", C.c_int64(0), C.byref(h), C.byref(n), C.byref(nb))
    assert want == 0 and n.value == 0
    L.bwams_fastq_close(h)
    for records, n_rec in ((b"", 0), (rec(b"s", 0x100, b"AC", b"II") + rec(b"t", 0x900, b"", None), 2)):
        h, n, nb, nr = C.c_void_p(), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        rc = L.bwams_bam_reads_decode(0, C.cast(C.c_char_p(records), C.c_void_p), len(records), b"RG", C.byref(h), C.byref(n), C.byref(nb),
                                      C.byref(nr))
        assert rc == want and (n.value, nb.value, nr.value) == (0, 0, n_rec)
        f = capi.Fastq(None)
        f.h = h
        assert f.fetch()["n"] == 0
        f.close()


# ------------------------------------------------------------------------------------- 4. round the project's own BAM, and to SAM
def _fq(reads, names, rng):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (nm, bytes(b"ACGTN"[c] for c in r), rand_qual(rng, len(r))) for nm, r in zip(names, reads))


@pytest.fixture(scope="module")
def toy():
    g, ix, _, names = _setup(seed=31)
    yield g, ix
    ix.close()


@pytest.fixture(scope="module")
def aligned(toy):
    """3000 simulated reads as FASTQ, their SAM (MEM_F_ALL) and that SAM as BAM records"""
    g, ix = toy
    reads, _, _ = simulate.make_reads(g, 3000, seed=72)
    text = _fq(reads, [b"s%d" % i for i in range(len(reads))], np.random.default_rng(9))
    b = capi.Batch(ix, 3000, 3000 * 160)
    sam, _ = b.process_chunk(text, sopt=capi.default_sam_opt(MEM_F_ALL))
    b.bam_run()
    records, _ = b.bam_fetch()
    plain, _ = b.process_chunk(text)
    b.close()
    return text, bytes(records), plain


def _flags(records: bytes):
    return [struct.unpack_from("<H", records, q + 18)[0] for q in bam_reads.record_offsets(records)]


def test_round_trip_single_end(toy, aligned):
    g, ix = toy
    text, records, plain = aligned
    fl = _flags(records)
    assert any(f & 0x10 for f in fl) and any(f & 0x900 for f in fl) and len(fl) > 3000       # otherwise this test shows nothing
    f, t = capi.bam_reads_decode(0, records), capi.Fastq(text)
    assert f.n_reads == 3000 and f.n_records == len(fl)
    x, y = f.fetch(), t.fetch()
    assert x["names"] == y["names"] and np.array_equal(x["enc"], y["enc"]) and np.array_equal(x["quals"], y["quals"])
    assert np.array_equal(x["cum"], y["cum"])
    f.close(); t.close()
    b = capi.Batch(ix, 3000, 3000 * 160)
    try:
        sam, off = b.process_chunk_bam(records)
        assert sam == plain and len(off) == 3001
        dev = torch.frombuffer(bytearray(records), dtype=torch.uint8).to("cuda:0")
        sam2, _ = b.process_chunk_bam((dev.data_ptr(), len(records)))
        assert sam2 == plain
        offs = bam_reads.record_offsets(records)
        last_kept = max(k for k, f in enumerate(fl) if not f & 0x900)
        with pytest.raises(capi.BwamsError) as e:                          # 2999 reads are not pairs
            b.process_chunk_bam(records[:offs[last_kept]], paired=True)
        assert e.value.code == ERR_ARG and "even number" in str(e.value)
    finally:
        b.close()


def test_round_trip_paired_and_smart(toy):
    g, ix = toy
    rng = np.random.default_rng(6)
    pr = simulate.make_read_pairs(g, 1500, seed=12, damaged_frac=0.2, discordant_frac=0.05)
    text = _fq(pr, [b"p%d" % (i // 2) for i in range(len(pr))], rng)
    b = capi.Batch(ix, len(pr), len(pr) * 160)
    try:
        want, _ = b.process_chunk(text, paired=True)
        b.bam_run()
        records = bytes(b.bam_fetch()[0])
        fl = _flags(records)
        assert any(f & 0x10 for f in fl) and all(f & 1 for f in fl)
        f, t = capi.bam_reads_decode(0, records), capi.Fastq(text)
        _same_handles(f, t)
        f.close(); t.close()
        got, _ = b.process_chunk_bam(records, paired=True)
        assert got == want
        # singles and pairs mixed: the pair of _smart calls
        singles, _, _ = simulate.make_reads(g, 200, seed=15)
        reads, rn = [], []
        for i in range(300):
            reads += [pr[2 * i], pr[2 * i + 1]]
            rn += [b"frag%d" % i] * 2
            if i < 200:
                reads.append(singles[i]); rn.append(b"solo%d" % i)
        mixed = _fq(reads, rn, rng)
        want, _, n_single = b.process_chunk_smart(mixed)
        b.bam_run()
        records = bytes(b.bam_fetch()[0])
        got, _, n1 = b.process_chunk_bam_smart(records)
        assert got == want and n1 == n_single == 200
    finally:
        b.close()


def test_read_group_tag_reaches_the_sam_text(toy, aligned):
    g, ix = toy
    text = aligned[0]
    b = capi.Batch(ix, 3000, 3000 * 160)
    try:
        b.process_chunk(text, sopt=capi.default_sam_opt(0, b"x"))
        b.bam_run()
        records = bytes(b.bam_fetch()[0])
        assert records.count(b"RGZx\0") == len(_flags(records))
        sam, _ = b.process_chunk_bam(records, tags=b"RG", copy_comment=True)
        lines = sam.split(b"\n")[:-1]
        assert len(lines) >= 3000 and all(ln.endswith(b"\tRG:Z:x") for ln in lines)
        none, _ = b.process_chunk_bam(records, tags=b"RG")                 # without COPY_COMMENT the comments are dropped
        assert b"RG:Z:x" not in none
        b.process_chunk_bam(records, tags=b"RG", copy_comment=True)
        nb, nr = b.bam_run()                                               # the text is one bwams_bam_run accepts
        assert nr == len(lines) and bytes(b.bam_fetch()[0]).count(b"RGZx\0") == nr
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. reader
HEADER_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@CO\tline %06d of a long header %s\n" % (k, b"x" * 60) for k in range(1100)) + \
    b"@RG\tID:x\tSM:sample\n"


@pytest.fixture(scope="module")
def bam_file(tmp_path_factory, aligned):
    text, records, _ = aligned
    assert len(HEADER_TEXT) > 100000
    d = tmp_path_factory.mktemp("bam_reads")
    hdr = bam.header_block(HEADER_TEXT, [b"chrA", b"chrB", b"chrC_alt"], [90000, 110000, 100000])
    path = d / "in.bam"
    path.write_bytes(bgzf.compress(hdr + records, 6))
    assert len(bgzf.walk(path.read_bytes())) > 4
    fq = d / "in.fq"
    fq.write_bytes(bam_reads.to_fastq(records))
    return d, str(path), str(fq), hdr, records


@pytest.mark.parametrize("paired", [False, True])
def test_reader_chunks_equal_the_fastq_reader(bam_file, paired):
    d, path, fq, hdr, records = bam_file
    want = capi.reader_chunks(capi.reader_open(fq, 150000, paired, 0, 2))
    assert len(want) >= 3
    decoded = []
    for t, _, _ in want:
        f = capi.Fastq(t)
        decoded.append(f)
    try:
        for device in (0, -1):
            for n_buffers in (1, 2, 3):
                r = capi.reader_open_bam(path, device, 150000, paired, 0, n_buffers)
                assert capi.reader_bam_header(r) == (HEADER_TEXT, 3)
                assert capi.reader_info(r).device_inflate == (1 if device == 0 else 0)
                got = capi.reader_chunks(r)
                assert [(n, nb) for _, n, nb in got] == [(n, nb) for _, n, nb in want], (device, n_buffers)
                assert b"".join(c[0] for c in got) == records[:sum(len(c[0]) for c in got)]
                assert all(not f & 0x900 for f in _flags(records[sum(len(c[0]) for c in got):]))   # only skipped records may be left out
                if n_buffers == 2:
                    for (c, _, _), t in zip(got, decoded):
                        f = capi.bam_reads_decode(0, c)
                        _same_handles(f, t)
                        f.close()
    finally:
        for f in decoded:
            f.close()


def test_reader_to_sam(toy, bam_file):
    g, ix = toy
    d, path, fq, hdr, records = bam_file
    b = capi.Batch(ix, 1200, 1200 * 160)
    try:
        sams = []
        for chunks, run in ((capi.reader_chunks(capi.reader_open(fq, 150000, False, 0, 2)), b.process_chunk),
                            (capi.reader_chunks(capi.reader_open_bam(path, 0, 150000, False, 0, 2)), b.process_chunk_bam)):
            sam, done = b"", 0
            for t, n, _ in chunks:
                sam += run(t, n_processed=done)[0]
                done += n
            sams.append(sam)
            assert done == 3000
        assert sams[0] == sams[1] and sams[0].count(b"\n") >= 3000
    finally:
        b.close()


def test_reader_refusals(bam_file):
    d, path, fq, hdr, records = bam_file
    small = bam.header_block(b"@HD\tVN:1.6\n", [b"chrA"], [90000])

    def fails(name, blob, device=0):
        p = d / name
        p.write_bytes(blob)
        with pytest.raises(capi.BwamsError) as e:                          # at open (the header block) or from a chunk
            capi.reader_chunks(capi.reader_open_bam(str(p), device, 10 ** 6, False, 0, 2))
        return e.value

    offs = bam_reads.record_offsets(records)
    for device in (0, -1):
        e = fails("cut.bam", bgzf.compress(small + records[:-10], 6), device)
        assert e.code == ERR_IO and "inside a record" in str(e)
        e = fails("bad_record.bam", bgzf.compress(small + records[:offs[100]] + struct.pack("<I", 31) + records[offs[100] + 4:], 6), device)
        assert e.code == ERR_IO and "BAM record 100 is not well formed" in str(e)
        assert fails("text.bam", bgzf.compress(open(fq, "rb").read(), 6), device).code == ERR_UNSUPPORTED
        assert fails("cut_header.bam", bgzf.compress(hdr[:70000], 6), device).code == ERR_IO
    bad, k, ms = _damaged(bgzf.compress(small + records, 6), "crc")
    e = fails("damaged.bam", bad)
    assert e.code == ERR_IO and "BGZF member %d at byte %d" % (k, ms[k][0]) in str(e) and "CRC32" in str(e)
    with pytest.raises(capi.BwamsError) as e:                              # a reader of text has no BAM header
        r = capi.reader_open(fq, 10 ** 9, False, 0, 2)
        try:
            capi.reader_bam_header(r)
        finally:
            capi.lib().bwams_reader_close(r)
    assert e.value.code == ERR_ARG
