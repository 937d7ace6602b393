"""BAM written on the GPU (csrc/bam.hip: bwams_bam_run / _fetch / _fetch_bgzf, bwams_sam_header, bwams_bam_header,
bwams_writer_open_bam) against bwams/bam.py applied to the bytes bwams_sam_fetch returns: every SAM producer (single-end, paired-end,
process_chunk2, smart pairing, exact-match records), the SAM options that change the text, BGZF members, file to file, the refusals and
a chunk past one workgroup's worth of records."""
import ctypes as C
import gzip
import numpy as np
import pytest

from bwams import bam, bgzf, capi, simulate
from test_gpu_inflate import _chunks, _device_open
from test_host_boundary import _setup

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -3, -6
MEM_F_ALL, MEM_F_REF_HDR = 0x8, 0x100


@pytest.fixture(scope="module")
def deflater():
    d = capi.Deflater(0, 64 << 20)
    yield d
    d.close()


@pytest.fixture(scope="module")
def toy():
    g, ix, contigs, names = _setup(seed=31)                 # three sequences, the last an ALT one
    yield g, ix, contigs, [n.encode() for n in names]
    ix.close()


def _fq(reads, names, rng, comments=None, fasta=False):
    out = []
    for i, (nm, r) in enumerate(zip(names, reads)):
        s = bytes(b"ACGTN"[c] for c in r)
        c = b" " + comments[i] if comments is not None and comments[i] else b""
        if fasta:
            out.append(b">%s%s\n%s\n" % (nm, c, s))
        else:
            out.append(b"@%s%s\n%s\n+\n%s\n" % (nm, c, s, bytes((rng.integers(0, 41, len(r)) + 33).astype(np.uint8))))
    return b"".join(out)


def _check(b, ref_names, n_reads=None):
    """bwams_bam_fetch == bam.encode_records(bwams_sam_fetch text), offsets those of each read's records; returns (sam, records)"""
    text, off, _ = b.sam_fetch()
    nb, nr = b.bam_run()
    rec, boff = b.bam_fetch(n_reads)
    assert nr == text.count(b"\n") and nb == len(rec)
    want = bam.encode_records(text, ref_names)
    assert rec == want
    per_read = [len(bam.encode_records(text[off[i]:off[i + 1]], ref_names)) for i in range(len(off) - 1)]
    assert np.array_equal(boff, np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64))
    return text, rec


@pytest.mark.parametrize("paired", [False, True])
def test_process_chunk_records(toy, paired):
    g, ix, _, names = toy
    rng = np.random.default_rng(3)
    if paired:
        reads = simulate.make_read_pairs(g, 700, seed=12, damaged_frac=0.2, discordant_frac=0.05)
        rn = [b"p%d" % (i // 2) for i in range(len(reads))]
    else:
        reads, _, _ = simulate.make_reads(g, 1400, seed=72)
        rn = [b"s%d" % i for i in range(len(reads))]
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    try:
        sam, _ = b.process_chunk(_fq(reads, rn, rng), paired=paired)
        text, rec = _check(b, names)
        assert text == sam and b"\tchrC_alt\t" in text and (b"\t=\t" in text) == paired
        _, _, back = bam.decode(rec, names)
        assert back.count(b"\n") == text.count(b"\n")
    finally:
        b.close()


def test_process_chunk2_and_options(toy):
    """two FASTQ files of mates; MEM_F_ALL (secondaries with SEQ and QUAL '*'), MEM_F_REF_HDR (XR:Z), an RG id, copied comments"""
    g, ix, _, names = toy
    rng = np.random.default_rng(4)
    pr = simulate.make_read_pairs(g, 500, seed=13, damaged_frac=0.2)
    r1, r2 = pr[0::2], pr[1::2]
    nm = [b"f%d" % i for i in range(len(r1))]
    com = [b"BC:Z:ACGT\tXN:i:%d" % (i - 250) if i % 3 else None for i in range(len(r1))]
    ix.set_contig_annos([b"", b"annotation of B", b"ALT"])
    b = capi.Batch(ix, len(pr), len(pr) * 160)
    try:
        sopt = capi.default_sam_opt(MEM_F_ALL | MEM_F_REF_HDR, b"grp1")
        b.process_chunk2(_fq(r1, nm, rng, com), _fq(r2, nm, rng, com), sopt=sopt, copy_comment=True)
        text, _ = _check(b, names)
        assert b"\tRG:Z:grp1" in text and b"\tXR:Z:annotation of B" in text and b"\tBC:Z:ACGT" in text and b"\tXN:i:-" in text
        assert b"\t*\t*\t" in text or b"\t*\t*\n" in text
    finally:
        b.close()


def test_smart_and_fasta(toy):
    """process_chunk_smart (singles and pairs mixed, text merged from two runs) and FASTA reads (QUAL '*')"""
    g, ix, _, names = toy
    rng = np.random.default_rng(5)
    pr = simulate.make_read_pairs(g, 300, seed=14)
    singles, _, _ = simulate.make_reads(g, 200, seed=15)
    reads, rn = [], []
    for i in range(300):
        reads += [pr[2 * i], pr[2 * i + 1]]
        rn += [b"frag%d/1" % i, b"frag%d/2" % i]
        if i < 200:
            reads.append(singles[i]); rn.append(b"solo%d" % i)
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    try:
        b.process_chunk_smart(_fq(reads, rn, rng))
        _check(b, names)
        b.process_chunk(_fq(singles, [b"fa%d" % i for i in range(len(singles))], rng, fasta=True))
        text, rec = _check(b, names)
        assert b"\t*\n" in text or b"\t*\t" in text
    finally:
        b.close()


def test_exact_match_records(toy):
    """bwams_sam_run_emf's text (mem_perfect2sam_cont's records next to mem_reg2sam's)"""
    from bwams import emf
    g, ix, _, names = toy
    rng = np.random.default_rng(6)
    e = capi.Emf(ix, table=emf.build_emf(g, 150))
    reads = []
    for i in range(600):
        st = int(rng.integers(0, len(g) - 150))
        rd = g[st:st + 150].copy()
        if i % 2:
            rd = simulate.revcomp(rd)
        if i % 5 == 0:
            rd[int(rng.integers(0, 150))] ^= 1
        reads.append(rd)
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    try:
        b.process_chunk(_fq(reads, [b"e%d" % i for i in range(len(reads))], rng), emf=e)
        _check(b, names)
    finally:
        b.close()
        e.close()


def test_bgzf_members(toy, deflater):
    g, ix, _, names = toy
    rng = np.random.default_rng(7)
    reads, _, _ = simulate.make_reads(g, 2000, seed=16)
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    try:
        b.process_chunk(_fq(reads, [b"z%d" % i for i in range(len(reads))], rng))
        _, rec = _check(b, names)
        gz = b.bam_fetch_bgzf(deflater, eof=True)
        bgzf.walk(gz)
        assert gz.endswith(bgzf.EOF_MEMBER) and gzip.decompress(gz) == rec and len(rec) > 65280
        assert b.bam_fetch_bgzf(deflater, eof=True) == gz
        b.bam_run()
        assert b.bam_fetch_bgzf(deflater, eof=True) == gz
    finally:
        b.close()


def test_sam_and_bam_header(toy):
    g, ix, contigs, names = toy
    sq = b"".join(b"@SQ\tSN:%s\tLN:%d%s\n" % (n, int(c["len"]), b"\tAH:*" if c["is_alt"] else b"") for n, c in zip(names, contigs))
    pg = b"@PG\tID:bwa-mem2\tPN:bwa-mem2\tVN:x\tCL:bwa-mem2 mem ref r.fq\n"
    assert ix.sam_header() == sq
    assert ix.sam_header(None, pg) == sq + pg
    rg = b"@RG\tID:g1\tSM:s"
    assert ix.sam_header(rg, pg) == sq + rg + b"\n" + pg
    own = b"@SQ\tSN:mine\tLN:5\n@CO\thello"
    assert ix.sam_header(own, pg) == own + b"\n" + pg                 # -H text with its own @SQ lines: none from the index
    assert ix.sam_header(b"@CO\tnot @SQ\tSN:x", None) == sq + b"@CO\tnot @SQ\tSN:x\n"
    text = ix.sam_header(rg, pg)
    blk = ix.bam_header(text)
    assert blk == bam.header_block(text, names, [int(c["len"]) for c in contigs])
    n = C.c_int64(0)
    L = capi.lib()
    assert L.bwams_sam_header(ix.h, None, None, None, 0, C.byref(n)) == -4 and n.value == len(sq)


@pytest.mark.parametrize("n_shards", [1, 3])
def test_bgzf_fastq_to_bam_file(tmp_path, toy, deflater, n_shards):
    g, ix, _, names = toy
    reads, _, _ = simulate.make_reads(g, 3000, seed=72)
    rng = np.random.default_rng(9)
    text = _fq(reads, [b"s%d" % i for i in range(len(reads))], rng)
    fq = tmp_path / "r.fq.bgz"
    fq.write_bytes(bgzf.compress(text, 6))
    chunks, info = _chunks(_device_open, str(fq), 150 * 500, False, 2)
    assert info.device_inflate == 1 and len(chunks) >= 4
    hdr_text = ix.sam_header(b"@RG\tID:g\tSM:x", b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n")
    path = str(tmp_path / "out.bam")
    w = capi.writer_open_bam(path, n_shards, 0, ix.bam_header(hdr_text))
    L = capi.lib()
    b = capi.Batch(ix, 1200, 1200 * 160)
    sams, done = [[] for _ in range(n_shards)], 0
    try:
        for i, (t, nr, _) in enumerate(chunks):
            s, _ = b.process_chunk(t, n_processed=done)
            done += nr
            b.bam_run()
            m = b.bam_fetch_bgzf(deflater)
            sams[i % n_shards].append(s)
            capi._chk(L.bwams_writer_put_bgzf(w, i % n_shards, C.c_int64(i // n_shards), m, C.c_int64(len(m))), "bwams_writer_put_bgzf")
        assert L.bwams_writer_put(w, 0, C.c_int64(10 ** 6), b"x\n", C.c_int64(2)) == ERR_ARG     # text in a BAM stream
    finally:
        capi._chk(L.bwams_writer_close(w), "bwams_writer_close")
        b.close()
    files = [path] if n_shards == 1 else [f"{path}.{s}.bam" for s in range(n_shards)]
    for f, want in zip(files, sams):
        data = open(f, "rb").read()
        assert data.endswith(bgzf.EOF_MEMBER)
        bgzf.walk(data)
        raw = gzip.decompress(data)
        h, refs, sam = bam.decode(raw)
        assert h == hdr_text and refs == [(n, int(ln)) for n, ln in zip(names, toy[2]["len"])]
        _same_text(sam, b"".join(want))
        blk, at = ix.bam_header(hdr_text), 0                   # the header is members of its own: the first record starts a member
        for p, _, total, _, isize in bgzf.walk(data):
            at += isize
            if at >= len(blk):
                break
        assert at == len(blk)


def _same_text(a: bytes, b: bytes):
    """SAM texts equal, floats by float32 value"""
    for x, y in zip(a.split(b"\n"), b.split(b"\n")):
        if x != y:
            fx, fy = x.split(b"\t"), y.split(b"\t")
            assert len(fx) == len(fy)
            for u, v in zip(fx, fy):
                assert u == v or (u[2:5] == b":f:" and u[:5] == v[:5] and np.float32(float(u[5:])) == np.float32(float(v[5:])))
    assert a.count(b"\n") == b.count(b"\n")


def test_refusals(toy):
    g, ix, _, names = toy
    L = capi.lib()
    L.bwams_last_error.restype = C.c_char_p
    rng = np.random.default_rng(10)
    reads, _, _ = simulate.make_reads(g, 40, seed=17)
    rn = [b"r%d" % i for i in range(len(reads))]
    b = capi.Batch(ix, 400, 400 * 160)
    try:
        nb = C.c_int64(0)
        assert L.bwams_bam_run(b.h, C.byref(nb), None) == ERR_ARG                          # before any SAM run
        com = [b"1:N:0:ACGT" if i in (23, 31) else b"BC:Z:AC" for i in range(len(reads))]
        b.process_chunk(_fq(reads, rn, rng, com), copy_comment=True)
        assert L.bwams_bam_run(b.h, C.byref(nb), None) == ERR_UNSUPPORTED
        assert b"read 23:" in L.bwams_last_error()
        assert L.bwams_bam_fetch(b.h, None, 0, None) == ERR_ARG                              # nothing kept
        b.process_chunk(_fq(reads, rn, rng, com))                                           # comments not copied: fine
        _check(b, names)
        long_names = [b"n" * 255 if i == 7 else nm for i, nm in enumerate(rn)]
        b.process_chunk(_fq(reads, long_names, rng))
        assert L.bwams_bam_run(b.h, C.byref(nb), None) == ERR_UNSUPPORTED and b"read 7:" in L.bwams_last_error()
        b.process_chunk(b"")                                                               # a chunk of no reads
        assert b.bam_run() == (0, 0)
        rec, off = b.bam_fetch(0)
        assert rec == b"" and list(off) == [0]
    finally:
        b.close()
    # two sequences of one name
    g2, ix2, _, _ = _setup(seed=33)
    try:
        ix2.set_contig_names(["chrA", "chrB", "chrA"])
        b2 = capi.Batch(ix2, 100, 100 * 160)
        b2.process_chunk(_fq(reads[:20], rn[:20], rng))
        assert L.bwams_bam_run(b2.h, C.byref(nb), None) == ERR_ARG
        b2.close()
    finally:
        ix2.close()


def test_scale_past_one_workgroup(toy):
    """50 000 reads: the record scan, the output growth and the per-read offsets over many workgroups"""
    g, ix, _, names = toy
    rng = np.random.default_rng(11)
    reads = simulate.make_read_pairs(g, 25000, seed=18, damaged_frac=0.1)
    rn = [b"big%d" % (i // 2) for i in range(len(reads))]
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    try:
        small, _, _ = simulate.make_reads(g, 100, seed=19)
        b.process_chunk(_fq(small, [b"t%d" % i for i in range(100)], rng))
        _check(b, names)
        b.process_chunk(_fq(reads, rn, rng), paired=True)
        text, rec = _check(b, names)
        assert text.count(b"\n") >= 50000
    finally:
        b.close()
