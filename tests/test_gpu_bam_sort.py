"""Coordinate-sorted BAM on the GPU (csrc/bam_sort.hip: bwams_bam_upload / _sort / _sorted_fetch) and the sorted BAM writer
(host/bam_sort.cpp: bwams_sorter_*) against Python restatements — bwams/bam.py's coord_sort (samtools sort's default order,
restated: samtools itself is not a dependency of the tests) and bwams/bai.py (the index, byte for byte, and brute-force queries)."""
import ctypes as C
import gzip
import os
import struct
import threading

import numpy as np
import pytest

from bwams import bai, bam, bgzf, capi, simulate
from test_gpu_bam import _fq
from test_gpu_inflate import _chunks, _device_open
from test_host_boundary import _setup

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -3, -4, -6


@pytest.fixture(scope="module")
def toy():
    g, ix, contigs, names = _setup(seed=41)                 # three sequences, the last an ALT one
    yield g, ix, contigs, [n.encode() for n in names]
    ix.close()


def _check_sorted(b):
    """bwams_bam_sorted_fetch == bam.coord_sort(bwams_bam_fetch), coords decoded from the records, the unsorted records kept"""
    rec, _ = b.bam_fetch()
    n = b.bam_sort()
    srt, coords = b.bam_sorted_fetch()
    assert srt == bam.coord_sort(rec)
    recs = bam.split_records(srt)
    assert n == len(recs) == len(coords)
    assert [int(k) for k in coords["key"]] == [bam.coord_key(r) for r in recs]
    assert coords["end"].tolist() == [bam.record_end(r) for r in recs]
    assert coords["size"].tolist() == [len(r) for r in recs]
    assert b.bam_fetch()[0] == rec
    assert b.bam_sort() == n and b.bam_sorted_fetch()[0] == srt          # sorted already: at once, the same
    return rec, srt


def _pairs_with_strays(g, n, seed):
    """simulated pairs, a few with one end of random sequence (an unmapped end placed at its mate) and a few of random sequence only"""
    rng = np.random.default_rng(seed)
    pr = simulate.make_read_pairs(g, n, seed=seed, damaged_frac=0.2, discordant_frac=0.05)
    out = []
    for i in range(n):
        a, b = pr[2 * i], pr[2 * i + 1]
        if i % 11 == 3:
            b = rng.integers(0, 4, len(b)).astype(np.uint8)
        if i % 17 == 5:
            a, b = rng.integers(0, 4, 150).astype(np.uint8), rng.integers(0, 4, 150).astype(np.uint8)
        out += [a, b]
    return out


@pytest.mark.parametrize("paired", [False, True])
def test_batch_sort_equals_restatement(toy, paired):
    g, ix, _, names = toy
    rng = np.random.default_rng(3)
    if paired:
        reads = _pairs_with_strays(g, 800, 12)
        rn = [b"p%d" % (i // 2) for i in range(len(reads))]
    else:
        reads, _, _ = simulate.make_reads(g, 1500, seed=72)
        reads = list(reads) + [rng.integers(0, 4, 150).astype(np.uint8) for _ in range(40)]        # unmapped, unplaced
        rn = [b"s%d" % i for i in range(len(reads))]
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    try:
        b.process_chunk(_fq(reads, rn, rng), paired=paired)
        b.bam_run()
        rec, srt = _check_sorted(b)
        keys = [bam.coord_key(r) for r in bam.split_records(srt)]
        assert keys[-1] >> 32 == 0xFFFFFFFF and len({k >> 32 for k in keys}) == 4          # unplaced records, last
        if paired:
            placed_unmapped = [r for r in bam.split_records(srt) if struct.unpack_from("<H", r, 18)[0] & 4 and bam.coord_key(r) >> 32 != 0xFFFFFFFF]
            assert placed_unmapped
        b.bam_run()                                                            # a new run: unsorted again
        assert capi.lib().bwams_bam_sorted_fetch(b.h, None, 0, None) == ERR_ARG
    finally:
        b.close()


def _line(name, flag, rid, pos0, cigar=b"10M"):
    rname = b"*" if rid < 0 else b"c%d" % rid
    seq = b"ACGTACGTAC" if cigar != b"*" else b"ACG"
    return b"%s\t%d\t%s\t%d\t7\t%s\t*\t0\t0\t%s\t%s" % (name, flag, rname, pos0 + 1, cigar, seq, b"I" * len(seq))


def test_extremes_through_upload(toy):
    g, ix, _, _ = toy
    ref_id = {b"c%d" % i: i for i in range(70000)}
    rng = np.random.default_rng(5)
    lines, far = [], (1 << 31) - 2
    for rid in (-1, 0, 255, 256, 65535, 69999):
        for pos0 in (-1, 0, 1 << 24, far):
            for flag in (0, 16, 4, 4 | 16):
                cig = b"*" if flag & 4 or rid < 0 else b"10M"
                lines.append((_line(b"x%d_%d_%d" % (rid, pos0, flag), flag, rid, 0 if pos0 == far else pos0, cig), pos0 == far))
    lines += [(_line(b"same%03d" % i, 16, 256, 1000, b"4M2D6M"), False) for i in range(300)]      # identical keys: stability
    lines += [(_line(b"n%d" % i, 0, 300, 5, b"3S2M4N5M"), False) for i in range(5)]

    def enc(ln, at_far):                                     # POS 2^31 - 2 has no bin that fits 16 bits: patched in after encoding
        r = bam.encode_record(ln, ref_id)
        return r[:8] + struct.pack("<i", far) + r[12:] if at_far else r
    order = rng.permutation(len(lines))
    recs = b"".join(enc(*lines[i]) for i in order)
    lines = [ln for ln, _ in lines]
    b = capi.Batch(ix, 1000, 1000 * 160)
    try:
        assert b.bam_upload(recs) == len(lines)
        got, off = b.bam_fetch()
        assert got == recs and off[-1] == len(recs) and len(off) == len(lines) + 1
        _, srt = _check_sorted(b)
        names = [r[36:36 + r[12] - 1] for r in bam.split_records(srt)]
        same = [n for n in names if n.startswith(b"same")]
        assert same == [lines[i].split(b"\t")[0] for i in order if lines[i].startswith(b"same")]
        for n in (0, 1):
            assert b.bam_upload(recs[:len(bam.split_records(recs)[0])] if n else b"") == n
            _check_sorted(b)
        big = [_line(b"b%06d" % i, 16 * (i % 2), int(rng.integers(-1, 400)), int(rng.integers(-1, 1 << 20))) for i in range(200000)]
        brecs = b"".join(bam.encode_record(ln, ref_id) for ln in big)
        b2 = capi.Batch(ix, 1000, 1000 * 160)                                 # a fresh batch that has run nothing
        try:
            assert b2.bam_upload(brecs) == 200000
            _check_sorted(b2)
        finally:
            b2.close()
    finally:
        b.close()


def test_more_than_256_references(toy):
    g, _, _, _ = toy
    ix = capi.Index.build(g, 0)
    try:
        n = 300
        contigs = np.zeros(n, capi.CONTIG_DTYPE)
        contigs["offset"] = np.arange(n) * (len(g) // n)
        contigs["len"] = len(g) // n
        ix.set_contigs(contigs)
        ix.set_contig_names(["seq%03d" % i for i in range(n)])
        reads, _, _ = simulate.make_reads(g, 2000, seed=9)
        rng = np.random.default_rng(7)
        b = capi.Batch(ix, len(reads), len(reads) * 160)
        try:
            b.process_chunk(_fq(reads, [b"m%d" % i for i in range(len(reads))], rng))
            b.bam_run()
            _, srt = _check_sorted(b)
            assert max(bam.coord_key(r) >> 32 for r in bam.split_records(srt) if bam.coord_key(r) >> 32 != 0xFFFFFFFF) > 256
        finally:
            b.close()
    finally:
        ix.close()


def test_refusals(toy):
    g, ix, _, _ = toy
    L = capi.lib()
    b = capi.Batch(ix, 100, 100 * 160)
    try:
        n = C.c_int64(0)
        assert L.bwams_bam_sort(b.h, C.byref(n)) == ERR_ARG                   # before any run
        ref_id = {b"c0": 0}
        recs = b"".join(bam.encode_record(_line(b"r%d" % i, 0, 0, 100 - i), ref_id) for i in range(5))
        assert L.bwams_bam_upload(b.h, recs[:-1], len(recs) - 1, C.byref(n)) == ERR_ARG          # truncated chain
        short = struct.pack("<I", 20) + recs[4:24]
        assert L.bwams_bam_upload(b.h, short, len(short), C.byref(n)) == ERR_ARG                  # block_size < 32
        b.bam_upload(recs)
        assert L.bwams_bam_sorted_fetch(b.h, None, 0, None) == ERR_ARG                            # not sorted yet
        b.bam_sort()
        buf = C.create_string_buffer(len(recs))
        assert L.bwams_bam_sorted_fetch(b.h, buf, len(recs) - 1, None) == ERR_CAPACITY
        assert L.bwams_bam_sorted_fetch(b.h, buf, len(recs), None) == 0 and buf.raw == bam.coord_sort(recs)
    finally:
        b.close()


def _run_sorter(tmp_path, tag, ix, chunks, hdr, mem_bytes):
    """chunks through process_chunk -> bam_run -> bam_sort -> put_batch / put, in shuffled seq order, puts from two threads"""
    path = str(tmp_path / ("%s.bam" % tag))
    s = capi.Sorter(path, 0, hdr, tmp_prefix=str(tmp_path / ("%s_tmp" % tag)), mem_bytes=mem_bytes)
    b = capi.Batch(ix, 1200, 1200 * 160)
    base = np.concatenate([[0], np.cumsum([nr for _, nr, _ in chunks])])
    order = np.random.default_rng(len(tag)).permutation(len(chunks))
    recs, later, errs = {}, [], []
    try:
        for i in order:
            t, nr, _ = chunks[i]
            b.process_chunk(t, paired=True, n_processed=int(base[i]))
            b.bam_run()
            recs[int(i)] = b.bam_fetch()[0]
            b.bam_sort()
            if i % 2:
                s.put_batch(int(i), b)
            else:
                later.append((int(i),) + b.bam_sorted_fetch())

        def put(items):
            try:
                for seq, r, c in items:
                    s.put(seq, r, c)
            except Exception as e:                                             # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=put, args=(later[k::2],)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
    finally:
        b.close()
        st = s.close()
    assert st.runs == len(chunks) and st.records == sum(len(bam.split_records(r)) for r in recs.values())
    return path, st, b"".join(recs[i] for i in range(len(chunks)))


def test_sorter_end_to_end_and_index(tmp_path, toy):
    g, ix, contigs, names = toy
    reads = _pairs_with_strays(g, 2400, 21)
    rng = np.random.default_rng(9)
    fq = tmp_path / "r.fq.bgz"
    fq.write_bytes(bgzf.compress(_fq(reads, [b"q%d" % (i // 2) for i in range(len(reads))], rng), 6))
    chunks, info = _chunks(_device_open, str(fq), 150 * 1000, True, 2)
    assert info.device_inflate == 1 and len(chunks) >= 4
    text = ix.sam_header(b"@RG\tID:g\tSM:x", b"@PG\tID:bwa-mem2\tPN:bwa-mem2\n")
    lens = [int(x) for x in contigs["len"]]
    hdr = bam.header_block(text, names + [b"chrEmpty"], lens + [5000])       # a reference with no records
    p1, st1, unsorted = _run_sorter(tmp_path, "mem", ix, chunks, hdr, 1 << 40)
    p2, st2, unsorted2 = _run_sorter(tmp_path, "spill", ix, chunks, hdr, 1)
    assert unsorted == unsorted2
    assert st1.spilled_runs == 0 and st2.spilled_runs == len(chunks) and st2.spilled_bytes > len(unsorted)
    assert sorted(os.listdir(tmp_path)) == sorted(["r.fq.bgz", "mem.bam", "mem.bam.bai", "spill.bam", "spill.bam.bai"])   # no temporary files
    d1, d2 = open(p1, "rb").read(), open(p2, "rb").read()
    x1, x2 = open(p1 + ".bai", "rb").read(), open(p2 + ".bai", "rb").read()
    assert d1 == d2 and x1 == x2 and st1.out_bytes == len(d1)
    walk = bgzf.walk(d1)
    assert d1.endswith(bgzf.EOF_MEMBER)
    at = 0
    for _, _, _, _, isize in walk:                                             # the header in members of its own
        at += isize
        if at >= len(hdr):
            break
    assert at == len(hdr)
    srt = bam.coord_sort(unsorted)
    assert gzip.decompress(d1) == hdr + srt
    # the index
    assert bai.build(d1) == x1
    idx = bai.read(x1)
    recs = bam.split_records(srt)
    for t in range(len(names) + 1):
        mine = [r for r in recs if struct.unpack_from("<i", r, 4)[0] == t]
        if not mine:
            assert idx["refs"][t]["bins"] == {} and idx["refs"][t]["lin"] == []
            continue
        unm = sum(struct.unpack_from("<H", r, 18)[0] & 4 != 0 for r in mine)
        assert idx["refs"][t]["bins"][bai.PSEUDO_BIN][1] == (len(mine) - unm, unm)
    assert idx["n_no_coor"] == sum(struct.unpack_from("<i", r, 4)[0] < 0 for r in recs) > 0
    assert any(struct.unpack_from("<H", r, 18)[0] & 4 for r in recs if struct.unpack_from("<i", r, 4)[0] >= 0)
    regions = []
    for t, ln in enumerate(lens + [5000]):
        regions.append((t, 0, ln))
        regions += [(t, (w << 14) - 5, (w << 14) + 5) for w in range(1, ln >> 14)]
    for _ in range(300):
        t = int(rng.integers(0, len(lens) + 1))
        a = int(rng.integers(0, (lens + [5000])[t]))
        regions.append((t, a, a + int(rng.choice([1, 100, 1000, 20000]))))
    for t, a, e in regions:
        assert bai.query(idx, d1, t, a, e) == bai.overlapping(srt, t, a, e), (t, a, e)


def test_sorter_refusals(tmp_path):
    names, lens = [b"a", b"b"], [1000, 2000]
    hdr = bam.header_block(b"", names, lens)
    ref_id = {b"c0": 0, b"c1": 1, b"c2": 2}
    recs = [bam.encode_record(_line(b"r%d" % i, 0, i % 3, 10 * i), ref_id) for i in range(6)]

    def run(rs):
        data = b"".join(rs)
        cd = np.array([(bam.coord_key(r), bam.record_end(r), len(r)) for r in rs], capi.BAM_COORD_DTYPE)
        return data, cd

    s = capi.Sorter(str(tmp_path / "x.bam"), 0, hdr, mem_bytes=1 << 30)
    ok = [r for r in recs if struct.unpack_from("<i", r, 4)[0] < 2]
    ok = bam.split_records(bam.coord_sort(b"".join(ok)))
    s.put(0, *run(ok))
    with pytest.raises(capi.BwamsError) as e:
        s.put(1, *run(ok[::-1]))                                               # keys out of order
    assert e.value.code == ERR_ARG
    with pytest.raises(capi.BwamsError) as e:
        s.put(0, *run(ok))                                                     # seq put before
    assert e.value.code == ERR_ARG
    with pytest.raises(capi.BwamsError) as e:
        s.put(2, *run([r for r in recs if struct.unpack_from("<i", r, 4)[0] == 2]))   # refID outside the header
    assert e.value.code == ERR_ARG
    data, cd = run(ok)
    cd["size"][0] += 1
    with pytest.raises(capi.BwamsError) as e:
        s.put(3, data, cd)                                                     # sizes that do not chain the records
    assert e.value.code == ERR_ARG
    s.close()
    assert gzip.decompress(open(tmp_path / "x.bam", "rb").read()) == hdr + b"".join(ok)
    with pytest.raises(capi.BwamsError) as e:
        capi.Sorter(str(tmp_path / "y.bam"), 0, bam.header_block(b"", [b"huge"], [(1 << 29) + 1]))
    assert e.value.code == ERR_UNSUPPORTED and not os.path.exists(tmp_path / "y.bam")
    capi.Sorter(str(tmp_path / "z.bam"), 0, bam.header_block(b"", [b"huge"], [(1 << 29) + 1]), bai=False).close()
