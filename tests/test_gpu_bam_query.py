"""A BAM file read back by region on the GPU (bwams_bam_file_*; include/bwams.h, "BAM file by region"): every comparison is byte
for byte against brute force over the records the file was made from (bwams.bai.overlapping per region).  The files are made in
tmp_path from bwams.bam.encode_record, bwams.bgzf.compress and bwams.bai.build, or by the project's own sorted writer.

The shapes, each the smallest at which its path can go wrong:
  * about 300 records of 40 to 150 bases in BGZF members of 300 bytes: most records straddle members, every chunk starts inside one;
  * the same kind of file at about 400 KB with piece_bytes 65536: several pieces, bytes carried from each to the next;
  * 63, 64, 65 records (one wave of the select kernel, a lane more or less) and 257 (a second workgroup);
  * a record whose aux bytes hold a whole well-formed record, behind a chunk that starts in the middle of a member."""
import ctypes as C
import struct

import numpy as np
import pytest

from bwams import bai, bam, bgzf, capi, simulate
import bam_query_cases as Q
import test_recal_model as M

pytestmark = pytest.mark.gpu

ERR_IO, ERR_ARG, ERR_CAPACITY = -2, -3, -4


def _write(tmp, name, data, index=True):
    p = tmp / name
    p.write_bytes(data)
    if index:
        (tmp / (name + ".bai")).write_bytes(bai.build(data))
    return str(p)


@pytest.fixture(scope="module")
def named(tmp_path_factory):
    records = Q.named_records()
    data = Q.bam_file(records, 300)
    return records, data, _write(tmp_path_factory.mktemp("bamq"), "named.bam", data)


def _read(f, regions):
    """the query fetched piece by piece -> (records, coords, pieces)"""
    f.query(regions)
    recs, coords, pieces = [], [], 0
    for p in f.pieces():
        r, c = p.fetch()
        assert len(r) == p.n_bytes and len(c) == p.n_records
        recs.append(r)
        coords.append(c)
        pieces += 1
    return b"".join(recs), np.concatenate(coords), pieces


def _same_coords(got, recs):
    want = Q.coords_of(recs)
    for k in ("key", "end", "size"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("case", sorted(Q.REGION_LISTS))
def test_records_and_coords(named, case):
    records, _, path = named
    regions = Q.REGION_LISTS[case]
    want = Q.brute(records, regions)
    f = capi.BamFile(path, piece_bytes=65536)                           # bai_path NULL: <path>.bai
    try:
        text, n_ref = f.header()
        assert text == Q.HEADER_TEXT and n_ref == 3 and f.refs().tolist() == Q.LENS
        got, coords, _ = _read(f, regions)
        assert got == b"".join(want)
        _same_coords(coords, want)
        i = f.info()
        assert i["records_kept"] == len(want) and i["records_seen"] >= len(want) and i["pieces"] >= 1
        assert i["intervals"] == len(bai.plan(bai.read(bai.build(named[1])), regions))
        got2, _, _ = _read(f, regions)                                  # a second query on the same handle
        assert got2 == got
    finally:
        f.close()


def test_carry_over_pieces(tmp_path):
    rng = np.random.default_rng(21)
    records = Q.encode(Q.background(rng, 2100, unplaced=9))
    assert 350000 <= len(records) <= 480000
    path = _write(tmp_path, "carry.bam", Q.bam_file(records, 300), index=False)
    f = capi.BamFile(path, piece_bytes=65536)
    try:
        got, coords, pieces = _read(f, ())                             # the whole file: no index needed
        assert got == records                                           # every record once and in order
        recs = bam.split_records(records)
        assert Q.ref_ids(recs)[-9:] == [-1] * 9                         # the unplaced ones last
        _same_coords(coords, recs)
        i = f.info()
        assert i["pieces"] == pieces > 1 and i["carried"] > 0
        assert i["records_seen"] == i["records_kept"] == len(recs) and i["inflated_bytes"] == Q.header_len() + len(records)
        # regions of the same file without an index are refused
        with pytest.raises(capi.BwamsError) as e:
            f.query([(0, 0, 100)])
        assert e.value.code == ERR_ARG and "needs an index" in str(e.value)
    finally:
        f.close()


def _with_aux(rec: bytes, raw: bytes) -> bytes:
    return struct.pack("<I", len(rec) - 4 + len(raw)) + rec[4:] + raw


def test_mid_block_start_and_false_candidates(tmp_path):
    """aux bytes that hold a whole well-formed record: returned as part of their owner only, behind a chunk that starts inside a member"""
    rng = np.random.default_rng(31)
    body = struct.pack("<iiBBHHHiiii", 1, 5000, 2, 0, 0, 0, 0, 1, 0, 0, 0) + b"\x30\0" + b"\x10" + b"\x05" + b"\0" * 4
    decoy = struct.pack("<I", len(body)) + body                         # refID 1, POS 5000: it would overlap the region
    lines = Q.background(rng, 40, refs=(0,)) + [Q.line(b"own%d" % k, 1, 4990 + 3 * k, b"50M", 0, rng) for k in range(6)]
    recs = bam.split_records(Q.encode(lines))
    own = [k for k, r in enumerate(recs) if r[36:39] == b"own"]
    recs[own[1]] = _with_aux(recs[own[1]], b"XBBC" + struct.pack("<I", len(decoy)) + decoy + b"NMC\x09")
    recs[own[3]] = _with_aux(recs[own[3]], b"XZZ" + decoy + b"\0")
    records = b"".join(recs)
    data = Q.bam_file(records, 300)
    path = _write(tmp_path, "decoy.bam", data)
    regions = [(1, 4995, 5010)]
    intervals = bai.plan(bai.read(bai.build(data)), regions)
    assert intervals and intervals[0][0] & 0xFFFF                       # the chain starts inside a member
    want = Q.brute(records, regions)
    assert len(want) == 6
    f = capi.BamFile(path, piece_bytes=65536)
    try:
        got, coords, _ = _read(f, regions)
        assert got == b"".join(want)
        _same_coords(coords, want)
        assert f.info()["candidates"] >= f.info()["records_seen"] + 2   # both decoys pass the filter; the chain skips them
        assert _read(f, ())[0] == records
    finally:
        f.close()


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_grid_edges(tmp_path, n):
    rng = np.random.default_rng(n)
    records = Q.encode(Q.background(rng, n, refs=(1,)))
    path = _write(tmp_path, "edge.bam", Q.bam_file(records, 300))
    f = capi.BamFile(path, piece_bytes=65536)
    try:
        for regions in ([(1, 0, Q.LENS[1])], [(0, 0, 100), (2, 5, 6)], (), Q.random_regions(rng, 3)):     # all, none, the file, some
            want = Q.brute(records, regions) if regions else bam.split_records(records)
            got, coords, _ = _read(f, regions)
            assert got == b"".join(want), regions
            _same_coords(coords, want)
        assert len(Q.brute(records, [(1, 0, Q.LENS[1])])) == n and Q.brute(records, [(0, 0, 100), (2, 5, 6)]) == []
    finally:
        f.close()


def test_round_trip_with_the_sorted_writer(tmp_path):
    rng = np.random.default_rng(41)
    lines = Q.named_lines(rng) + Q.background(rng, 200, unplaced=3, hi1=120000)
    unsorted = b"".join(bam.encode_record(ln, Q.REF_ID, k) for k, ln in enumerate(lines))
    path = str(tmp_path / "sorted.bam")
    ix = capi.Index.build(simulate.make_genome(3000, seed=3, repeat_frac=0.0), 0)
    b = capi.Batch(ix, 1000, 200000)
    try:
        assert b.bam_upload(unsorted) == len(lines)
        b.bam_sort()
        s = capi.Sorter(path, 0, bam.header_block(Q.HEADER_TEXT, Q.NAMES, Q.LENS))
        s.put_batch(0, b)
        s.close()
    finally:
        b.close()
        ix.close()
    records = bam.coord_sort(unsorted)
    f = capi.BamFile(path)                                              # the writer's own <path>.bai, the default piece
    try:
        for case in ("reverse_order", "adjacent_pair", "whole_references", "behind_last_window"):
            regions = Q.REGION_LISTS[case]
            want = Q.brute(records, regions)
            got, coords, _ = _read(f, regions)
            assert got == b"".join(want), case
            _same_coords(coords, want)
        assert _read(f, ())[0] == records
    finally:
        f.close()


CONSUMER_REGIONS = [(0, 99000, 101000), (1, 4000, 6000)]
QUERY = [(1, 0, 60000), (0, 100000, 100200), (0, 0, 50000)]


def _depth():
    return capi.Depth(Q.LENS), lambda h: [h.finish().fetch(t).tolist() for t in (1, 2)] + [h.fetch(0, 0, 310000).tolist()]


def _pileup():
    h = capi.Pileup(Q.LENS, CONSUMER_REGIONS)
    h.set_quality()
    h.set_indels()
    return h, lambda p: [p.fetch(k).tolist() for k in (0, 1)] + [p.fetch_quality(k).tolist() for k in (0, 1)] + \
        [p.fetch_span(k).tolist() for k in (0, 1)] + [p.indel_alleles().tolist()]


def _qc():
    def state(q):
        flags, scalars = q.summary()
        return [flags.tolist(), scalars.tolist()] + [q.table(k).tolist() for k in range(6)]
    return capi.Qc(), state


def _recal():
    h = capi.Recal(Q.LENS, max_cycle=200)
    rng = np.random.default_rng(7)
    for t, n in enumerate(Q.LENS):
        h.set_ref(t, rng.integers(0, 4, n).astype(np.uint8))
    return h, lambda r: [r.table(k).tolist() for k in range(4)]


@pytest.mark.parametrize("make", [_depth, _pileup, _qc, _recal], ids=["depth", "pileup", "qc", "recal"])
def test_consumers_add_file(named, make):
    records, _, path = named
    want_recs = Q.brute(records, QUERY)
    assert len(want_recs) > 100
    f = capi.BamFile(path, piece_bytes=65536)
    h, state = make()
    ref, _ = make()
    try:
        f.query(QUERY)
        n = sum(h.add_file(p) for p in f.pieces())
        assert n == ref.add_records(b"".join(want_recs)) and n > 0
        assert state(h) == state(ref)
    finally:
        f.close()
        h.close()
        ref.close()


def test_recal_apply_file(named):
    records, _, path = named
    want_recs = Q.brute(records, QUERY)
    m = capi.RecalModel(M.zero_tables(0, 200), 200)
    a = capi.RecalApply(m, None, 0)
    m.close()
    f = capi.BamFile(path, piece_bytes=65536)
    try:
        want, n_want = a.records(b"".join(want_recs))
        assert want != b"".join(want_recs) and n_want > 0               # qualities above 60 come down to it
        f.query(QUERY)
        got, n = [], 0
        for p in f.pieces():
            n += a.file(p)
            got.append(p.fetch()[0])                                    # the piece as rewritten where it lies
        assert b"".join(got) == want and n == n_want
    finally:
        f.close()
        a.close()


def _refused(code, part, fn, *args):
    with pytest.raises(capi.BwamsError) as e:
        fn(*args)
    assert e.value.code == code and part in str(e.value), str(e.value)


def test_refusals(named, tmp_path):
    records, data, path = named
    L = capi.lib()
    d = capi.Depth(Q.LENS)
    f = capi.BamFile(path, piece_bytes=65536)
    try:
        # the order of calls
        _refused(ERR_ARG, "bwams_bam_file_next: call bwams_bam_file_query first", f.next)
        _refused(ERR_ARG, "bwams_bam_file_fetch: call bwams_bam_file_query first", f.fetch)
        _refused(ERR_ARG, "bwams_depth_add_file: call bwams_bam_file_query first", d.add_file, f)
        f.query([Q.R_EDGE])
        _refused(ERR_ARG, "bwams_bam_file_fetch: call bwams_bam_file_next first", f.fetch)
        _refused(ERR_ARG, "bwams_depth_add_file: call bwams_bam_file_next first", d.add_file, f)
        while not f.next():
            pass
        assert d.add_file(f) >= 0 and len(f.fetch()[0]) == f.n_bytes     # the last piece stays current
        _refused(ERR_ARG, "bwams_bam_file_next: the query's last piece was consumed", f.next)
        _refused(ERR_ARG, "bwams_bam_file_fetch: the query's last piece was consumed", f.fetch)
        _refused(ERR_ARG, "bwams_depth_add_file: the query's last piece was consumed", d.add_file, f)
        # regions
        for bad in ([(3, 0, 10)], [(-1, 0, 10)], [(0, 10, 10)], [(0, -1, 10)]):
            _refused(ERR_ARG, "bwams_bam_file_query: region 0", f.query, bad)
        # a capacity too small
        f.query([Q.R_EDGE])
        while not f.next():
            pass
        buf = C.create_string_buffer(max(f.n_bytes, 1))
        assert f.n_bytes > 0 and L.bwams_bam_file_fetch(f.h, buf, f.n_bytes - 1, None) == ERR_CAPACITY
        assert L.bwams_depth_add_file(d.h, None, None) == ERR_ARG and L.bwams_depth_add_file(None, f.h, None) == ERR_ARG
    finally:
        f.close()
        d.close()
    _refused(ERR_ARG, "piece_bytes", capi.BamFile, path, None, 0, 4096)
    _refused(ERR_IO, "cannot be opened", capi.BamFile, str(tmp_path / "missing.bam"))
    _refused(ERR_IO, "cannot be read", capi.BamFile, path, str(tmp_path / "missing.bai"))
    # an index of another header
    other = bgzf.compress(bam.header_block(b"", Q.NAMES[:2], Q.LENS[:2]), 1)
    p_other = tmp_path / "other.bai"
    p_other.write_bytes(bai.build(other))
    _refused(ERR_IO, "the index has 2 references, the BAM header 3", capi.BamFile, path, str(p_other))
    # an index cut off
    p_cut = tmp_path / "cut.bai"
    p_cut.write_bytes(bai.build(data)[:-9])
    _refused(ERR_IO, "cut off", capi.BamFile, path, str(p_cut))
    # a chunk end past the end of the file, in a hand-edited index
    raw = bai.build(data)
    chunk = bai.read(raw)["refs"][1]["bins"][bam.reg2bin(5000, 5100)][-1]                   # of the 16 kb bin that holds R_EDGE
    edited = raw.replace(struct.pack("<QQ", *chunk), struct.pack("<QQ", chunk[0], (len(data) + 1000) << 16), 1)
    assert edited != raw
    p_edit = tmp_path / "edited.bai"
    p_edit.write_bytes(edited)
    f = capi.BamFile(path, str(p_edit), piece_bytes=65536)
    try:
        f.query([Q.R_EDGE])

        def drain():
            while not f.next():
                pass
        _refused(ERR_IO, "points past the file", drain)
        _refused(ERR_ARG, "last piece was consumed", f.next)            # the query is over
        assert _read(f, [Q.R_N])[0] == b"".join(Q.brute(records, [Q.R_N]))      # the handle is not
    finally:
        f.close()
    # a flipped byte inside a member: stored blocks, so that only the CRC can notice
    stored = bgzf.compress(bam.header_block(Q.HEADER_TEXT, Q.NAMES, Q.LENS) + records, 0, block=3000)
    members = bgzf.walk(stored)
    p, hdr = members[len(members) // 2][:2]
    broken = bytearray(stored)
    broken[p + hdr + 100] ^= 0x55
    path_b = _write(tmp_path, "flipped.bam", bytes(broken), index=False)
    f = capi.BamFile(path_b, piece_bytes=65536)
    try:
        f.query(())
        with pytest.raises(capi.BwamsError) as e:
            while not f.next():
                pass
        assert e.value.code == ERR_IO and "CRC" in str(e.value) and "file offset" in str(e.value), str(e.value)
    finally:
        f.close()
    # a chain that reaches bytes where no record starts: block_size of a record in the middle set to 20
    recs = bam.split_records(records)
    k = len(recs) // 2
    recs[k] = struct.pack("<I", 20) + recs[k][4:]
    path_c = _write(tmp_path, "chain.bam", Q.bam_file(b"".join(recs), 300), index=False)
    f = capi.BamFile(path_c, piece_bytes=65536)
    try:
        f.query(())
        with pytest.raises(capi.BwamsError) as e:
            while not f.next():
                pass
        assert e.value.code == ERR_IO and "record %d at byte" % k in str(e.value) and "not a well-formed BAM record" in str(e.value)
    finally:
        f.close()
    # a record larger than piece_bytes
    big = Q.encode([Q.line(b"big", 0, 100, b"70000M", 0, np.random.default_rng(1))] + Q.background(np.random.default_rng(2), 20))
    path_d = _write(tmp_path, "big.bam", Q.bam_file(big, 65280), index=False)
    f = capi.BamFile(path_d, piece_bytes=65536)
    try:
        f.query(())
        with pytest.raises(capi.BwamsError) as e:
            while not f.next():
                pass
        size = max(len(r) for r in bam.split_records(big))
        assert e.value.code == ERR_CAPACITY and "of %d bytes does not fit piece_bytes 65536" % size in str(e.value), str(e.value)
    finally:
        f.close()
