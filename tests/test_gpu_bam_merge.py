"""Several coordinate-sorted BAM files merged as one record stream on the GPU (bwams_bam_file_open_merge; include/bwams.h, rules M1
to M9): every comparison is byte for byte against bwams/merge.py (merge_records, merge_header, rounds) over the records the files
were made from.  The files are made in tmp_path from bam_query_cases (300-byte BGZF members).

The shapes, each the smallest at which its path can go wrong:
  * K = 1 and K = 3 at about 400 KB a file with child_bytes 65536: many rounds, every child refilled several times, carries in the children;
  * a run of 400 records of one key (over 100 KB, so it crosses a 64 KiB piece) in one file or in all three; 600 unplaced records at
    the end of two files;
  * 63, 64, 65 and 257 records (a wave of the rank kernel, a lane more or less, a second workgroup) merged pairwise;
  * K = 64 (every lane of the frontier kernel's wave), header-only files, regions, unsorted input inside a piece and across two."""
import numpy as np
import pytest

from bwams import bai, bam, bgzf, capi, markdup, merge
import bam_query_cases as Q
from dup_join_cases import equivalence_input

pytestmark = pytest.mark.gpu

ERR_IO, ERR_ARG, ERR_UNSUPPORTED = -2, -3, -6
CHILD = 65536


def _write(tmp, name, records, index=True, block=300):
    data = Q.bam_file(records, block)
    p = tmp / name
    p.write_bytes(data)
    if index:
        (tmp / (name + ".bai")).write_bytes(bai.build(data))
    return str(p)


def _pieces(f, regions=()):
    """the query fetched piece by piece -> [(records, coords), ...]"""
    f.query(regions)
    out = []
    for p in f.pieces():
        r, c = p.fetch()
        assert len(r) == p.n_bytes and len(c) == p.n_records
        out.append((r, c))
    return out


def _flat(pieces):
    return b"".join(r for r, _ in pieces), np.concatenate([c for _, c in pieces])


def _same_coords(got, recs):
    want = Q.coords_of(recs)
    for k in ("key", "end", "size"):
        assert np.array_equal(got[k], want[k]), k


def _merged(files):
    """rule M4 over the files' record bytes -> the merged records as a list"""
    return merge.merge_records([bam.split_records(f) for f in files])


def _check(paths, files, **kw):
    """the whole-file query of the merged handle equals the Python merge; -> (pieces, merge_info)"""
    want = _merged(files)
    f = capi.BamFile.merge(paths, child_bytes=CHILD, **kw)
    try:
        pieces = _pieces(f)
        got, coords = _flat(pieces)
        assert got == b"".join(want)
        _same_coords(coords, want)
        return pieces, f.merge_info()
    finally:
        f.close()


def _refused(code, parts, fn, *args, **kw):
    with pytest.raises(capi.BwamsError) as e:
        fn(*args, **kw)
    assert e.value.code == code and all(p in str(e.value) for p in parts), str(e.value)


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """three files of about 2100 records and 400 KB each, 9 unplaced reads at each file's end, indexed"""
    tmp = tmp_path_factory.mktemp("merge3")
    files = [Q.encode(Q.background(np.random.default_rng(100 + k), 2100, tag=b"f%d_" % k, unplaced=9)) for k in range(3)]
    assert all(350000 <= len(f) <= 480000 for f in files) and Q.unique_names(b"".join(files))
    return files, [_write(tmp, "lane%d.bam" % k, f) for k, f in enumerate(files)]


def test_one_file_equals_the_plain_handle(tmp_path):
    records = Q.encode(Q.background(np.random.default_rng(21), 2100, unplaced=9))
    path = _write(tmp_path, "one.bam", records, index=False)
    plain = capi.BamFile(path, piece_bytes=CHILD)
    try:
        want, wcoords = plain.read()
    finally:
        plain.close()
    pieces, info = _check([path], [records])
    got, coords = _flat(pieces)
    assert got == want == records and np.array_equal(coords, wcoords)
    assert info["n_files"] == 1 and info["child_bytes"] == CHILD and info["rounds"] == len(pieces) > 1


def test_three_files(three):
    files, paths = three
    f = capi.BamFile.merge(paths, child_bytes=CHILD)
    try:
        pieces = _pieces(f)
        got, coords = _flat(pieces)
        want = _merged(files)
        assert got == b"".join(want)
        _same_coords(coords, want)
        i = f.merge_info()
        assert i["rounds"] == len(pieces) > 3 and i["refills"] > 3 and i["records"] == len(want) and i["bytes"] == len(got)
        assert i["max_piece_records"] == max(len(c) for _, c in pieces) and i["max_window_left"] > 0
        assert f.info()["carried"] > 0 and f.info()["records_kept"] == len(want)
        again = _pieces(f)                                              # rule M8: the same pieces on a second query
        assert [r for r, _ in again] == [r for r, _ in pieces]
        # and they are rule M7's rounds over the pieces that plain handles of the same piece size give
        kid_pieces = []
        for p in paths:
            k = capi.BamFile(p, piece_bytes=CHILD)
            try:
                kid_pieces.append([bam.split_records(r) for r, _ in _pieces(k)])
            finally:
                k.close()
        assert [b"".join(p) for p in merge.rounds(kid_pieces)] == [r for r, _ in pieces]
        text, n_ref = f.header()
        assert text == Q.HEADER_TEXT and n_ref == 3 and f.refs().tolist() == Q.LENS
    finally:
        f.close()


@pytest.mark.parametrize("where", ["all", "first", "last"])
def test_ties_across_a_piece_boundary(tmp_path, where):
    files = []
    for k in range(3):
        rng = np.random.default_rng(200 + k)
        lines = Q.background(rng, 300, tag=b"f%d_" % k)
        if where == "all" or (where == "first" and k == 0) or (where == "last" and k == 2):
            lines += [Q.line(b"f%dtie%d" % (k, i), 0, 150000, b"150M", 0, rng) for i in range(400)]
            assert sum(len(bam.encode_record(ln, Q.REF_ID, 0)) for ln in lines[-400:]) > 100000
        files.append(Q.encode(lines))
    assert Q.unique_names(b"".join(files))
    pieces, info = _check([_write(tmp_path, "t%d.bam" % k, f, index=False) for k, f in enumerate(files)], files)
    assert info["rounds"] >= 3 and info["refills"] >= 5             # the file with the run alone gives three pieces


def test_unplaced_tails(tmp_path):
    files = [Q.encode(Q.background(np.random.default_rng(300 + k), 200, tag=b"f%d_" % k, unplaced=600)) for k in range(2)]
    pieces, _ = _check([_write(tmp_path, "u%d.bam" % k, f, index=False) for k, f in enumerate(files)], files)
    tail = bam.split_records(_flat(pieces)[0])[-1200:]
    want = [b"f%d_u%d\0" % (k, i) for k in range(2) for i in range(600)]       # all of file 0's, then all of file 1's, in file order
    assert [r[36:36 + r[12]] for r in tail] == want and Q.ref_ids(tail) == [-1] * 1200


@pytest.mark.parametrize("a,b", [(63, 64), (63, 65), (63, 257), (64, 65), (64, 257), (65, 257)])
def test_wave_edges(tmp_path, a, b):
    files = [Q.encode(Q.background(np.random.default_rng(n), n, tag=b"n%d_" % n, refs=(1,))) for n in (a, b)]
    _check([_write(tmp_path, "w%d.bam" % k, f, index=False) for k, f in enumerate(files)], files)


def test_64_files_and_their_neighbours(tmp_path):
    files = [Q.encode(Q.background(np.random.default_rng(400 + k), 5, tag=b"k%d_" % k, unplaced=k % 2)) for k in range(64)]
    paths = [_write(tmp_path, "k%d.bam" % k, f, index=False) for k, f in enumerate(files)]
    _, info = _check(paths, files)
    assert info["n_files"] == 64 and info["refills"] == 64
    _refused(ERR_ARG, ["n_files in [1, 64]"], capi.BamFile.merge, paths + paths[:1], child_bytes=CHILD)
    _refused(ERR_ARG, ["n_files in [1, 64]"], capi.BamFile.merge, [], child_bytes=CHILD)
    # a header-only file among three; three header-only files: one empty last piece
    empty = _write(tmp_path, "empty.bam", b"", index=False)
    _check([paths[0], empty, paths[1]], [files[0], b"", files[1]])
    f = capi.BamFile.merge([empty] * 3, child_bytes=CHILD)
    try:
        f.query()
        assert f.next() is True and (f.n_records, f.n_bytes) == (0, 0) and f.fetch()[0] == b""
        assert f.merge_info()["rounds"] == 1
        _refused(ERR_ARG, ["the query's last piece was consumed"], f.next)
    finally:
        f.close()


def test_inputs(three, tmp_path):
    files, paths = three
    # rule M1: child_bytes from piece_bytes, and the refusals
    assert merge.child_bytes_of(0, 4) == 32 << 20 and merge.child_bytes_of(3 * 65536 - 1, 3) == 0 and merge.child_bytes_of(1, 3, 70000) == 70000
    f = capi.BamFile.merge(paths, piece_bytes=3 * 65536 + 65535)
    try:
        assert f.merge_info()["child_bytes"] == merge.child_bytes_of(3 * 65536 + 65535, 3) == 65536
        _refused(ERR_ARG, ["bwams_bam_file_next: call bwams_bam_file_query first"], f.next)
        _refused(ERR_ARG, ["bwams_bam_file_fetch: call bwams_bam_file_query first"], f.fetch)
        f.query()
        _refused(ERR_ARG, ["bwams_bam_file_fetch: call bwams_bam_file_next first"], f.fetch)
    finally:
        f.close()
    _refused(ERR_ARG, ["below 65536", "piece_bytes of at least %d" % (3 * 65536)], capi.BamFile.merge, paths, piece_bytes=3 * 65536 - 1)
    _refused(ERR_ARG, ["below 65536"], capi.BamFile.merge, paths, child_bytes=4096)
    _refused(ERR_ARG, ["reserved"], capi.BamFile.merge, paths, child_bytes=CHILD, reserved=1)
    missing = str(tmp_path / "missing.bam")
    _refused(ERR_IO, ["file 1 (%s): " % missing, "cannot be opened"], capi.BamFile.merge, [paths[0], missing], child_bytes=CHILD)
    plain = capi.BamFile(paths[0], piece_bytes=CHILD)
    try:
        _refused(ERR_ARG, ["plain"], plain.merge_info)
    finally:
        plain.close()


@pytest.mark.parametrize("case", ["reverse_order", "whole_references"])
def test_regions(tmp_path, case):
    files = []
    for k in range(3):
        rng = np.random.default_rng(500 + k)
        lines = [ln.replace(ln.split(b"\t")[0], b"f%d_" % k + ln.split(b"\t")[0], 1) for ln in Q.named_lines(rng)]
        files.append(Q.encode(lines + Q.background(rng, 293, tag=b"f%d_" % k, unplaced=4, hi1=120000)))
    paths = [_write(tmp_path, "r%d.bam" % k, f) for k, f in enumerate(files)]
    regions = Q.REGION_LISTS[case]
    want = Q.brute(b"".join(_merged(files)), regions)
    assert len(want) > 3
    f = capi.BamFile.merge(paths, child_bytes=CHILD)
    try:
        got, coords = _flat(_pieces(f, regions))
        assert got == b"".join(want)
        _same_coords(coords, want)
        assert f.info()["records_kept"] == len(want) and f.info()["intervals"] >= 3
    finally:
        f.close()


def test_region_query_needs_every_index(three, tmp_path):
    files, paths = three
    bare = _write(tmp_path, "bare.bam", files[1], index=False)
    f = capi.BamFile.merge([paths[0], bare, paths[2]], child_bytes=CHILD)
    try:
        _refused(ERR_ARG, ["file 1 (%s)" % bare, "index"], f.query, [Q.R_EDGE])
        assert _flat(_pieces(f))[0] == b"".join(_merged(files))          # the whole file needs none
    finally:
        f.close()


def _piece_counts(path):
    k = capi.BamFile(path, piece_bytes=CHILD)
    try:
        return [len(c) for _, c in _pieces(k)]
    finally:
        k.close()


def _drain(f):
    f.query()
    while not f.next():
        pass


def _unsorted(three, tmp_path, at):
    """file 1 with records at and at + 1 exchanged -> its path, or None when their keys are equal"""
    recs = bam.split_records(three[0][1])
    if bam.coord_key(recs[at]) == bam.coord_key(recs[at + 1]):
        return None
    recs[at], recs[at + 1] = recs[at + 1], recs[at]
    return _write(tmp_path, "unsorted%d.bam" % at, b"".join(recs), index=False)


def _check_unsorted(three, path, at):
    f = capi.BamFile.merge([three[1][0], path, three[1][2]], child_bytes=CHILD)
    try:
        _refused(ERR_IO, ["file 1 (%s): record %d: key below its predecessor's" % (path, at + 1)], _drain, f)
        _refused(ERR_ARG, ["last piece was consumed"], f.next)          # the query is over
    finally:
        f.close()


def test_unsorted_inside_a_piece(three, tmp_path):
    recs = bam.split_records(three[0][1])
    counts = _piece_counts(three[1][1])
    at = counts[0] + counts[1] // 2                                     # in the middle of the second piece
    assert sum(len(r) for r in recs[:at]) > 65536
    while (path := _unsorted(three, tmp_path, at)) is None:
        at += 1
    assert _piece_counts(path) == counts
    _check_unsorted(three, path, at)


def test_unsorted_across_a_piece_boundary(three, tmp_path):
    counts = _piece_counts(three[1][1])
    assert len(counts) > 3
    for n_pieces in range(1, len(counts)):                              # the first boundary that the exchange itself does not move
        at = sum(counts[:n_pieces]) - 1
        path = _unsorted(three, tmp_path, at)
        if path is not None and _piece_counts(path) == counts:
            break
    else:
        pytest.fail("no piece boundary of file 1 is fit for the exchange")
    _check_unsorted(three, path, at)


def test_headers(three, tmp_path):
    files, paths = three
    # a length that differs in reference 1 of file 2
    data = bam.header_block(Q.HEADER_TEXT, Q.NAMES, [Q.LENS[0], Q.LENS[1] + 1, Q.LENS[2]]) + files[2]
    other = tmp_path / "other.bam"
    other.write_bytes(bgzf.compress(data, 1, block=300))
    _refused(ERR_UNSUPPORTED, ["file 2", "reference 1", "length"], capi.BamFile.merge, [paths[0], paths[1], str(other)], child_bytes=CHILD)
    # the merged header: read groups united, a @PG collision dropped
    texts = [Q.HEADER_TEXT + b"@RG\tID:l%d\tLB:lib\n@PG\tID:bwa\tCL:lane%d\n" % (k, k) for k in range(3)]
    blocks = [bam.header_block(t, Q.NAMES, Q.LENS) for t in texts]
    ps = []
    for k, b in enumerate(blocks):
        p = tmp_path / ("h%d.bam" % k)
        p.write_bytes(bgzf.compress(b, 1, block=300))                   # header-only files
        ps.append(str(p))
    want, dropped = merge.merge_header(blocks)
    assert dropped == 2 and want.count(b"@RG") == 3
    f = capi.BamFile.merge(ps, child_bytes=CHILD)
    try:
        assert f.header_block() == want and f.merge_info()["pg_dropped"] == 2
        assert f.header()[0] == want[8:8 + int.from_bytes(want[4:8], "little")]
    finally:
        f.close()


def test_depth_through_the_merged_handle(three):
    files, paths = three
    want = b"".join(_merged(files))
    f = capi.BamFile.merge(paths, child_bytes=CHILD)
    d, ref = capi.Depth(Q.LENS), capi.Depth(Q.LENS)
    try:
        f.query()
        n = sum(d.add_file(p) for p in f.pieces())
        assert n == ref.add_records(want) and n > 0
        d.finish()
        ref.finish()
        assert np.array_equal(d.summary(), ref.summary())
        for t, end in ((0, 310000), (1, Q.LENS[1])):
            assert np.array_equal(d.fetch(t, 0, end), ref.fetch(t, 0, end))
    finally:
        f.close()
        d.close()
        ref.close()


def test_dupjoin_over_two_lanes(tmp_path):
    """a site's template in lane 0, its planted copies in lane 1: duplicates of each other only across the files"""
    _, recs = equivalence_input(seed=7, n_sites=400)
    lanes = [[r for r in recs if r[36:36 + r[12] - 1].endswith(b"_0")], [r for r in recs if not r[36:36 + r[12] - 1].endswith(b"_0")]]
    assert all(lanes)
    alone = [markdup.mark_joined([b"".join(lane)])[1]["records_marked"] for lane in lanes]
    merged = merge.merge_records(lanes)
    (want,), counts, _ = markdup.mark_joined([b"".join(merged)])
    assert counts["records_marked"] > sum(alone) and alone[0] == 0     # templates marked only because of the other file
    paths = [_write(tmp_path, "lane%d.bam" % k, b"".join(lane), index=False) for k, lane in enumerate(lanes)]
    f = capi.BamFile.merge(paths, child_bytes=CHILD)
    j = capi.DupJoin()
    try:
        f.query()
        assert sum(j.add_file(p) for p in f.pieces()) == len(merged)
        st, _ = j.finish()
        assert st.counts() == {k: counts[k] for k in st.counts()}
        f.query()
        got, marked = [], 0
        for p in f.pieces():
            marked += j.apply_file(p)
            got.append(p.fetch()[0])
        assert b"".join(got) == want and marked == counts["records_marked"]
    finally:
        j.close()
        f.close()


def test_sorter_output_equals_the_runs_route(three, tmp_path):
    """the merged pieces as runs of a Sorter against each whole file as run seq = k: the same BAM and the same BAI"""
    files, paths = three
    f = capi.BamFile.merge(paths, child_bytes=CHILD)
    try:
        s = capi.Sorter(str(tmp_path / "a.bam"), 0, f.header_block(), bai=True)
        f.query()
        for k, p in enumerate(f.pieces()):
            s.put(k, *p.fetch())
        s.close()
    finally:
        f.close()
    s = capi.Sorter(str(tmp_path / "b.bam"), 0, bam.header_block(Q.HEADER_TEXT, Q.NAMES, Q.LENS), bai=True)
    for k, p in enumerate(paths):
        plain = capi.BamFile(p)
        try:
            s.put(k, *plain.read())
        finally:
            plain.close()
    s.close()
    assert (tmp_path / "a.bam").read_bytes() == (tmp_path / "b.bam").read_bytes()
    assert (tmp_path / "a.bam.bai").read_bytes() == (tmp_path / "b.bam.bai").read_bytes()
