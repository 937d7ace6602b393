"""Collating a coordinate-sorted BAM by read name on the GPU (csrc/collate.hip, bwams_collate_t): every comparison is byte-exact
against bwams/collate.py (rules C1-C8, include/bwams.h above bwams_collate_open)."""
import ctypes as C

import numpy as np
import pytest

import bam_query_cases as Q
from bam_reads_util import fetched, same_reads
from bwams import bam, capi, collate, simulate
from collate_cases import CASES, REFUSALS, cuts, flag_of, kept, renamed
from dup_join_cases import equivalence_input, key_names, names_of
from test_markdup import P1, P2, R, rec

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_NOMEM, ERR_UNSUPPORTED = -3, -4, -5, -6


def offsets(recs) -> list:
    return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64).tolist()


def same_output(c, pairs, singles):
    """the handle's current output == (pairs as (first, last) tuples, singles as records), bytes and offsets"""
    flat = [r for p in pairs for r in p]
    got_pairs, poff, got_singles, soff = c.fetch()
    assert got_pairs == b"".join(flat) and poff.tolist() == offsets(flat)
    assert got_singles == b"".join(singles) and soff.tolist() == offsets(singles)
    o = c.out()
    assert (o.pairs_bytes, o.n_pairs, o.singles_bytes, o.n_singles) == (len(got_pairs), len(pairs), len(got_singles), len(singles))
    assert bool(o.pairs) == bool(pairs) and bool(o.singles) == bool(singles)


def check(c, adds):
    """adds (lists of records) through add_records / fetch / finish on handle c (reset first): all equal to the restatement;
    -> (the per-add outputs and the orphans as bytes, info())"""
    c.reset()
    w = collate.Collate()
    out = []
    for a in adds:
        pairs, singles = w.add(a)
        assert c.add_records(b"".join(a)) == len(a)
        same_output(c, pairs, singles)
        out.append((collate.pairs_bytes(pairs), b"".join(singles)))
        i = c.info()
        assert (i["records"], i["skipped"], i["pairs"], i["singles"], i["pending"], i["pending_bytes"], i["bytes_pooled"], i["adds"]) == \
            (w.records, w.skipped, w.pairs, w.singles, len(w.pending), w.pending_bytes(), w.bytes_pooled, w.adds)
        assert i["bytes_compacted"] <= i["bytes_pooled"] and i["state"] == 1
    orphans = w.finish()
    assert c.finish() == len(orphans)
    same_output(c, [], orphans)
    i = c.info()
    n_kept = sum(kept(r) for a in adds for r in a)
    assert i["records"] == n_kept + i["skipped"] == sum(len(a) for a in adds) and i["pending"] == 0 and i["pending_bytes"] == 0
    assert 2 * i["pairs"] + i["singles"] + i["orphans"] == n_kept and i["orphans"] == len(orphans) and i["state"] == 2
    return out + [b"".join(orphans)], i


@pytest.fixture(scope="module")
def handle():
    c = capi.Collate()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sorted_recs():
    return equivalence_input()[1]


def _refused(code, text, fn, *args):
    with pytest.raises(capi.BwamsError) as e:
        fn(*args)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_hand_cases(handle):
    same_output(handle, [], [])                              # before any add the output is empty
    for name, adds, want, orphans in CASES:
        got, _ = check(handle, adds)
        assert got == [(collate.pairs_bytes(p), b"".join(s)) for p, s in want] + [b"".join(orphans)], name


def test_refusals_leave_the_handle(handle):
    c = handle
    for name, adds, bad_add, ordinal, reason in REFUSALS:
        c.reset()
        w = collate.Collate()
        for a in adds[:bad_add]:
            c.add_records(b"".join(a))
            w.add(a)
        info, fetch = c.info(), c.fetch()
        _refused(ERR_UNSUPPORTED, "bwams_collate_add_records: record %d: %s" % (ordinal, collate.REASONS[reason]), c.add_records,
                 b"".join(adds[bad_add]))
        assert c.info() == info, name
        for a, b in zip(c.fetch(), fetch):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, name
        ok = adds[bad_add][:ordinal - w.records]                                                # the add up to the record named
        pairs, singles = w.add(ok)
        assert c.add_records(b"".join(ok)) == len(ok)
        same_output(c, pairs, singles)
        orphans = w.finish()
        assert c.finish() == len(orphans)
        same_output(c, [], orphans)
    # a malformed chain, as the other consumers refuse it; C5's states; the options; capacities
    c.reset()
    good = b"".join(CASES[1][1][0])
    _refused(ERR_ARG, "bwams_collate_add_records", c.add_records, good[:-3])
    assert c.info()["adds"] == 0
    c.add_records(good)
    c.finish()
    _refused(ERR_ARG, "bwams_collate_reset starts another round", c.add_records, good)
    _refused(ERR_ARG, "bwams_collate_reset starts another round", c.finish)
    c.reset()
    assert c.info()["state"] == 0 and c.add_records(good) == 6
    L = capi.lib()
    o = c.out()
    buf, off = np.zeros(o.pairs_bytes, np.uint8), np.zeros(2 * o.n_pairs + 1, np.int64)
    assert L.bwams_collate_fetch(c.h, capi._p(buf), o.pairs_bytes - 1, capi._p(off), None, 0, None) == ERR_CAPACITY
    assert L.bwams_collate_fetch(c.h, None, 0, None, capi._p(buf), o.singles_bytes - 1, None) == ERR_CAPACITY
    assert L.bwams_collate_fetch(c.h, None, 0, None, None, 0, None) == 0                        # any pointer NULL
    assert L.bwams_collate_fetch(c.h, capi._p(buf), o.pairs_bytes, None, None, 0, None) == 0 and buf.tobytes() == c.fetch()[0]
    h = C.c_void_p()
    bad = capi.CollateOpt(0, 0, (C.c_uint32 * 2)(0, 1))
    assert L.bwams_collate_open(0, C.byref(bad), C.byref(h)) == ERR_ARG
    assert L.bwams_collate_open(0, C.byref(capi.CollateOpt(-1, 0)), C.byref(h)) == ERR_ARG
    assert L.bwams_collate_close(None) == 0
    with pytest.raises(capi.BwamsError):                                                        # a device that is not there
        capi.Collate(device=1 << 20)
    d = capi.Collate(opt=False)                                                                 # NULL options: the defaults
    try:
        assert check(d, CASES[1][1])[0] == check(c, CASES[1][1])[0]
    finally:
        d.close()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_shapes(handle, sorted_recs, n):
    """a wave of the entry kernel, one lane more or less, a second workgroup, nothing at all; three cuts into adds"""
    recs = sorted_recs[:n]
    one, _ = check(handle, cuts(recs, "one"))
    each, _ = check(handle, cuts(recs, "each"))
    thirds, _ = check(handle, cuts(recs, "thirds"))
    assert one[-1] == each[-1] == thirds[-1]                                                    # the orphans
    for other in (each, thirds):                                                                # the pairs, in completing order
        assert b"".join(p for p, _ in other[:-1]) == one[0][0] and b"".join(s for _, s in other[:-1]) == one[0][1]


def test_collisions(sorted_recs):
    recs = sorted_recs[:257]
    adds = cuts(recs, "thirds")
    want, info = None, {}
    for mask in ((1 << 64) - 1, 0, 0xF):
        c = capi.Collate(key_mask=mask)
        try:
            got, info[mask] = check(c, adds)
            want = want or got
            assert got == want, mask
            if mask == 0:                                    # one run: every entry grouped in the one add
                c.reset()
                c.add_records(b"".join(recs))
                assert c.info()["max_run"] == sum(1 for r in recs if kept(r) and flag_of(r) & 1) > 100
        finally:
            c.close()
    assert info[0]["max_run"] > info[0xF]["max_run"] > info[(1 << 64) - 1]["max_run"] >= 1
    # names of every length, two that differ in the last byte, a name and its prefix: each pairs with itself only
    names = key_names()
    firsts = [renamed(rec(b"x", P1, 100 + 10 * k), nm) for k, nm in enumerate(names)]
    lasts = [renamed(rec(b"x", P2 | R, 400 + 10 * k), nm) for k, nm in enumerate(names)]
    assert names_of(firsts) == names and len(names[0]) == 0 and len(names[7]) == 254
    order = list(range(len(names)))[::-1]
    for mask in ((1 << 64) - 1, 0, 0x3):
        c = capi.Collate(key_mask=mask)
        try:
            got, _ = check(c, [firsts, [lasts[k] for k in order]])
            assert got[1][0] == b"".join(firsts[k] + lasts[k] for k in order) and got[2] == b""
            lone, _ = check(c, [firsts[:-1], lasts[1:]])     # the shortest and the last name stay without a mate
            assert lone[2] == firsts[0] + lasts[-1]
        finally:
            c.close()


def _pool_adds(n_pairs=300, n_adds=10):
    firsts = [rec(b"pool%d" % k, P1, 100 + k, b"%dM" % (40 + k % 50)) for k in range(n_pairs)]
    lasts = [rec(b"pool%d" % k, P2 | R, 5000 + k, b"%dM" % (40 + (7 * k) % 50)) for k in range(n_pairs)]
    per = 2 * n_pairs // n_adds
    both = firsts + lasts
    return [both[k:k + per] for k in range(0, len(both), per)]


def test_pool_rises_falls_and_compacts():
    adds = _pool_adds()
    c = capi.Collate()
    try:
        pending = []
        c.reset()
        w = collate.Collate()
        for a in adds:
            pairs, singles = w.add(a)
            c.add_records(b"".join(a))
            same_output(c, pairs, singles)
            i = c.info()
            pending.append(i["pending"])
            assert i["pending_bytes"] == w.pending_bytes() and i["bytes_compacted"] <= i["bytes_pooled"] == w.bytes_pooled
            assert i["pool_capacity"] >= i["pending_bytes"]
        assert pending == [60, 120, 180, 240, 300, 240, 180, 120, 60, 0]
        assert i["compactions"] >= 1 and 0 < i["bytes_compacted"] <= i["bytes_pooled"]
        assert c.finish() == 0
        # a truncated run: the orphans in ordinal order, across a compaction
        got, i = check(c, adds[:8])
        assert i["compactions"] >= 1 and got[-1] == b"".join(adds[3] + adds[4]) and i["orphans"] == 120
    finally:
        c.close()


def test_pool_cap():
    adds = _pool_adds()
    w = collate.Collate()
    need = []
    for a in adds[:3]:
        w.add(a)
        need.append(w.pending_bytes())
    assert need[0] < need[1] < need[2]
    want = collate.collate(adds[:2])
    c = capi.Collate(pool_bytes=need[2] - 1)
    try:
        for a in adds[:2]:
            c.add_records(b"".join(a))
        info, fetch = c.info(), c.fetch()
        _refused(ERR_NOMEM, "%d bytes" % need[2], c.add_records, b"".join(adds[2]))
        assert c.info() == info and c.fetch()[0] == fetch[0] and c.fetch()[2] == fetch[2]
        assert c.finish() == len(want[1]) == 120
        same_output(c, [], want[1])
    finally:
        c.close()
    c = capi.Collate(pool_bytes=need[2])                     # just enough: dead bytes give way under the cap
    try:
        more = [rec(b"more%d" % k, P1, 9000 + k, b"40M") for k in range(60)]                   # none larger than a record of add 0
        assert sum(len(r) for r in more) <= sum(len(r) for r in adds[0])
        _, i = check(c, adds[:3] + [adds[5], more])          # add 0's mates free its room; the next 60 fit only once that is reclaimed
        assert i["compactions"] == 1 and i["orphans"] == 180
    finally:
        c.close()


def test_file_pieces(tmp_path, sorted_recs):
    records = b"".join(sorted_recs)
    p = tmp_path / "sorted.bam"
    p.write_bytes(Q.bam_file(records, 300))
    f = capi.BamFile(str(p), piece_bytes=65536)
    c = capi.Collate()
    try:
        f.query()
        got, n_piece = [], []
        for piece in f.pieces():
            n_piece.append(c.add_file(piece))
            got.append(c.fetch())
        assert f.info()["pieces"] > 1 and sum(n_piece) == len(sorted_recs)
        bounds = np.concatenate([[0], np.cumsum(n_piece)])
        adds = [sorted_recs[bounds[k]:bounds[k + 1]] for k in range(len(n_piece))]
        w = collate.Collate()
        across = 0
        for a, g, base in zip(adds, got, bounds):
            before = {nm: o for nm, (o, _, _) in w.pending.items()}
            pairs, singles = w.add(a)
            across += sum(before.get(nm, base) < base for nm in names_of([f1 for f1, _ in pairs]))
            flat = [r for pr in pairs for r in pr]
            assert g[0] == b"".join(flat) and g[1].tolist() == offsets(flat) and g[2] == b"".join(singles) and g[3].tolist() == offsets(singles)
        assert across >= 1                                                                      # a pair completed across a piece boundary
        orphans = w.finish()
        assert c.finish() == len(orphans)
        same_output(c, [], orphans)
    finally:
        c.close()
        f.close()


def _fq(reads, names):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (nm, bytes(b"ACGT"[c] for c in r), bytes(33 + (7 * k + 3 * j) % 40 for j in range(len(r))))
                    for k, (nm, r) in enumerate(zip(names, reads)))


def test_round_trip_end_to_end(tmp_path):
    g = simulate.make_genome(6000, seed=3, repeat_frac=0.0)
    ix = capi.Index.build(g, 0)
    contigs = np.zeros(1, capi.CONTIG_DTYPE)
    contigs["offset"], contigs["len"], contigs["is_alt"] = [0], [6000], [0]
    ix.set_contigs(contigs)
    ix.set_contig_names(["big"])
    pr = simulate.make_read_pairs(g, 200, seed=12, read_len=100, damaged_frac=0.0, discordant_frac=0.0)
    text = _fq(pr, [b"p%d" % (k // 2) for k in range(len(pr))])
    b = capi.Batch(ix, len(pr), len(pr) * 160)
    c = capi.Collate()
    f = None
    try:
        b.process_chunk(text, paired=True)
        b.bam_run()
        b.bam_sort()
        records, _ = b.bam_sorted_fetch()
        assert records != b.bam_fetch()[0]                                                      # the sort moved something
        p = tmp_path / "aligned.bam"
        p.write_bytes(Q.bam_file(records, 300))
        f = capi.BamFile(str(p), piece_bytes=65536)                                             # the smallest piece there is
        f.query()
        w = collate.Collate()
        pairs_dev, pairs_host, rest = [], [], []
        want_reads = {x[0] + (b"/1" if k % 2 == 0 else b"/2"): x for k, x in enumerate(fetched(capi.Fastq(text)))}
        got_reads = {}

        def decoded(data: bytes):
            if data:
                for rd, r in zip(fetched(capi.bam_reads_decode(0, data)), bam.split_records(data)):
                    key = rd[0] + (b"/1" if flag_of(r) & 0x40 else b"/2")
                    assert key not in got_reads
                    got_reads[key] = rd

        for piece in f.pieces():
            recs = bam.split_records(piece.fetch()[0])
            wp, ws = w.add(recs)
            assert c.add_file(piece) == len(recs)
            o = c.out()
            host = collate.pairs_bytes(wp)
            if o.n_pairs:                                                                       # (b): from the device pointer
                pairs_dev.append(b.process_chunk_bam((o.pairs, o.pairs_bytes), paired=True)[0])
                pairs_host.append(b.process_chunk_bam(host, paired=True)[0])
            got = c.fetch()
            assert got[0] == host and got[2] == b"".join(ws)
            decoded(got[0]); decoded(got[2])
        assert f.info()["pieces"] > 1 and len(pairs_dev) > 1 and pairs_dev == pairs_host
        c.finish()
        decoded(c.fetch()[2])
        assert c.fetch()[2] == b"".join(w.finish())
        same_reads([got_reads[k] for k in sorted(got_reads)], [want_reads[k] for k in sorted(want_reads)])     # (a): every read once
        assert c.info()["pairs"] > 150
    finally:
        if f is not None:
            f.close()
        c.close()
        b.close()
        ix.close()
