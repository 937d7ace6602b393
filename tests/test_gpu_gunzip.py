"""Plain gzip inflated on the GPU (csrc/gunzip.hip: bwams_gunzip_*, bwams_reader_open_device2) against zlib / gzip byte for byte, with
the output on the host and on the device: pieces that each hold a block start and pieces that merge, every block kind and gzip shape,
histories that are mostly markers, false candidates, streaming in calls of any size, capacity, damage and refusals, the reader chunk
for chunk against bwams_reader_open, FASTQ.gz to SAM, and 63 MB in several calls.  bwams/gunzip.py (the restatement, checked against
zlib in tests/test_gunzip.py) proves that each input has the shape its test claims."""
import ctypes as C
import gzip
import hashlib
import re
import zlib

import numpy as np
import pytest
import torch

from bwams import bgzf, capi, simulate
from bwams import gunzip as G
from gunzip_util import fastq_text, marker_text, member, raw_deflate

pytestmark = pytest.mark.gpu

ERR_IO, ERR_CAPACITY, ERR_UNSUPPORTED = -2, -4, -6
TEXT = fastq_text(3000, 1)


def check(gz, want, piece_bytes=32768, max_in=4 << 20, max_out=16 << 20):
    """gz inflated in one call, to the host and to the device (guard bytes around it): the stats of the host run"""
    g = capi.Gunzipper(0, max_in, max_out, piece_bytes)
    got, used, st = g.run(gz, True)
    g.close()
    assert got == want and used == len(gz) and st.out_bytes == len(want) and st.in_bytes == len(gz)
    g = capi.Gunzipper(0, max_in, max_out, piece_bytes)
    dev = torch.full((len(want) + 128,), 0x5A, dtype=torch.uint8, device="cuda:0")
    rc, used, n, _ = g.run_raw(gz, True, dev.data_ptr() + 61, len(want), True)          # an odd address: head and tail bytes
    g.close()
    assert (rc, used, n) == (0, len(gz), len(want)), capi.lib().bwams_last_error()
    host = dev.cpu().numpy().tobytes()
    assert host[61:61 + len(want)] == want and host[:61] == b"\x5a" * 61 and host[61 + len(want):] == b"\x5a" * 67
    return st


@pytest.fixture(scope="module")
def levels():
    """level -> (gzip file of TEXT, its blocks by the restatement)"""
    out = {}
    for level in (1, 6, 9):
        gz = member(TEXT, level)
        out[level] = (gz, G.walk_gzip(gz)[0])
    return out


@pytest.mark.parametrize("level", [1, 6, 9])
def test_pieces_that_each_hold_a_block_start(levels, level):
    gz, blocks = levels[level]
    cand = G.first_candidates(gz, 32768)
    starts = {b[0] for b in blocks}
    held = [c for c in cand[1:] if c is not None]          # (the file's last piece may hold the final block's start only)
    assert len(held) + 1 >= 15 and all(c in starts for c in held) and None not in cand[1:-1]       # the condition of this test
    st = check(gz, TEXT, 32768)
    assert (st.pieces, st.pieces_dropped, st.recounts, st.members, st.trailing_bytes) == (len(held) + 1, 0, 0, 1, 0)


def test_pieces_below_the_block_size_merge(levels):
    gz, blocks = levels[6]
    cand = G.first_candidates(gz, 8192)
    starts = {b[0] for b in blocks}
    with_start = [c for c in cand[1:] if c is not None]
    assert all(c in starts for c in with_start) and len(with_start) < (len(cand) - 1) / 2        # most pieces hold no start
    st = check(gz, TEXT, 8192)
    assert (st.pieces, st.pieces_dropped) == (len(with_start) + 1, 0)


def _shapes():
    t = TEXT[:300000]
    a, b = t[:120000], t[120000:]
    on_border = member(a, 6, fname=b"")                                   # FNAME pads member 1 to a multiple of the piece size
    on_border = member(a, 6, fname=b"n" * (-(len(on_border)) % 4096))
    assert len(on_border) % 4096 == 0
    return {
        "stored": (member(t, 0), t, 0),
        "fixed": (member(t, 6, strategy=zlib.Z_FIXED), t, 0),
        "sync_flushes": (member(t, 6, flush_at=range(7000, len(t), 7000)), t, 0),
        "full_flushes": (member(t, 6, flush_at=range(50000, len(t), 50000), flush=zlib.Z_FULL_FLUSH), t, 0),
        "members_and_an_empty_one": (member(a, 9) + member(b"") + member(b, 1) + member(b""), t, 0),
        "header_fields": (member(a, 6, fname=b"reads.fq", fextra=b"XY\x03\x00abc", fcomment=b"made by hand", fhcrc=True) +
                          member(b, 6, fextra=b"", fhcrc=True), t, 0),
        "bgzf": (bgzf.compress(t, 6), t, 0),
        "trailing_zeros": (member(t, 6) + bytes(5000), t, 5000),
        "boundary_inside_a_piece": (member(a, 6) + member(b, 6), t, 0),
        "boundary_on_a_piece_border": (on_border + member(b, 6), t, 0),
        "python_gzip": (gzip.compress(t, 6), t, 0),
    }


SHAPES = _shapes()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_block_kind_and_gzip_shape(shape):
    gz, want, trailing = SHAPES[shape]
    assert gzip.decompress(gz) == want
    st = check(gz, want, 4096)
    assert st.trailing_bytes == trailing and st.members == len(G.walk_gzip(gz)[1])
    if shape == "boundary_on_a_piece_border":
        assert G.walk_gzip(gz)[1][1][0] % 4096 == 0


def test_history_that_is_mostly_markers():
    text, flushes = marker_text()
    gz = member(text, 9, flush_at=flushes)
    blocks, members = G.walk_gzip(gz)
    starts = {b[0] for b in blocks}
    cand = G.first_candidates(gz, 4096)
    assert len(gz) >= 8 * 4096 and all(c in starts for c in cand if c is not None)
    live = [blocks[0][0]] + [c for c in cand if c is not None]
    assert len(live) >= 8
    depth_w, shares, deepest, run_pieces = np.zeros(G.WIN, np.int64), [], 0, 0
    for a, e in zip(live, live[1:] + [8 * members[0][1]]):
        s = np.array(G.decode_piece(gz, a, e), np.int64)
        mk = (s & 0x8000) != 0
        shares.append(mk.mean())
        d = np.where(mk, 1 + depth_w[s & 0x7fff], 0)       # how many windows a byte is looked up through
        deepest = max(deepest, int(d.max()))
        run_pieces += bool(mk.all() and len(set(s.tolist())) == 1)         # a piece inside the run: distance 1 across its border
        depth_w = np.concatenate([depth_w, d])[-G.WIN:]
    assert sum(x > 0.5 for x in shares) >= len(shares) / 2 and deepest >= 3 and run_pieces >= 1
    st = check(gz, text, 4096)
    assert (st.pieces, st.pieces_dropped) == (len(live), 0)


def test_false_candidates_are_harmless():
    inner = raw_deflate(fastq_text(1000, 3), 6)
    gz = member(inner, 0)                                   # valid gzip: stored blocks whose payload is a DEFLATE stream
    starts = {b[0] for b in G.walk_gzip(gz)[0]}
    cand = G.first_candidates(gz, 16384)
    assert any(c is not None and c not in starts for c in cand)
    st = check(gz, inner, 16384)
    assert st.pieces_dropped >= 1 and st.pieces + st.pieces_dropped <= len(cand)


def _feed(gz, cuts, piece_bytes=4096, out_cap=None):
    """gz presented up to each cut in turn (what was not consumed again, followed by more): (outputs, calls)"""
    g = capi.Gunzipper(0, 1 << 20, 4 << 20, piece_bytes)
    pos, outs = 0, []
    for cut in list(cuts) + [len(gz)]:
        got, used, _ = g.run(gz[pos:cut], cut == len(gz), out_cap)
        assert 0 <= used <= cut - pos
        pos += used
        outs.append(got)
    g.close()
    assert pos == len(gz)
    return outs


def test_streaming_in_calls_of_any_size():
    gz = member(TEXT[:400000], 6, fname=b"a.fq") + member(TEXT[400000:], 6, fcomment=b"second")
    blocks, members = G.walk_gzip(gz)
    for stride in (100000, 4097):
        assert b"".join(_feed(gz, range(stride, len(gz), stride))) == TEXT
    second = members[1][0]
    cuts = sorted({5, second + 3, second - 4, len(gz) - 3, (blocks[3][0] >> 3) + 1, (blocks[3][0] >> 3) + 2, 200000})
    assert b"".join(_feed(gz, cuts)) == TEXT               # inside a header, inside a trailer, one byte past a block boundary


def test_capacity(levels):
    gz, blocks = levels[6]
    cand = G.first_candidates(gz, 32768)
    out_at = dict(zip([b[0] for b in blocks], np.cumsum([0] + [b[3] for b in blocks])))
    three = int(out_at[cand[3]])                            # the output of pieces 0, 1 and 2
    g = capi.Gunzipper(0, 4 << 20, 16 << 20, 32768)
    got, used, st = g.run(gz, True, three + 100)
    assert (len(got), used, st.pieces) == (three, cand[3] >> 3, 3) and got == TEXT[:three]
    rest, used2, _ = g.run(gz[used:], True)
    assert got + rest == TEXT and used + used2 == len(gz)
    g.close()
    g = capi.Gunzipper(0, 4 << 20, 16 << 20, 32768)
    small = int(out_at[cand[1]]) - 1
    rc, used, n, _ = g.run_raw(gz, True, C.addressof(C.create_string_buffer(small)), small, False)
    g.close()
    assert (rc, used, n) == (ERR_CAPACITY, 0, 0)


def _damaged(gz, kind):
    b = bytearray(gz)
    if kind == "flip":
        b[len(b) // 2] ^= 0x10
    elif kind == "crc":
        b[-8] ^= 0x10
    elif kind == "isize":
        b[-4] ^= 0x01
    elif kind == "reserved_flag":
        b[3] |= 0x20
    elif kind == "cut":
        del b[len(b) * 3 // 4:]
    return bytes(b)


@pytest.mark.parametrize("kind", ["flip", "crc", "isize", "reserved_flag", "cut"])
def test_damage_is_an_io_error_and_earlier_output_stays(levels, kind):
    gz, blocks = levels[6]
    bad = _damaged(gz, kind)
    guard, first, room = 4096, 150000, len(TEXT) + (1 << 20)     # room: damaged data may inflate to more than the text
    dev = torch.full((room + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    g = capi.Gunzipper(0, 4 << 20, 16 << 20, 32768)
    n1 = used = 0
    if kind != "reserved_flag":                             # an earlier call on the undamaged front of the file
        rc, used, n1, _ = g.run_raw(bad[:first], False, dev.data_ptr() + guard, room, True)
        assert rc == 0 and used > 0 and n1 > 0
    rc, used2, n2, _ = g.run_raw(bad[used:], True, dev.data_ptr() + guard + n1, room - n1, True)
    err = capi.lib().bwams_last_error()
    g.close()
    assert (rc, used2, n2) == (ERR_IO, 0, 0)
    m = re.search(rb"gzip member 0 at byte (\d+): (.*)", err)
    assert m and used <= int(m.group(1)) <= len(bad), err
    if kind == "crc":
        assert b"CRC32 mismatch" in err
    if kind == "isize":
        assert b"ISIZE" in err
    host = dev.cpu().numpy()
    assert host[guard:guard + n1].tobytes() == TEXT[:n1]
    assert (host[:guard] == 0xA5).all() and (host[guard + room:] == 0xA5).all()


def test_refusals():
    g = capi.Gunzipper(0, 1 << 20, 1 << 20, 4096)
    buf = C.create_string_buffer(1 << 20)
    for bad in (TEXT[:5000], zlib.compress(TEXT[:5000])):
        rc, used, n, _ = g.run_raw(bad, True, C.addressof(buf), 1 << 20, False)
        assert (rc, used, n) == (ERR_UNSUPPORTED, 0, 0)
    g.close()


def _chunks(open_fn, path, chunk_bases, paired, n_buffers):
    L = capi.lib()
    r = open_fn(path, chunk_bases, paired, n_buffers)
    out = []
    while True:
        text, nb, nr, nbases = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = L.bwams_reader_next(r, C.byref(text), C.byref(nb), C.byref(nr), C.byref(nbases))
        if rc == 1:
            break
        assert rc == 0, (rc, L.bwams_reader_error(r))
        out.append((C.string_at(text.value, nb.value), nr.value, nbases.value))
        capi._chk(L.bwams_reader_release(r, text), "bwams_reader_release")
    info = capi.reader_info(r)
    L.bwams_reader_close(r)
    return out, info


def _host_open(path, chunk_bases, paired, n_buffers):
    r = C.c_void_p()
    capi._chk(capi.lib().bwams_reader_open(path.encode(), C.c_int64(chunk_bases), int(paired), C.c_int64(0), n_buffers, C.byref(r)),
              "bwams_reader_open")
    return r


def _gunzip_open(path, chunk_bases, paired, n_buffers):
    return capi.reader_open_device2(path, 0, chunk_bases, paired, 0, n_buffers, capi.READER_GUNZIP)


def _plain_open(path, chunk_bases, paired, n_buffers):
    return capi.reader_open_device2(path, 0, chunk_bases, paired, 0, n_buffers, 0)


def _wrapped(n, seed):
    """records with wrapped sequence / quality lines, comments and CRLF, so chunk cuts do not fall on fixed strides"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(50, 260))
        s = bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, ln)])
        q = bytes((rng.integers(0, 41, ln) + 33).astype(np.uint8))
        eol = b"\r\n" if i % 7 == 3 else b"\n"
        if i % 5 == 0:
            out.append(b"@w%d c%d%s%s%s%s%s+%s%s%s%s%s" % (i, i, eol, s[:40], eol, s[40:], eol, eol, q[:40], eol, q[40:], eol))
        else:
            out.append(b"@w%d%s%s%s+%s%s%s" % (i, eol, s, eol, eol, q, eol))
    return b"".join(out)


@pytest.fixture(scope="module")
def reads_gz(tmp_path_factory):
    """(path of the .fq.gz, its text, the host reader's chunks by (chunk_bases, paired): computed once, shared by the cases)"""
    text = fastq_text(40000, 6) + _wrapped(3000, 7)
    p = tmp_path_factory.mktemp("gunzip_reader") / "reads.fq.gz"
    p.write_bytes(gzip.compress(text, 6))
    return str(p), text, {}


@pytest.mark.parametrize("chunk_bases", [150 * 3000 + 7, 10 ** 9, 1000])
@pytest.mark.parametrize("n_buffers", [1, 2, 3])
@pytest.mark.parametrize("paired", [False, True])
def test_gunzip_reader_equals_host_reader(reads_gz, paired, n_buffers, chunk_bases):
    path, text, host = reads_gz
    if (chunk_bases, paired) not in host:
        host[chunk_bases, paired] = _chunks(_host_open, path, chunk_bases, paired, 2)[0]
    got, info = _chunks(_gunzip_open, path, chunk_bases, paired, n_buffers)
    assert got == host[chunk_bases, paired]
    assert b"".join(x[0] for x in got) == text
    assert info.device_inflate == 2 and info.out_bytes == len(text) and info.in_bytes == len(open(path, "rb").read())


@pytest.mark.parametrize("paired", [False, True])
def test_without_the_flag_plain_gzip_stays_on_zlib(reads_gz, paired):
    path, text, _ = reads_gz
    got, info = _chunks(_plain_open, path, 150 * 2000, paired, 2)
    want, _ = _chunks(_host_open, path, 150 * 2000, paired, 2)
    assert got == want and info.device_inflate == 0 and info.out_bytes == len(text)


def test_gunzip_reader_reports_damage(tmp_path):
    bad = _damaged(gzip.compress(fastq_text(5000, 8), 6), "crc")
    p = tmp_path / "bad.fq.gz"
    p.write_bytes(bad)
    L = capi.lib()
    r = _gunzip_open(str(p), 10 ** 9, False, 2)
    text_p, nb, nr, nbs = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    rc = L.bwams_reader_next(r, C.byref(text_p), C.byref(nb), C.byref(nr), C.byref(nbs))
    err = L.bwams_reader_error(r)
    L.bwams_reader_close(r)
    assert rc == ERR_IO and b"gzip member 0 at byte %d" % (len(bad) - 8) in err and b"CRC32" in err


def test_fastq_gz_through_gunzip_reader_to_sam(tmp_path):
    from test_host_boundary import _setup
    g, ix, _, _ = _setup(seed=31)
    reads, _, _ = simulate.make_reads(g, 3000, seed=72)
    rng = np.random.default_rng(9)
    text = b"".join(b"@s%d\n%s\n+\n%s\n" % (i, bytes(b"ACGTN"[c] for c in r), bytes((rng.integers(0, 41, len(r)) + 33).astype(np.uint8)))
                    for i, r in enumerate(reads))
    plain, gzp = tmp_path / "r.fq", tmp_path / "r.fq.gz"
    plain.write_bytes(text)
    gzp.write_bytes(gzip.compress(text, 6))
    b = capi.Batch(ix, 1200, 1200 * 160)
    sams = []
    for open_fn, path in ((_host_open, plain), (_gunzip_open, gzp)):
        chunks, info = _chunks(open_fn, str(path), 150 * 1000, False, 2)
        assert len(chunks) >= 3
        sam, done = b"", 0
        for t, nr, _ in chunks:
            s, _ = b.process_chunk(t, n_processed=done)
            sam += s
            done += nr
        sams.append(sam)
    b.close()
    ix.close()
    assert info.device_inflate == 2 and sams[0] == sams[1] and sams[0].count(b"\n") >= len(reads)


def test_63_megabytes_in_calls_of_8_mib():
    text = fastq_text(200_000, 5)
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    gz = c.compress(text) + c.flush()
    g = capi.Gunzipper(0, 16 << 20, 64 << 20, 0)            # the default piece_bytes
    h, pos, end, calls, out, pieces = hashlib.sha256(), 0, 0, 0, 0, 0
    while pos < len(gz):
        end = min(max(end, pos) + (8 << 20), len(gz))
        got, used, st = g.run(gz[pos:end], end == len(gz))
        h.update(got)
        pos += used
        out += len(got)
        pieces += st.pieces
        calls += 1
        assert calls < 50
    g.close()
    assert calls >= 3 and pieces >= 40 and out == len(text) and h.hexdigest() == hashlib.sha256(text).hexdigest()
