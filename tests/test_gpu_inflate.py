"""BGZF inflated on the GPU (csrc/inflate.hip: bwams_inflater_*, bwams_reader_open_device) against zlib, the reference's own
dependency for this step: every DEFLATE block kind, partial input and capacity, refusals, damaged members (the kernel's checks, with
the output ranges of the other members untouched), a 1 M-read FASTQ in several calls, the device reader chunk for chunk against
bwams_reader_open, and two end-to-end compositions (FASTQ -> SAM, FASTA -> index files)."""
import ctypes as C
import gzip
import hashlib
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from bwams import bgzf, capi, simulate

pytestmark = pytest.mark.gpu

ERR_IO, ERR_CAPACITY, ERR_UNSUPPORTED = -2, -4, -6


def fastq_text(n, seed=0, read_len=150):
    """n FASTQ records of fixed shape (name, read_len random bases, '+', read_len qualities), built with numpy."""
    rng = np.random.default_rng(seed)
    name = np.frombuffer(b"".join(b"@r%09d\n" % i for i in range(n)), np.uint8).reshape(n, 12)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len))]
    seq[rng.random((n, read_len)) < 0.002] = ord("N")
    qual = (rng.integers(0, 41, (n, read_len)) + 33).astype(np.uint8)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0)
    return np.concatenate([name, seq, nl, plus, qual, nl], axis=1).tobytes()


# a hand-made fixed-Huffman stream (zlib never emits distance 32768: its matches stay MIN_LOOKAHEAD inside the window)
_LB = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LE = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DB = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
       12289, 16385, 24577]
_DE = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_member(ops):
    """ops: literal bytes or (length, distance) -> a BGZF member of one final fixed-Huffman block, and its text."""
    acc, n, out, text = 0, 0, bytearray(), bytearray()

    def bits(v, k):
        nonlocal acc, n
        acc |= v << n
        n += k
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8

    def huff(code, k):
        bits(int(format(code, f"0{k}b")[::-1], 2), k)

    def sym(x):
        if x < 144:
            huff(0x30 + x, 8)
        elif x < 256:
            huff(0x190 + x - 144, 9)
        elif x < 280:
            huff(x - 256, 7)
        else:
            huff(0xC0 + x - 280, 8)

    bits(1, 1)
    bits(1, 2)
    for op in ops:
        if isinstance(op, (bytes, bytearray)):
            for c in op:
                sym(c)
            text += op
        else:
            ln, d = op
            i = max(k for k in range(29) if _LB[k] <= ln)
            sym(257 + i)
            bits(ln - _LB[i], _LE[i])
            j = max(k for k in range(30) if _DB[k] <= d)
            huff(j, 5)
            bits(d - _DB[j], _DE[j])
            for _ in range(ln):
                text.append(text[-d])
    sym(256)
    if n:
        out.append(acc & 255)
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, 18 + len(out) + 8 - 1)
    return hdr + bytes(out) + struct.pack("<II", zlib.crc32(text), len(text)), bytes(text)


def _cases():
    fq = fastq_text(1500, 1)
    rnd = os.urandom(150000)
    far, far_text = fixed_member([os.urandom(32768), (258, 32768), (258, 32768), b"x", (258, 1), (3, 1), (100, 32768)])
    run, run_text = fixed_member([b"A", *([(258, 1)] * 200)])
    ex = fq[:65536]
    return {
        "stored_level0": bgzf.compress(fq[:200000], 0),
        "stored_random": bgzf.compress(rnd, 6),
        "fixed": bgzf.compress(fq, 6, zlib.Z_FIXED),
        "dynamic_1": bgzf.compress(fq, 1),
        "dynamic_6": bgzf.compress(fq, 6),
        "dynamic_9": bgzf.compress(fq, 9),
        "rle": bgzf.compress(fq, 6, zlib.Z_RLE),
        "huffman_only": bgzf.compress(fq, 6, zlib.Z_HUFFMAN_ONLY),
        "filtered": bgzf.compress(fq, 6, zlib.Z_FILTERED),
        "sync_flushes": bgzf.compress(fq, 6, flush_every=3000) + bgzf.member(fq[:9000], 6, flush_at=(0, 0, 4000, 9000)),
        "exactly_65536": bgzf.compress(ex, 6, block=65536) + bgzf.compress(ex[::-1], 1, zlib.Z_FIXED, block=65536),
        "eof_only": bgzf.EOF_MEMBER,
        "mixed_levels": bgzf.member(fq[:30000], 9) + bgzf.member(rnd[:1000], 6) + bgzf.member(b"", 6) + bgzf.member(fq[:5000], 6, zlib.Z_FIXED),
        "distance_32768": far + run + bgzf.EOF_MEMBER,
    }


CASES = _cases()


@pytest.fixture(scope="module")
def inflater():
    f = capi.Inflater(0, 4 << 20, 16 << 20)
    yield f
    f.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_block_kind_equals_zlib(inflater, case):
    z = CASES[case]
    want = gzip.decompress(z)
    got, used, st = inflater.run(z)
    assert got == want and used == len(z) and st.members == len(bgzf.walk(z)) and st.out_bytes == len(want)
    dev = torch.full((len(want) + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")       # device output, guard bytes behind it
    rc, used, n, _ = inflater.run_raw(z, dev.data_ptr(), len(want), True)
    assert (rc, used, n) == (0, len(z), len(want))
    host = dev.cpu().numpy().tobytes()
    assert host[:len(want)] == want and host[len(want):] == b"\x5a" * 64


def test_partial_input_and_capacity(inflater):
    data = fastq_text(3000, 2)
    z = bgzf.compress(data, 6)
    ms = bgzf.walk(z)
    cut = ms[3][0] + 100                                       # inside member 3
    got, used, _ = inflater.run(z[:cut])
    assert used == ms[3][0] and got == data[:3 * bgzf.BLOCK]
    rest, used2, _ = inflater.run(z[used:])
    assert used2 == len(z) - used and got + rest == data
    got, used, _ = inflater.run(z[:10])                        # not even a whole header: nothing yet
    assert (got, used) == (b"", 0)
    cap = 2 * bgzf.BLOCK + 1000                                # whole members only
    got, used, _ = inflater.run(z, out_cap=cap)
    assert used == ms[2][0] and got == data[:2 * bgzf.BLOCK]
    rc, used, n, _ = inflater.run_raw(z, C.addressof(C.create_string_buffer(1000)), 1000, False)
    assert (rc, used, n) == (ERR_CAPACITY, 0, 0)


def test_refusals(inflater):
    data = fastq_text(500, 3)
    buf = C.create_string_buffer(1 << 20)
    for bad in (gzip.compress(data), data, b"\x1f\x8c" + bgzf.compress(data)[2:], zlib.compress(data)):
        rc, used, n, _ = inflater.run_raw(bad, C.addressof(buf), 1 << 20, False)
        assert (rc, used, n) == (ERR_UNSUPPORTED, 0, 0)
    # BGZF members followed by something else: the members go, the call stops in front of the rest
    z = bgzf.compress(data, 6)
    got, used, _ = inflater.run(z + gzip.compress(b"tail"))
    assert got == data and used == len(z)


def _damaged(z, kind):
    ms = bgzf.walk(z)
    k = 1
    p, hdr, total, _, _ = ms[k]
    b = bytearray(z)
    if kind == "crc":
        b[p + total - 8] ^= 0x10
    elif kind == "isize":
        b[p + total - 4] ^= 0x01
    else:                                                       # bits inside the dynamic block's body, well past its code tables
        assert bgzf.first_block_header(z[p:p + total])[1] == 2
        at = p + hdr + int(kind.split("_")[1])
        b[at] ^= 0x24
    return bytes(b), k, ms


@pytest.mark.parametrize("kind", ["crc", "isize", "flip_2000", "flip_9000", "flip_20000"])
def test_damaged_member_is_an_io_error_and_writes_stay_in_range(kind):
    data = fastq_text(2000, 4)
    z = bgzf.compress(data, 6)
    bad, k, ms = _damaged(z, kind)
    guard = 4096
    dev = torch.full((len(data) + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    f = capi.Inflater(0, 4 << 20, 16 << 20)                    # a fresh handle: the error counts members from 0
    rc, used, n, _ = f.run_raw(bad, dev.data_ptr() + guard, len(data), True)
    f.close()
    assert (rc, used, n) == (ERR_IO, 0, 0)
    assert b"BGZF member %d at byte %d" % (k, ms[k][0]) in capi.lib().bwams_last_error()
    host = dev.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + len(data):] == 0xA5).all()
    off = np.concatenate([[0], np.cumsum([m[4] for m in bgzf.walk(bad)])])      # where the host puts each member: the damaged chain
    for j in range(len(ms) - 1):
        seg = host[guard + off[j]:guard + off[j + 1]].tobytes()
        if j == k:
            assert seg == b"\xa5" * len(seg)                   # the damaged member's range: not written
        else:                                                   # every other member: its own bytes, or untouched
            assert seg == data[j * bgzf.BLOCK:(j + 1) * bgzf.BLOCK] or seg == b"\xa5" * len(seg)


def test_one_million_reads_in_several_calls():
    text = fastq_text(1_000_000, 5)
    z = bgzf.compress(text, 6)
    f = capi.Inflater(0, 8 << 20, 64 << 20)
    h, at, calls, out = hashlib.sha256(), 0, 0, 0
    while at < len(z):
        got, used, st = f.run(z[at:at + (8 << 20)], out_cap=64 << 20)
        assert used > 0
        h.update(got)
        at += used
        out += len(got)
        calls += 1
    f.close()
    assert calls >= 10 and out == len(text)
    assert h.hexdigest() == hashlib.sha256(text).hexdigest()


def _chunks(open_fn, path, chunk_bases, paired, n_buffers):
    L = capi.lib()
    L.bwams_reader_error.restype = C.c_char_p
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


def _device_open(path, chunk_bases, paired, n_buffers):
    return capi.reader_open_device(path, 0, chunk_bases, paired, 0, n_buffers)


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


@pytest.mark.parametrize("paired", [False, True])
def test_device_reader_equals_host_reader(tmp_path, paired):
    text = fastq_text(40000, 6) + _wrapped(3000, 7)
    bg = tmp_path / "reads.fq.bgz"
    bg.write_bytes(bgzf.compress(text, 6, flush_every=20000))
    for n_buffers in (1, 2, 3):
        for chunk_bases in (150 * 3000 + 7, 10 ** 9, 1000):
            want, _ = _chunks(_host_open, str(bg), chunk_bases, paired, n_buffers)
            got, info = _chunks(_device_open, str(bg), chunk_bases, paired, n_buffers)
            assert got == want, (n_buffers, chunk_bases)
            assert b"".join(g[0] for g in got) == text
            assert info.device_inflate == 1 and info.out_bytes == len(text) and info.in_bytes == bg.stat().st_size
    # plain gzip and uncompressed: the zlib path, the same chunks
    for name, blob in (("reads.fq.gz", gzip.compress(text)), ("reads.fq", text)):
        p = tmp_path / name
        p.write_bytes(blob)
        want, _ = _chunks(_host_open, str(p), 150 * 2000, paired, 2)
        got, info = _chunks(_device_open, str(p), 150 * 2000, paired, 2)
        assert got == want and info.device_inflate == 0 and info.out_bytes == len(text)


def test_device_reader_reports_damage(tmp_path):
    text = fastq_text(5000, 8)
    bad, k, ms = _damaged(bgzf.compress(text, 6), "crc")
    p = tmp_path / "bad.fq.bgz"
    p.write_bytes(bad)
    L = capi.lib()
    L.bwams_reader_error.restype = C.c_char_p
    r = capi.reader_open_device(str(p), 0, 10 ** 9, False, 0, 2)
    text_p, nb, nr, nbs = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    rc = L.bwams_reader_next(r, C.byref(text_p), C.byref(nb), C.byref(nr), C.byref(nbs))
    err = L.bwams_reader_error(r)
    L.bwams_reader_close(r)
    assert rc == ERR_IO and b"BGZF member %d at byte %d" % (k, ms[k][0]) in err and b"CRC32" in err


def test_bgzf_fastq_through_device_reader_to_sam(tmp_path):
    from test_host_boundary import _setup
    g, ix, _, _ = _setup(seed=31)
    reads, _, _ = simulate.make_reads(g, 3000, seed=72)
    rng = np.random.default_rng(9)
    text = b"".join(b"@s%d\n%s\n+\n%s\n" % (i, bytes(b"ACGTN"[c] for c in r), bytes((rng.integers(0, 41, len(r)) + 33).astype(np.uint8)))
                    for i, r in enumerate(reads))
    plain, bg = tmp_path / "r.fq", tmp_path / "r.fq.bgz"
    plain.write_bytes(text)
    bg.write_bytes(bgzf.compress(text, 6))
    b = capi.Batch(ix, 1200, 1200 * 160)
    sams = []
    for open_fn, path in ((_host_open, plain), (_device_open, bg)):
        chunks, _ = _chunks(open_fn, str(path), 150 * 1000, False, 2)
        assert len(chunks) >= 3
        sam, done = b"", 0
        for t, nr, _ in chunks:
            s, _ = b.process_chunk(t, n_processed=done)
            sam += s
            done += nr
        sams.append(sam)
    b.close()
    ix.close()
    assert sams[0] == sams[1] and sams[0].count(b"\n") >= len(reads)


def test_bgzipped_fasta_inflated_on_device_to_index_files(tmp_path):
    from test_gpu_fasta_index import make_fasta
    text = make_fasta(11, n_contigs=40, total=3_000_000, n_total=200_000)
    plain = tmp_path / "ref.fa"
    plain.write_bytes(text)
    z = bgzf.compress(text, 6)
    f = capi.Inflater(0, 32 << 20, 64 << 20)
    dev = torch.empty(len(text), dtype=torch.uint8, device="cuda:0")
    rc, used, n, _ = f.run_raw(z, dev.data_ptr(), len(text), True)
    f.close()
    assert (rc, used, n) == (0, len(z), len(text))
    a = capi.Index.from_fasta(dev)
    a.save(str(tmp_path / "dev"))
    a.close()
    b = capi.Index.from_fasta_file(str(plain))
    b.save(str(tmp_path / "file"))
    b.close()
    for e in ("ann", "amb", "pac", "bwt.2bit.64", "0123"):
        assert (tmp_path / f"dev.{e}").read_bytes() == (tmp_path / f"file.{e}").read_bytes(), e
