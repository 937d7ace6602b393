"""BGZF written on the GPU (csrc/deflate.hip: bwams_deflater_*, bwams_sam_fetch_bgzf, bwams_writer_open_bgzf) against zlib and the
project's own inflater: round trips of edge-case and realistic inputs, the member format, determinism across handles and memory
kinds, the size against zlib level 1 on SAM-like text, the SAM path of a batch, file to file through the BGZF writer, and refusals."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest
import torch

from bwams import bgzf, capi, simulate
from test_gpu_inflate import _chunks, _device_open, fastq_text

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -3, -4
HEADER = bytes.fromhex("1f8b08040000000000ff06004243020000")[:16]     # bgzip's header up to BSIZE


def sam_like(n_bytes, seed=0, genome_len=50_000_000):
    """SAM-like text: 150-base reads from a random genome, qualities from 'F:,#' (0.85 / 0.10 / 0.04 / 0.01), the usual fields."""
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, genome_len, dtype=np.uint8)]
    n = n_bytes // 380 + 1
    pos = rng.integers(0, genome_len - 150, n)
    quals = np.frombuffer(b"F:,#", np.uint8)[rng.choice(4, (n, 150), p=[0.85, 0.10, 0.04, 0.01])]
    flags = rng.choice([0, 16], n)
    chrs = rng.integers(1, 23, n)
    nm = rng.integers(0, 4, n)
    lines = []
    for i in range(n):
        seq = genome[pos[i]:pos[i] + 150].tobytes()
        lines.append(b"r%09d\t%d\tchr%d\t%d\t60\t150M\t*\t0\t0\t%s\t%s\tNM:i:%d\tMD:Z:150\tAS:i:%d\tXS:i:0\n"
                     % (i, flags[i], chrs[i], pos[i] + 1, seq, quals[i].tobytes(), nm[i], 150 - 5 * nm[i]))
    return b"".join(lines)[:n_bytes]


@pytest.fixture(scope="module")
def deflater():
    d = capi.Deflater(0, 64 << 20)
    yield d
    d.close()


@pytest.fixture(scope="module")
def inflater():
    f = capi.Inflater(0, 64 << 20, 64 << 20)
    yield f
    f.close()


def _inputs():
    rng = np.random.default_rng(5)
    blk = rng.integers(0, 256, 40 << 10, dtype=np.uint8).tobytes()
    one_dist = b"".join(bytes([65 + (i % 26)]) for i in range(26)) * 2     # a 26-byte run repeated once: one distance
    return {
        "empty": b"",
        "one": b"x",
        "65279": rng.integers(0, 4, 65279, dtype=np.uint8).tobytes(),
        "65280": fastq_text(300)[:65280],
        "65281": fastq_text(300)[:65281],
        "3x65280": fastq_text(1000)[:3 * 65280],
        "random_8MiB": rng.integers(0, 256, 8 << 20, dtype=np.uint8).tobytes(),
        "zeros_1MiB": bytes(1 << 20),
        "dist_32768": blk[:32768] + blk,                                      # the block again 32768 bytes on
        "all_bytes": bytes(range(256)),
        "no_repeats": bytes(range(200)),
        "one_distance": one_dist,
        "fastq": fastq_text(20000, seed=3),
        "sam_like": sam_like(3 << 20, seed=4),
    }


INPUTS = _inputs()


def _check_format(data, out, eof):
    ms = bgzf.walk(out)
    body = ms[:-1] if eof else ms
    if eof:
        assert out.endswith(bgzf.EOF_MEMBER) and ms[-1][4] == 0
    assert len(body) == -(-len(data) // bgzf.BLOCK)
    for k, (off, hdr, total, crc, isize) in enumerate(body):
        assert hdr == 18 and total <= 65536
        assert out[off:off + 16] == HEADER
        assert isize == min(bgzf.BLOCK, len(data) - bgzf.BLOCK * k)
        assert crc == zlib.crc32(data[bgzf.BLOCK * k:bgzf.BLOCK * k + isize])
    assert len(out) <= capi.deflate_bound(len(data))
    return body


@pytest.mark.parametrize("name", list(INPUTS))
def test_round_trip_and_format(deflater, inflater, name):
    data = INPUTS[name]
    cap = capi.deflate_bound(len(data)) + 64
    buf = C.create_string_buffer(b"\xa5" * cap, cap)
    rc, n, st = deflater.run_raw(data, C.addressof(buf), cap, flags=capi.DEFLATE_EOF)
    assert rc == 0
    out = buf.raw[:n]
    assert buf.raw[n:] == b"\xa5" * (cap - n)                                     # guard bytes past n_out
    assert gzip.decompress(out) == data
    body = _check_format(data, out, eof=True)
    assert st.members == len(body) and st.in_bytes == len(data) and st.out_bytes == n
    if data:
        got, used, _ = inflater.run(out[:-len(bgzf.EOF_MEMBER)])
        assert got == data and used == n - len(bgzf.EOF_MEMBER)
    if name == "random_8MiB":                                                    # incompressible: every member stored
        for off, hdr, total, _, isize in body:
            assert total == isize + 31 and bgzf.first_block_header(out[off:off + total]) == (1, 0)
    print(f"{name}: {len(data)} -> {n} bytes")


def de_bruijn(k, n):
    """a sequence over k letters in which every n-letter string occurs once (its n-1 first letters appended): no 3-byte repeat"""
    a, seq = [0] * k * n, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(65 + x for x in seq + seq[:n - 1])


def _block(out):
    """(BTYPE, number of distance codes) of the first member's block (the second is only meaningful for BTYPE 2)"""
    b = int.from_bytes(out[18:22], "little")
    return (b >> 1) & 3, ((b >> 8) & 31) + 1


def test_members_with_no_and_one_distance_code_inflate(deflater, inflater):
    # dynamic blocks (few letters: short literal codes) with no match at all, and with matches at one distance only
    for data, matches in ((de_bruijn(4, 3), False), (de_bruijn(8, 3), False), (de_bruijn(4, 3) * 2, True), (de_bruijn(8, 3) * 2, True)):
        out, _ = deflater.run(data)
        assert _block(out)[0] == 2
        assert gzip.decompress(out) == data
        assert inflater.run(out)[0] == data
        print(len(data), "->", len(out), "distance codes", _block(out)[1], "matches" if matches else "no matches")


def test_determinism_across_runs_handles_and_memory(deflater):
    data = INPUTS["sam_like"] + INPUTS["fastq"][:1_000_003]
    ref, _ = deflater.run(data)
    assert deflater.run(data)[0] == ref
    small = capi.Deflater(0, 65536)                                              # one member per launch
    try:
        assert small.run(data)[0] == ref
    finally:
        small.close()
    dev_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    assert deflater.run((dev_in.data_ptr(), len(data)))[0] == ref              # device input, host output
    cap = capi.deflate_bound(len(data))
    dev_out = torch.full((cap + 256,), 0x5A, dtype=torch.uint8, device="cuda:0")
    for src, on_dev in ((data, False), ((dev_in.data_ptr(), len(data)), True)):
        dev_out.fill_(0x5A)
        torch.cuda.synchronize()
        rc, n, _ = deflater.run_raw(src, dev_out.data_ptr(), cap, in_on_device=on_dev, out_on_device=True)
        assert rc == 0
        got = dev_out.cpu().numpy().tobytes()
        assert got[:n] == ref and got[n:] == b"\x5a" * (cap + 256 - n)


def test_calls_concatenate_into_one_stream(deflater):
    parts = [INPUTS["fastq"][:100_000], b"", INPUTS["sam_like"][:70_001], b"z"]
    out = b"".join(deflater.run(p)[0] for p in parts) + deflater.run(b"", eof=True)[0]
    assert deflater.run(b"", eof=True)[0] == bgzf.EOF_MEMBER
    assert gzip.decompress(out) == b"".join(parts)
    bgzf.walk(out)


def test_ratio_against_zlib_level_1(deflater):
    text = sam_like(32 << 20, seed=11)
    out, st = deflater.run(text, eof=True)
    z1 = bgzf.compress(text, level=1)
    print(f"SAM-like {len(text)} bytes: device {len(out)} ({len(text) / len(out):.3f}x), zlib-1 {len(z1)} ({len(text) / len(z1):.3f}x), "
          f"size vs zlib-1 {len(out) / len(z1):.4f}; kernel {st.ms_kernel:.1f} ms")
    assert gzip.decompress(out) == text
    assert len(out) <= len(z1)
    for name in ("fastq", "sam_like", "zeros_1MiB", "dist_32768"):
        d = INPUTS[name]
        o, _ = deflater.run(d, eof=True)
        print(f"{name}: size vs zlib-1 {len(o) / len(bgzf.compress(d, level=1)):.4f}")


def _batch_sam(paired):
    from test_host_boundary import _setup
    g, ix, _, _ = _setup(seed=31)
    rng = np.random.default_rng(9)
    if paired:
        reads = simulate.make_read_pairs(g, 600, seed=12)
        names = [b"p%d" % (i // 2) for i in range(len(reads))]
    else:
        reads, _, _ = simulate.make_reads(g, 1200, seed=72)
        names = [b"s%d" % i for i in range(len(reads))]
    text = b"".join(b"@%s\n%s\n+\n%s\n" % (nm, bytes(b"ACGTN"[c] for c in r), bytes((rng.integers(0, 41, len(r)) + 33).astype(np.uint8)))
                    for nm, r in zip(names, reads))
    return ix, text, len(reads)


@pytest.mark.parametrize("paired", [False, True])
def test_sam_fetch_bgzf_inflates_to_sam_fetch(deflater, paired):
    ix, text, n = _batch_sam(paired)
    b = capi.Batch(ix, n, n * 160)
    try:
        sam, _ = b.process_chunk(text, paired=paired)
        assert sam.count(b"\n") >= n
        gz = b.sam_fetch_bgzf(deflater, eof=True)
        assert gzip.decompress(gz) == sam and gz.endswith(bgzf.EOF_MEMBER)
        assert gz == deflater.run(sam, eof=True)[0]
    finally:
        b.close()
        ix.close()


def _write(tmp_path, name, n_shards, puts, bgzf_dev=None):
    """puts: (shard, seq, bytes, is_members) in any order; returns the shard files' bytes"""
    L = capi.lib()
    w = C.c_void_p()
    path = str(tmp_path / name)
    if bgzf_dev is None:
        capi._chk(L.bwams_writer_open(path.encode(), n_shards, C.byref(w)), "bwams_writer_open")
    else:
        capi._chk(L.bwams_writer_open_bgzf(path.encode(), n_shards, bgzf_dev, C.byref(w)), "bwams_writer_open_bgzf")
    for s, q, data, members in puts:
        if members:
            capi._chk(L.bwams_writer_put_bgzf(w, s, C.c_int64(q), data, C.c_int64(len(data))), "bwams_writer_put_bgzf")
        else:
            capi._chk(L.bwams_writer_put(w, s, C.c_int64(q), data, C.c_int64(len(data))), "bwams_writer_put")
    capi._chk(L.bwams_writer_close(w), "bwams_writer_close")
    if n_shards == 1:
        return [open(path, "rb").read()]
    ext = ".sam.gz" if bgzf_dev is not None else ".sam"
    return [open(f"{path}.{s}{ext}", "rb").read() for s in range(n_shards)]


@pytest.mark.parametrize("n_shards", [1, 3])
def test_bgzf_fastq_to_bgzf_sam_file(tmp_path, deflater, n_shards):
    from test_host_boundary import _setup
    g, ix, _, _ = _setup(seed=31)
    reads, _, _ = simulate.make_reads(g, 3000, seed=72)
    rng = np.random.default_rng(9)
    text = b"".join(b"@s%d\n%s\n+\n%s\n" % (i, bytes(b"ACGTN"[c] for c in r), bytes((rng.integers(0, 41, len(r)) + 33).astype(np.uint8)))
                    for i, r in enumerate(reads))
    fq = tmp_path / "r.fq.bgz"
    fq.write_bytes(bgzf.compress(text, 6))
    chunks, info = _chunks(_device_open, str(fq), 150 * 500, False, 2)
    assert info.device_inflate == 1 and len(chunks) >= 4
    b = capi.Batch(ix, 1200, 1200 * 160)
    plain, gz, done = [], [], 0
    try:
        for i, (t, nr, _) in enumerate(chunks):
            s, _ = b.process_chunk(t, n_processed=done)
            done += nr
            shard, seq = i % n_shards, i // n_shards
            plain.append((shard, seq, s, False))
            gz.append((shard, seq, b.sam_fetch_bgzf(deflater) if i % 2 else s, bool(i % 2)))
    finally:
        b.close()
        ix.close()
    want = _write(tmp_path, "plain.sam", n_shards, plain[::-1])
    got = _write(tmp_path, "out.sam", n_shards, gz[::-1], bgzf_dev=0)
    for w_, g_ in zip(want, got):
        assert g_.endswith(bgzf.EOF_MEMBER)
        bgzf.walk(g_)
        assert gzip.decompress(g_) == w_
    assert sum(len(w_) for w_ in want) > 0


def test_refusals(deflater):
    L = capi.lib()
    data = INPUTS["fastq"][:200_000]
    need = capi.deflate_bound(len(data))
    buf = C.create_string_buffer(b"\x33" * need, need)
    rc, n, _ = deflater.run_raw(data, C.addressof(buf), need - 1)
    assert rc == ERR_CAPACITY and n == need and buf.raw == b"\x33" * need                 # nothing written
    assert deflater.run_raw(data, C.addressof(buf), need)[0] == 0
    n_out = C.c_int64(0)
    assert L.bwams_deflater_run(None, data, len(data), 0, C.addressof(buf), need, 0, 0, C.byref(n_out), None) == ERR_ARG
    assert L.bwams_deflater_run(deflater.h, None, 5, 0, C.addressof(buf), need, 0, 0, C.byref(n_out), None) == ERR_ARG
    assert L.bwams_deflater_run(deflater.h, data, len(data), 0, None, need, 0, 0, C.byref(n_out), None) == ERR_ARG
    assert L.bwams_deflater_run(deflater.h, data, -1, 0, C.addressof(buf), need, 0, 0, C.byref(n_out), None) == ERR_ARG
    assert L.bwams_deflater_run(deflater.h, data, len(data), 0, C.addressof(buf), need, 0, 0x10, C.byref(n_out), None) == ERR_ARG
    h = C.c_void_p()
    assert L.bwams_deflater_create(0, 1000, C.byref(h)) == ERR_ARG
    assert L.bwams_deflater_create(0, 1 << 20, None) == ERR_ARG
    # a batch with no SAM run yet, and a deflater bound to another device than the batch
    from test_host_boundary import _setup
    _, ix, _, _ = _setup(seed=31)
    b = capi.Batch(ix, 100, 100 * 160)
    try:
        assert L.bwams_sam_fetch_bgzf(b.h, deflater.h, C.addressof(buf), need, 0, C.byref(n_out)) == ERR_ARG
        assert L.bwams_sam_fetch_bgzf(b.h, None, C.addressof(buf), need, 0, C.byref(n_out)) == ERR_ARG
        b.process_chunk(fastq_text(50, seed=2))
        assert L.bwams_sam_fetch_bgzf(b.h, deflater.h, C.addressof(buf), 10, 0, C.byref(n_out)) == ERR_CAPACITY
        if torch.cuda.device_count() > 1:
            other = capi.Deflater(1, 1 << 20)
            try:
                assert L.bwams_sam_fetch_bgzf(b.h, other.h, C.addressof(buf), need, 0, C.byref(n_out)) == ERR_ARG
            finally:
                other.close()
        else:                                                                     # the check itself: the handle's device field
            other = capi.Deflater(0, 1 << 20)
            try:
                C.cast(other.h, C.POINTER(C.c_int))[0] = 1
                assert L.bwams_sam_fetch_bgzf(b.h, other.h, C.addressof(buf), need, 0, C.byref(n_out)) == ERR_ARG
                C.cast(other.h, C.POINTER(C.c_int))[0] = 0
            finally:
                other.close()
        w = C.c_void_p()
        assert L.bwams_writer_open_bgzf(None, 1, 0, C.byref(w)) == ERR_ARG
    finally:
        b.close()
        ix.close()
