"""The BGZF writer and header walker (bwams/bgzf.py) that the device inflater's tests and lab are built on: its files are gzip,
its member list is the BSIZE / ISIZE chain, and its options really make stored, fixed, dynamic and multi-block members."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from bwams import bgzf


def _text(n=200000, seed=1):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(b"ACGTN\n", np.uint8)[rng.integers(0, 6, n)])


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_writer_output_is_gzip_of_the_input(level):
    for data in (b"", b"x", _text(), os.urandom(150000)):
        z = bgzf.compress(data, level)
        assert gzip.decompress(z) == data
        assert z.endswith(bgzf.EOF_MEMBER)


def test_walker_follows_the_bsize_isize_chain():
    data = _text(400000, 2)
    z = bgzf.compress(data, 6, flush_every=7000)
    ms = bgzf.walk(z)
    assert len(ms) == -(-len(data) // bgzf.BLOCK) + 1
    at = 0
    for i, (p, hdr, total, crc, isize) in enumerate(ms):
        assert p == at and hdr == 18
        assert struct.unpack_from("<H", z, p + 16)[0] + 1 == total                    # BSIZE
        piece = data[i * bgzf.BLOCK:(i + 1) * bgzf.BLOCK]
        assert isize == len(piece) and crc == zlib.crc32(piece)
        assert zlib.decompress(z[p + hdr:p + total - 8], -15) == piece
        at += total
    assert at == len(z) and ms[-1][4] == 0
    with pytest.raises(ValueError):
        bgzf.walk(z[:-5])
    with pytest.raises(ValueError):
        bgzf.walk(gzip.compress(data))


def test_options_make_every_block_kind():
    data = _text(60000, 3)
    first = bgzf.first_block_header
    assert first(bgzf.member(data, 0))[1] == 0                                         # level 0: stored
    assert first(bgzf.member(os.urandom(60000), 6))[1] == 0                            # incompressible: stored
    assert first(bgzf.member(data, 6, zlib.Z_FIXED)) == (1, 1)                         # one fixed block
    assert first(bgzf.member(data, 6)) == (1, 2)                                       # one dynamic block
    m = bgzf.member(data, 6, flush_at=(20000, 40000))
    assert first(m) == (0, 2)                                                          # dynamic, more blocks follow
    body = m[18:-8]
    assert b"\x00\x00\xff\xff" in body                                                 # the sync flushes' empty stored blocks
    assert zlib.decompress(body, -15) == data
