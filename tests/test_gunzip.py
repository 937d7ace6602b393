"""bwams/gunzip.py, the pure-Python restatement of csrc/gunzip.hip, against zlib: its walk over a DEFLATE stream, its candidate test
(exactly the non-final dynamic block starts of zlib-made FASTQ streams), and piece-wise decoding with markers plus resolving."""
import gzip
import zlib

import pytest

from bwams import gunzip as G
from gunzip_util import fastq_text, marker_text, member, raw_deflate

TEXT = fastq_text(3000, 1)


@pytest.fixture(scope="module", params=[1, 6, 9])
def stream(request):
    raw = raw_deflate(TEXT, request.param)
    assert zlib.decompress(raw, -15) == TEXT
    return raw, G.walk(raw)


def test_walk_lists_the_blocks_of_a_zlib_stream(stream):
    raw, (blocks, end) = stream
    assert sum(b[3] for b in blocks) == len(TEXT)
    assert [b[2] for b in blocks] == [0] * (len(blocks) - 1) + [1] and (end + 7) // 8 == len(raw)
    assert 28 <= len(blocks) <= 32 and all(b[1] == 2 for b in blocks)
    assert max(b[0] - a[0] for a, b in zip(blocks, blocks[1:])) <= 21 * 1024 * 8


def test_candidates_are_exactly_the_non_final_dynamic_block_starts(stream):
    raw, (blocks, _) = stream
    assert G.candidates(raw, 0, 8 * len(raw)) == [b[0] for b in blocks if b[1] == 2 and not b[2]]


def test_piecewise_decode_and_resolve_equals_zlib(stream):
    raw, (blocks, end) = stream
    cuts = [b[0] for b in blocks][::5] + [end]
    out, win, markers = b"", b"", 0
    for a, e in zip(cuts, cuts[1:]):
        sym = G.decode_piece(raw, a, e)
        markers += sum(1 for s in sym if s & 0x8000)
        out += G.resolve(sym, win)
        win = G.next_window(sym, win)
    assert out == TEXT and markers > 0


def test_every_block_kind_and_gzip_header_shape():
    small = TEXT[:60000]
    for raw in (raw_deflate(small, 0), raw_deflate(small, 6, zlib.Z_FIXED), raw_deflate(small, 6, flush_at=(10000, 30000)),
                raw_deflate(small, 6, flush_at=(20000,), flush=zlib.Z_FULL_FLUSH)):
        blocks, _ = G.walk(raw)
        assert sum(b[3] for b in blocks) == len(small)
        front = G.decode_piece(raw, blocks[0][0], blocks[-1][0])          # every block but the last, as one piece
        assert G.resolve(front, b"") == small[:sum(b[3] for b in blocks[:-1])]
    gz = member(small, 6, fname=b"reads.fq", fextra=b"AB\x02\x00xy", fcomment=b"a comment", fhcrc=True) + member(b"") + gzip.compress(small)
    assert gzip.decompress(gz) == small * 2
    blocks, members = G.walk_gzip(gz)
    assert len(members) == 3 and sum(b[3] for b in blocks) == 2 * len(small) and members[-1][1] + 8 == len(gz)


def test_candidate_test_refuses_what_the_decoder_refuses():
    raw = raw_deflate(TEXT[:40000], 6, flush_at=(20000,))
    blocks, _ = G.walk(raw)
    at = blocks[0][0]
    assert G.is_candidate(raw, at)
    bad = bytearray(raw)
    bad[0] |= 1                                          # BFINAL set: a final block is no candidate
    assert not G.is_candidate(bytes(bad), at)
    assert not G.is_candidate(raw[:40], at)              # the header runs past the end
    assert not G.is_candidate(raw_deflate(TEXT[:1000], 6, zlib.Z_FIXED), 0)


def test_marker_text_has_the_shape_the_gpu_test_needs():
    text, flushes = marker_text()
    gz = member(text, 9, flush_at=flushes)
    assert gzip.decompress(gz) == text and len(gz) >= 8 * 4096
