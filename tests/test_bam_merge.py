"""Several BAM files merged as one stream, on the CPU (include/bwams.h above bwams_bam_file_open_merge): rule M7's rounds
(bwams.merge.rounds) concatenated against rule M4's order (bwams.merge.merge_records) on inputs drawn so that ties dominate, and rule
M3's header merge: bwams.merge.merge_header against hand-written expectations, bwams_bam_header_merge of the library and
host/bam_merge_header.cpp built alone with its own main (tools/bam_header_merge_check.cpp) under -fsanitize=address,undefined give
the same bytes, and a block cut off at any length is an error return."""
import os
import subprocess

import numpy as np
import pytest

from bwams import bam, capi, merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -3, -6


# ---- the frontier rule: a record is (key, file, ordinal), so a wrong order or a lost record shows ----

def _cut(recs, sizes):
    """recs cut into pieces of the given sizes (0 allowed); what is left goes into a last piece"""
    out, p = [], 0
    for n in sizes:
        out.append(recs[p:p + n])
        p += n
    if p < len(recs):
        out.append(recs[p:])
    return out


def _file(k, keys):
    return [(key, k, i) for i, key in enumerate(sorted(keys))]


def _check(files):
    """files: piece lists.  The rounds concatenated are the merge; every round with an open child empties a window."""
    log = []
    pieces = merge.rounds(files, log=log)
    flat = [[r for p in f for r in p] for f in files]
    want = merge.merge_records(flat)
    got = [r for p in pieces for r in p]
    assert got == want
    assert want == sorted(r for f in flat for r in f)                   # (key, file, ordinal): rule M4 itself
    for is_open, before, emit in log:
        if any(is_open):
            assert any(o and b > 0 and e == b for o, b, e in zip(is_open, before, emit)), (is_open, before, emit)
    assert not any(log[-1][0]) and all(any(row[0]) for row in log[:-1])     # only the last round has no open child
    return pieces


def test_rounds_equal_the_merge_on_random_inputs():
    rng = np.random.default_rng(2026)
    for case in range(300):
        K = int(rng.choice([1, 2, 3, 7]))
        files = []
        for k in range(K):
            n = 0 if rng.random() < 0.15 else int(rng.integers(1, 25))             # empty files
            recs = _file(k, rng.integers(0, 4, n).tolist())                       # 4 distinct keys: ties dominate
            sizes = []
            while sum(sizes) < n:
                sizes.append(0 if rng.random() < 0.2 else int(rng.integers(1, 6)))  # empty pieces, pieces of 1 to 5
            if rng.random() < 0.3:
                sizes.append(0)                                                   # an empty last piece
            files.append(_cut(recs, sizes))                                       # an empty file: no piece, or empty ones
        _check(files)


NAMED = {
    "tie_run_longer_than_a_piece_in_the_lowest_file": [
        _cut(_file(0, [1] + [5] * 11 + [9]), [3, 3, 3, 3]), _cut(_file(1, [2, 5, 5, 7]), [2, 2]), _cut(_file(2, [5, 6]), [1, 1])],
    "tie_run_longer_than_a_piece_in_the_highest_file": [
        _cut(_file(0, [2, 5, 5, 7]), [2, 2]), _cut(_file(1, [5, 6]), [1, 1]), _cut(_file(2, [1] + [5] * 11 + [9]), [3, 3, 3, 3])],
    "tie_runs_in_two_files_at_once": [
        _cut(_file(0, [1] + [5] * 9 + [8]), [2, 2, 2, 2, 2]), _cut(_file(1, [5] * 10), [3, 3, 3]), _cut(_file(2, [4, 5, 6]), [1, 1, 1])],
    "all_records_of_one_key": [_cut(_file(0, [3] * 7), [2, 2, 2]), _cut(_file(1, [3] * 5), [4]), _cut(_file(2, [3] * 6), [1, 5])],
    "one_file_exhausted_early": [_cut(_file(0, [1, 1, 2]), [3]), _cut(_file(1, list(range(1, 20))), [4, 4, 4, 4]),
                                 _cut(_file(2, list(range(0, 30, 2))), [5, 5, 5])],
}


@pytest.mark.parametrize("case", sorted(NAMED))
def test_rounds_named_cases(case):
    pieces = _check(NAMED[case])
    if case.startswith("tie_run"):
        assert len(pieces) > 3                                          # the run crosses pieces and still moves on


def test_rounds_of_empty_input():
    assert merge.rounds([[], [[]], [[], []]]) == [[]]                   # one empty last piece
    assert merge.rounds([[[(1, 0, 0)]]]) == [[(1, 0, 0)]]               # K = 1, one piece: closed at once, emitted whole


# ---- the header merge ----

NAMES, LENS = [b"big", b"mid"], [9000, 200]
HD = b"@HD\tVN:1.6\tSO:coordinate\n"
SQ = b"@SQ\tSN:big\tLN:9000\n@SQ\tSN:mid\tLN:200\n"


def _block(text, names=NAMES, lens=LENS):
    return bam.header_block(text, names, lens)


def _rg(i, lib):
    return b"@RG\tID:%s\tLB:%s\tSM:s\n" % (i, lib)


HEADER_CASES = {
    "identical_files": ([HD + SQ + _rg(b"a", b"l1")] * 3, HD + SQ + _rg(b"a", b"l1"), 0),
    "rg_union": ([HD + SQ + _rg(b"a", b"l1"), HD + SQ + _rg(b"b", b"l1") + _rg(b"a", b"l1"), HD + SQ + _rg(b"c", b"l2")],
                 HD + SQ + _rg(b"a", b"l1") + _rg(b"b", b"l1") + _rg(b"c", b"l2"), 0),
    "pg_collision_dropped": ([HD + SQ + b"@PG\tID:bwa\tCL:lane1\n", HD + SQ + b"@PG\tID:bwa\tCL:lane2\n@PG\tID:sort\tPP:bwa\n",
                              b"@HD\tVN:1.0\n" + SQ + b"@PG\tID:bwa\tCL:lane3\n@PG\tID:sort\tPP:bwa\n"],
                             HD + SQ + b"@PG\tID:bwa\tCL:lane1\n@PG\tID:sort\tPP:bwa\n", 2),
    "co_kept_once": ([HD + SQ + b"@CO\tone\n@CO\ttwo\n", HD + SQ + b"@CO\ttwo\n@CO\tthree\n@CO\tone\n"],
                     HD + SQ + b"@CO\tone\n@CO\ttwo\n@CO\tthree\n", 0),
    "hd_and_sq_of_file_0_only": ([SQ + b"@CO\tx\n", HD + b"@SQ\tSN:big\tLN:9000\tM5:0\n@SQ\tSN:mid\tLN:200\n@CO\ty"],
                                 SQ + b"@CO\tx\n@CO\ty\n", 0),
    "nul_padding_and_no_text": ([b"", HD + SQ + b"@CO\tz\n\0\0\0"], b"@CO\tz\n", 0),
}


@pytest.mark.parametrize("case", sorted(HEADER_CASES))
def test_merge_header_cases(case):
    texts, want, dropped = HEADER_CASES[case]
    blocks = [_block(t) for t in texts]
    assert merge.merge_header(blocks) == (_block(want), dropped)
    capi.build()
    assert capi.bam_header_merge(blocks) == (_block(want), dropped)


def _refusals():
    two = [_block(HD + SQ + _rg(b"a", b"l1")), _block(HD + SQ + _rg(b"b", b"l1")), _block(HD + SQ + _rg(b"a", b"l2"))]
    return [
        (two, ERR_UNSUPPORTED, ["file 2", "@RG ID a", "file 0"]),
        ([_block(HD), _block(HD), _block(HD, NAMES, [9000, 201])], ERR_UNSUPPORTED, ["file 2", "reference 1", "length"]),
        ([_block(HD), _block(HD, [b"big", b"mix"], LENS)], ERR_UNSUPPORTED, ["file 1", "reference 1", "name"]),
        ([_block(HD), _block(HD, NAMES[:1], LENS[:1])], ERR_UNSUPPORTED, ["file 1", "1 references"]),
        ([_block(HD), b"BAM\2" + _block(HD)[4:]], ERR_ARG, ["magic"]),
        ([_block(HD)[:-1]], ERR_ARG, ["cut off"]),
        ([], ERR_ARG, ["1 to 64"]),
        ([_block(HD)] * 65, ERR_ARG, ["1 to 64"]),
    ]


def test_merge_header_refusals():
    capi.build()
    for blocks, code, parts in _refusals():
        with pytest.raises(merge.MergeRefusal) as e:
            merge.merge_header(blocks)
        assert e.value.code == code and all(p in str(e.value) for p in parts), str(e.value)
        with pytest.raises(capi.BwamsError) as e:
            capi.bam_header_merge(blocks)
        assert e.value.code == code and all(p in str(e.value) for p in parts), str(e.value)
    assert len(merge.merge_header([_block(HD)] * 64)[0]) == len(_block(HD))


def test_library_capacity_convention():
    import ctypes as C
    capi.build()
    blocks = [_block(HD + SQ)]
    ptr, sizes = (C.c_char_p * 1)(*blocks), (C.c_int64 * 1)(len(blocks[0]))
    n = C.c_int64(0)
    out = C.create_string_buffer(len(blocks[0]))
    assert capi.lib().bwams_bam_header_merge(ptr, sizes, 1, out, len(blocks[0]) - 1, C.byref(n), None) == -4 and n.value == len(blocks[0])
    assert capi.lib().bwams_bam_header_merge(ptr, sizes, 1, out, len(blocks[0]), C.byref(n), None) == 0 and out.raw == blocks[0]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hdrmerge") / "bam_header_merge_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "bam_merge_header.cpp"),
                           os.path.join(ROOT, "tools", "bam_header_merge_check.cpp"), "-o", exe])
    return exe


def _files(tmp_path, blocks):
    paths = []
    for k, b in enumerate(blocks):
        p = tmp_path / ("block%d" % k)
        p.write_bytes(b)
        paths.append(str(p))
    return paths


def test_host_program_under_sanitizers(program, tmp_path):
    for case, (texts, want, dropped) in sorted(HEADER_CASES.items()):
        out = tmp_path / "out"
        p = subprocess.run([program, str(out)] + _files(tmp_path, [_block(t) for t in texts]), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=60)
        assert p.returncode == 0, (case, p.stderr.decode())
        assert out.read_bytes() == _block(want) and p.stdout == b"pg_dropped %d\n" % dropped, case
    for blocks, code, parts in _refusals():
        if not 1 <= len(blocks) <= 64:
            continue
        p = subprocess.run([program, str(tmp_path / "out")] + _files(tmp_path, blocks), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        text = p.stderr.decode()
        assert p.returncode == 1 and text.startswith("%d: " % code) and all(x in text for x in parts), text


def test_truncated_block_is_an_error_return(program, tmp_path):
    texts = HEADER_CASES["pg_collision_dropped"][0]
    p = subprocess.run([program, "--truncations"] + _files(tmp_path, [_block(t) for t in texts]), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert p.returncode == 0, p.stderr.decode()                         # no sanitizer report at any length of any block
    assert p.stdout == b"", "lengths that merged: " + p.stdout.decode()
    whole = _block(texts[1])
    for n in range(len(whole)):                                         # the Python restatement refuses the same lengths
        with pytest.raises(merge.MergeRefusal) as e:
            merge.merge_header([_block(texts[0]), whole[:n]])
        assert e.value.code == ERR_ARG
