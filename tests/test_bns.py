"""CPU checks of bwams/bns.py, the restatement of bns_fasta2bntseq that the GPU FASTA indexer is compared with: the reference's
own .ann / .amb / .pac bytes (tests/golden/bns_cases.npz, written by tests/make_bns_golden.py) and glibc's srand48 / lrand48."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from bwams import bns

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "bns_cases.npz"))
CASES = sorted({k.split("/")[0] for k in GOLDEN.files})


@pytest.mark.parametrize("case", CASES)
def test_restatement_writes_the_reference_bytes(case):
    got = bns.fasta2bntseq(bytes(GOLDEN[case + "/fa"]))
    for ext in ("ann", "amb", "pac"):
        assert got[ext] == bytes(GOLDEN[case + "/" + ext]), ext


def test_golden_covers_every_rule():
    texts = {c: bytes(GOLDEN[c + "/fa"]) for c in CASES}
    allb = b"".join(texts.values())
    assert any(not t.startswith((b">", b"@")) for t in texts.values())                  # preamble junk
    assert any(b"\n@" in t or t.startswith(b"@") for t in texts.values())               # '@' headers
    for piece in (b"\t", b"\r\n", b"\n\r\n", b"\n\n", b"-", b" ", b"acgt", b"RY", b"NR"):
        assert piece in allb, piece
    assert {int(GOLDEN[c + "/pac"][-1]) for c in CASES} == {0, 1, 2, 3}                  # l_pac % 4
    assert any(b"0 0 0\n" in bytes(GOLDEN[c + "/ann"]) or b" 0 0\n" in bytes(GOLDEN[c + "/ann"]) for c in CASES)   # empty contigs


def test_issue_example():
    t = b"junk\n>chr1 first contig\nACGTNNNNacgtRYnnNNA\nCCGT\n>chr2\nNNNNGGGG\n\n>c3 x y\r\nAC\r\n\r\nGT\n>e\n>f\tt\nA-A A\n"
    r = bns.fasta2bntseq(t)
    assert r["ann"].replace(b"\n", b" | ").strip(b" |") == (b"40 5 11 | 0 chr1 first contig | 0 23 5 | 0 chr2 (null) | 23 8 1 | "
                                                             b"0 c3 x y | 31 4 0 | 0 e (null) | 35 0 0 | 0 f t | 35 5 2")
    assert r["pac"] == bytes.fromhex("1b6a1b04916f76a86c4c0000")


def test_refusals():
    with pytest.raises(bns.FastaError):
        bns.fasta2bntseq(b">r\nACGT\n+\nIIII\n")
    with pytest.raises(bns.FastaError):
        bns.fasta2bntseq(b"ACGT\nACGT\n")


def test_restored_annotations():
    assert bns.restored_annos([b"", b"x y", b"(null)"]) == [b"", b"x y", b""]


def _libc():
    libc = C.CDLL(None)
    libc.lrand48.restype = C.c_long
    libc.srand48.argtypes = [C.c_long]
    return libc


def test_lcg_equals_glibc_first_million_draws():
    libc = _libc()
    libc.srand48(11)
    n = 1_000_000
    want = np.fromiter((libc.lrand48() for _ in range(n)), np.int64, n)
    assert np.array_equal(bns.lrand48_draws(0, n), want)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_lcg_equals_glibc_far_from_the_seed(tmp_path):
    # glibc cannot jump: a small C helper draws sequentially up to each offset, ctypes calls it
    src = tmp_path / "far.c"
    src.write_text("#include <stdlib.h>\nlong far(long k) { srand48(11); long v = 0; for (long i = 0; i < k; ++i) v = lrand48(); return v; }\n")
    so = tmp_path / "libfar.so"
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", str(so), str(src)])
    far = C.CDLL(str(so)).far
    far.restype, far.argtypes = C.c_long, [C.c_long]
    for k in (1 << 24, 1 << 24 | 12345, 100_000_000):
        assert int(bns.lrand48_draws(k - 1, 1)[0]) == far(k), k
