"""host/qc_text.cpp (rule 7's texts) built apart from the library with its own main (tools/qc_text_check.cpp) under
-fsanitize=address,undefined and run on the CPU; what it prints against the literal texts of tests/test_qc.py and bwams/qc.py."""
import os
import subprocess

import pytest

from bwams import qc
import test_qc as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qct") / "qc_text_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "qc_text.cpp"),
                           os.path.join(ROOT, "tools", "qc_text_check.cpp"), "-o", exe])
    return exe


def test_text(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    big = qc.Qc(max_cycle=64, max_isize=1 << 20)
    big.tables[qc.ISIZE][0, (1 << 20) - 1] = big.tables[qc.ISIZE][1, 1] = 1 << 40
    assert big.insert_size() == (1 << 41, 524288.0, 524287.0, 1)
    want = ("== hand flagstat\n" + T.HAND_FLAGSTAT + "== hand stats\n" + T.HAND_STATS + "== empty flagstat\n" + T.EMPTY_FLAGSTAT +
            "== empty stats\n" + T.EMPTY_STATS + "== big flagstat\n" + T.EMPTY_FLAGSTAT + "== big stats\n" + big.text(qc.TEXT_STATS))
    assert p.stdout.decode() == want
    assert T.hand().text(qc.TEXT_STATS) == T.HAND_STATS and qc.Qc().text(qc.TEXT_STATS) == T.EMPTY_STATS
