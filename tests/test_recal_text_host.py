"""host/recal_text.cpp (rule 10's text) built apart from the library with its own main (tools/recal_text_check.cpp) under
-fsanitize=address,undefined and run on the CPU; what it prints against the literal texts of tests/test_recal.py and bwams/recal.py."""
import os
import subprocess

import pytest

from bwams import recal
import test_recal as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rct") / "recal_text_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "recal_text.cpp"),
                           os.path.join(ROOT, "tools", "recal_text_check.cpp"), "-o", exe])
    return exe


def test_text(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    edges = recal.Recal([1], None, max_cycle=3)
    edges.tables[recal.RG][0] = [(1 << 40) + 6, (1 << 39) + 1]
    edges.tables[recal.QUAL][0, 0], edges.tables[recal.QUAL][0, 93] = [5, 0], [(1 << 40) + 1, (1 << 39) + 1]
    edges.tables[recal.CYCLE][0, 0, 0], edges.tables[recal.CYCLE][0, 93, 6], edges.tables[recal.CYCLE][0, 93, 2] = [5, 0], [1 << 40, 1 << 39], [1, 1]
    edges.tables[recal.CONTEXT][0, 0, 0], edges.tables[recal.CONTEXT][0, 93, 15] = [5, 0], [1 << 40, 1 << 39]
    edges_text = ("RG\t*\t1099511627782\t549755813889\n" "QUAL\t*\t0\t5\t0\n" "QUAL\t*\t93\t1099511627777\t549755813889\n"
                  "CYCLE\t*\t0\t-3\t5\t0\n" "CYCLE\t*\t93\t-1\t1\t1\n" "CYCLE\t*\t93\t3\t1099511627776\t549755813888\n"
                  "CONTEXT\t*\t0\tAA\t5\t0\n" "CONTEXT\t*\t93\tTT\t1099511627776\t549755813888\n")
    assert edges.text() == edges_text
    two_text = ("RG\tré2\t3\t2\n" "RG\t*\t1\t0\n" "QUAL\tré2\t6\t3\t2\n" "QUAL\t*\t7\t1\t0\n" "CYCLE\tré2\t6\t1\t3\t2\n"
                "CYCLE\t*\t7\t2\t1\t0\n" "CONTEXT\tré2\t6\tGC\t3\t2\n")
    want = "== hand\n" + T.EX_TEXT + "== empty\n" + "== edges\n" + edges_text + "== two\n" + two_text
    assert p.stdout.decode() == want
    assert T.example().text() == T.EX_TEXT and recal.Recal([5], [b"a", b"b"]).text() == ""
