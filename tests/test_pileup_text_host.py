"""host/pileup_text.cpp (rule 9's text) built apart from the library with its own main (tools/pileup_text_check.cpp) under
-fsanitize=address,undefined and run on the CPU; what it prints against the literal texts of tests/test_pileup.py and bwams/pileup.py."""
import os
import subprocess

import pytest

from bwams import pileup
import test_pileup as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pileupt") / "pileup_text_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "pileup_text.cpp"),
                           os.path.join(ROOT, "tools", "pileup_text_check.cpp"), "-o", exe])
    return exe


def test_text(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    hand_last = "c1\t2\tC\t3\t0\t1\t1\t0\t0\t0\t0\t1\t0\t0\t1\tG,T,INS\n"
    assert p.stdout.decode() == "== example\n" + T.EX_TEXT + "== hand\n" + T.HAND_TEXT + hand_last + "== none\n" + pileup.TEXT_HEADER
    assert T.example().text(T.EX_NAMES) == T.EX_TEXT
    h = T.hand(min_alt=1, min_permille=300)
    h.set_ref(0, T.REF0[2:12])
    h.set_ref(2, [1])
    assert h.text(T.NAMES).startswith(T.HAND_TEXT) and h.text(T.NAMES).endswith(hand_last)
