"""host/depth_text.cpp (rule 11's three texts) built apart from the library with its own main (tools/depth_text_check.cpp) under
-fsanitize=address,undefined and run on the CPU; what it prints against the literal texts of tests/test_depth.py and bwams/depth.py."""
import os
import subprocess

import pytest

from bwams import depth
import test_depth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deptht") / "depth_text_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "depth_text.cpp"),
                           os.path.join(ROOT, "tools", "depth_text_check.cpp"), "-o", exe])
    return exe


def test_three_texts(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    hand = T.hand()
    want = ("== example summary\n" + T.EX_SUMMARY + "== example dist\n" + T.EX_DIST + "== example windows\n" + T.EX_WINDOWS_4 +
            "== hand summary\n" + T.TEXT_SUMMARY + "== hand dist\n" + hand.text(T.NAMES, depth.TEXT_DIST, 3) +
            "== hand windows\n" + T.TEXT_WINDOWS_8 +
            "== none summary\n" + "chrom\tlength\tbases\tmean\tmin\tmax\ntotal\t0\t0\t0.00\t0\t0\n" + "== none dist\n== none windows\n")
    assert p.stdout.decode() == want
    assert hand.text(T.NAMES, depth.TEXT_DIST, 3).startswith("total\t2\t0.2727\ntotal\t1\t0.5758\n")
