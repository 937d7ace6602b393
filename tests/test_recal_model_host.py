"""host/recal_model.cpp (the quality model) built apart from the library with its own main (tools/recal_model_check.cpp) under
-fsanitize=address,undefined and run on the CPU; what it prints against bwams/recal_apply.py over the tables of
tests/test_recal_model.py."""
import os
import subprocess

import numpy as np
import pytest

from bwams import recal
from bwams import recal_apply as A
import test_recal as T
import test_recal_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -3, -6


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rmc") / "recal_model_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "recal_model.cpp"),
                           os.path.join(ROOT, "tools", "recal_model_check.cpp"), "-o", exe])
    return exe


def text_of(tag: str, m: A.Model) -> str:
    rows = ["== %s\n" % tag]
    rows += ["RG %d %d %d %d\n" % ((g,) + tuple(r)) for g, r in enumerate(m.table(recal.RG).tolist())]
    rows += ["B %d %s\n" % (g, " ".join(str(v) for v in r)) for g, r in enumerate(m.table(recal.QUAL).tolist())]
    dc, dx = m.table(recal.CYCLE), m.table(recal.CONTEXT)
    rows += ["DC %d %d %d %d\n" % (g, q, c - m.max_cycle, dc[g, q, c]) for g, q, c in np.argwhere(dc != 0)]
    rows += ["DX %d %d %d %d\n" % (g, q, x, dx[g, q, x]) for g, q, x in np.argwhere(dx != 0)]
    return "".join(rows)


def test_model(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    want = "== constants\n" + "".join("S %d %d\n" % (k, A.S[k]) for k in range(1, 61)) + "".join("P %d %d\n" % (q, A.P[q]) for q in range(94))
    want += text_of("example", A.Model(T.example().tables, 10))
    want += text_of("zero", A.Model(M.zero_tables(1, 5), 5))
    want += text_of("extreme", A.Model(M.extreme_tables(), 3))
    want += text_of("two", A.Model(M.two_tables(), 4))
    want += text_of("two_opt", A.Model(M.two_tables(), 4, exclude=0x400, preserve_below=10, max_q=45, prior_obs=16))
    want += "== refused\n" + "".join("%s %d\n" % (k, ERR_UNSUPPORTED) for k in ("count", "errors", "negative"))
    want += "option %d\n" % ERR_ARG * 8 + "option 0\n"
    assert p.stdout.decode() == want
    assert "DC 0 30 6 -1\n" in want and "RG 0 60 0 -60\n" in want and "DC 1 93 -2 -93\n" in want and "RG 2 12 " in want
