"""host/dup_metrics.cpp (the groups table, rule 14, the metrics text) built apart from the library with its own main
(tools/dup_metrics_check.cpp) under -fsanitize=address,undefined and run on the CPU; what it prints against bwams/markdup.py."""
import os
import subprocess

import pytest

from bwams import markdup
from test_markdup_metrics import GROUPS, GROUPS_REFUSED, SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dupm") / "dup_metrics_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "dup_metrics.cpp"),
                           os.path.join(ROOT, "tools", "dup_metrics_check.cpp"), "-o", exe])
    return exe


def run(exe, text: str, args=()):
    p = subprocess.run([exe, *map(str, args)], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode("latin-1")


def test_groups_sizes_and_text(program):
    args = [v for (n, c), _ in SIZES for v in (n, c)]
    for _, text, ids, _, libs in GROUPS:
        out = run(program, text, args)
        lines = out.split("\n")
        assert lines[0] == "groups 0"
        assert lines[1:1 + len(SIZES)] == ["size %d %d -> %d" % (n, c, -1 if v is None else v) for (n, c), v in SIZES]
        at = 1 + len(SIZES)
        assert lines[at] == "%d %d" % (len(ids), len(libs)) and lines[at + 1:at + 1 + len(libs)] == libs
        rows = []
        for k in range(len(libs)):
            r = dict.fromkeys(markdup.LIB_COUNTS, 0)
            if k % 2 == 0:
                r.update(unpaired_examined=7 + k, pairs_examined=1000 * (k + 1), secondary_or_supplementary=3, unmapped=11,
                         unpaired_duplicates=2, pair_duplicates=100 * (k + 1), pair_optical_duplicates=k)
            rows.append(markdup.finish_row(r))
        assert "\n".join(lines[at + 1 + len(libs):]) == markdup.metrics_text(markdup.groups(text), rows, "check")
    for _, text in GROUPS_REFUSED:
        assert run(program, text) == "groups -3\n"
    assert run(program, "") .startswith("groups 0\n0 1\nUnknown Library\n")
    assert run(program, "@RG\tID:a\tLB:x")[:len("groups 0\n1 2\nx\n")] == "groups 0\n1 2\nx\n"       # no newline at the end
