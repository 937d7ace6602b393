"""The plan of a region query on the CPU (include/bwams.h, "BAM file by region", rules 1 to 3): bwams/bai.py's plan walked over
the inflated file against brute force, on seeded random files with small BGZF blocks and on the named cases; bwams_bai_plan of the
library and host/bam_query.cpp built alone with its own main (tools/bai_plan_check.cpp) under -fsanitize=address,undefined give
the same intervals, and a BAI cut off at any length is an error return."""
import os
import subprocess

import numpy as np
import pytest

from bwams import bai, bam, capi
import bam_query_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def named():
    records = Q.named_records()
    assert Q.unique_names(records) and 280 <= len(bam.split_records(records)) <= 320
    data = Q.bam_file(records, 300)                                    # members of 300 bytes: most records straddle them
    raw = bai.build(data)
    return records, data, raw, bai.read(raw)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("baiplan") / "bai_plan_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "bam_query.cpp"),
                           os.path.join(ROOT, "tools", "bai_plan_check.cpp"), "-o", exe])
    return exe


def _disjoint(intervals):
    return all(b < e for b, e in intervals) and all(intervals[k][1] < intervals[k + 1][0] for k in range(len(intervals) - 1))


@pytest.mark.parametrize("seed,block", [(1, 300), (2, 777), (3, 4096), (4, 65280)])
def test_plan_against_brute_force(seed, block):
    rng = np.random.default_rng(seed)
    records = Q.encode(Q.background(rng, 400, unplaced=5, refs=(0, 1, 2)))
    assert Q.unique_names(records)
    data = Q.bam_file(records, block)
    idx = bai.read(bai.build(data))
    lists = [Q.random_regions(rng, int(rng.integers(1, 5))) for _ in range(60)] + [[(t, 0, Q.LENS[t])] for t in range(3)] + \
            [[(t, 0, Q.LENS[t]) for t in (2, 1, 0)]]
    for regions in lists:
        intervals = bai.plan(idx, regions)
        assert _disjoint(intervals), regions
        assert bai.walk(intervals, data, regions) == Q.brute(records, regions), regions
    got = bai.walk(bai.plan(idx, lists[-1]), data, lists[-1])
    assert len(got) == len(bam.split_records(records)) - 5             # every placed record, once


@pytest.mark.parametrize("case", sorted(Q.REGION_LISTS))
def test_named_cases(named, case):
    records, data, _, idx = named
    regions = Q.REGION_LISTS[case]
    intervals = bai.plan(idx, regions)
    assert _disjoint(intervals)
    got = bai.walk(intervals, data, regions)
    assert got == Q.brute(records, regions)
    names = {r[36:36 + r[12] - 1] for r in got}
    want_in = {"n_op_from_another_window": {b"n70k"}, "level1_bin": {b"lvl1"},
               "edges_and_placed_unmapped": {b"end_beg1", b"pos_end1", b"placed_unmapped"},
               "adjacent_pair": {b"end_eq_beg", b"end_beg1", b"pos_end1", b"placed_unmapped"},
               "reverse_order": {b"n70k", b"lvl1", b"end_beg1", b"pos_end1", b"placed_unmapped"},
               "overlapping_pair": {b"n70k"}}.get(case, set())
    assert want_in <= names
    if case == "edges_and_placed_unmapped":
        assert not names & {b"end_eq_beg", b"pos_end"}
    if case in ("behind_last_window", "reference_without_records", "keeps_none"):
        assert got == []
    if case == "reference_without_records":
        assert intervals == []
    if case == "behind_last_window":                                    # the window index is clamped to the last entry
        assert len(idx["refs"][1]["lin"]) <= 199000 >> 14


def test_merge_regions():
    assert bai.merge_regions([(1, 5000, 5100), (1, 4000, 5000), (0, 7, 9), (0, 8, 20), (0, 30, 31)]) == [(0, 7, 20), (0, 30, 31), (1, 4000, 5100)]


def test_library_plan_equals_python(named):
    _, _, raw, idx = named
    for case, regions in sorted(Q.REGION_LISTS.items()):
        assert capi.bai_plan(raw, regions) == bai.plan(idx, regions), case
    assert capi.bai_plan(raw, []) == []
    for bad in ([(3, 0, 10)], [(-1, 0, 10)], [(0, 10, 10)], [(0, -1, 10)]):
        with pytest.raises(capi.BwamsError) as e:
            capi.bai_plan(raw, bad)
        assert e.value.code == -3 and "bwams_bai_plan: region 0" in str(e.value)
    with pytest.raises(capi.BwamsError) as e:
        capi.bai_plan(raw[:-1], [Q.R_N])
    assert e.value.code == -2 and "cut off" in str(e.value)


def test_host_program_under_sanitizers(named, program, tmp_path):
    _, _, raw, idx = named
    p_bai = tmp_path / "named.bam.bai"
    p_bai.write_bytes(raw)
    rng = np.random.default_rng(5)
    lists = sorted(Q.REGION_LISTS.items()) + [("random%d" % k, Q.random_regions(rng, 4)) for k in range(5)]
    for case, regions in lists:
        p_reg = tmp_path / "regions.txt"
        p_reg.write_text("".join("%d %d %d\n" % g for g in regions))
        p = subprocess.run([program, str(p_bai), str(p_reg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 0, (case, p.stderr.decode())
        got = [tuple(int(x) for x in ln.split()) for ln in p.stdout.decode().splitlines()]
        assert got == bai.plan(idx, regions), case
    p_reg.write_text("3 0 10\n")                                        # a reference the index does not have
    p = subprocess.run([program, str(p_bai), str(p_reg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"region 0" in p.stderr


def test_truncated_bai_is_an_error_return(named, program, tmp_path):
    _, _, raw, _ = named
    p_bai = tmp_path / "named.bam.bai"
    p_bai.write_bytes(raw)
    p = subprocess.run([program, str(p_bai), "--truncations"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()                         # no sanitizer report at any of the len(raw) lengths
    assert p.stdout == b"", "lengths that parsed: " + p.stdout.decode()
    p_cut = tmp_path / "cut.bai"
    p_reg = tmp_path / "regions.txt"
    p_reg.write_text("0 100000 100200\n")
    for n in (0, 3, 8, len(raw) // 2, len(raw) - 8, len(raw) - 1):      # and through the program's ordinary path
        p_cut.write_bytes(raw[:n])
        p = subprocess.run([program, str(p_cut), str(p_reg)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and b"BAI" in p.stderr, (n, p.stderr.decode())
