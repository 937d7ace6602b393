"""Pin oracle/bsw_oracle.c to the REAL reference objects in oracle/_ref
(bandedSWA.cpp / ksw.cpp compiled from the reference tree, see oracle/Makefile; their stored answers where it is absent)."""
import ctypes as C

import numpy as np
import pytest

from oracle import loader
from ref_answers import Answers
from util import (BSW_SCORING_EDGES, BSW_WIDE_W, OUT_FIELDS, assert_pairs_equal, bsw_class_edge_tasks, bsw_n_run_tasks, bsw_score_limit_tasks,
                  bsw_scoring_edge_tasks, bsw_sw_opt, bsw_wide_band_tasks, make_pairs)

REF = loader.ref_lib()


@pytest.mark.parametrize("w", [100, 200, 7])
@pytest.mark.parametrize("end_bonus,zdrop", [(5, 100), (0, 0), (5, 20)])
def test_restatement_equals_reference_scalar(w, end_bonus, zdrop):
    pairs, ref, qer = make_pairs(600, seed=w + end_bonus + zdrop)
    opt = loader.default_sw_opt(end_bonus)
    opt.zdrop = zdrop
    ours, cells = loader.bsw_pairs(pairs, ref, qer, w, opt)
    theirs = Answers(REF is not None)(lambda: loader.ref_bsw(REF, "scalar", pairs, ref, qer, w, opt))
    assert_pairs_equal(ours, theirs, "scalar")
    assert cells > 0



def _outputs(p):
    return np.stack([p[f] for f in OUT_FIELDS], axis=1)


def _pin(tasks, w, opt):
    """the restatement equals scalarBandedSWA on these tasks (the answers are stored as the six output fields)"""
    pairs, ref, qer = tasks
    ours, _ = loader.bsw_pairs(pairs, ref, qer, w, opt)
    theirs = Answers(REF is not None)(lambda: _outputs(loader.ref_bsw(REF, "scalar", pairs, ref, qer, w, opt))).reshape(-1, len(OUT_FIELDS))
    bad = np.flatnonzero((_outputs(ours) != theirs).any(axis=1))
    assert bad.size == 0, f"{bad.size} tasks differ, first {pairs[bad[0]]}: ours {_outputs(ours)[bad[0]]}, reference {theirs[bad[0]]}"


# The edge families of tests/test_gpu_bsw.py: the GPU kernels are compared with the restatement on exactly these inputs.
@pytest.mark.parametrize("a", [1, 5])
def test_reference_scalar_at_the_score_limits(a):
    """scores up to 2^14 + 1 at every class edge, h0 up to 10^6, h0 = 0 and h0 < 0"""
    _pin(bsw_score_limit_tasks(a), 100, bsw_sw_opt(loader, a=a))


@pytest.mark.parametrize("w", [100, 5])
def test_reference_scalar_at_the_class_edges(w):
    _pin(bsw_class_edge_tasks(w), w, bsw_sw_opt(loader))


@pytest.mark.parametrize("w", BSW_WIDE_W)
def test_reference_scalar_in_wide_bands(w):
    _pin(bsw_wide_band_tasks(), w, bsw_sw_opt(loader))


def test_reference_scalar_with_runs_of_n():
    _pin(bsw_n_run_tasks(), 100, bsw_sw_opt(loader))


@pytest.mark.parametrize("a,gaps,n_score", BSW_SCORING_EDGES, ids=lambda v: str(v).replace(" ", ""))
def test_reference_scalar_at_the_scoring_edges(a, gaps, n_score):
    _pin(bsw_scoring_edge_tasks(a, seed=sum(gaps) + a), 100, bsw_sw_opt(loader, a=a, gaps=gaps, n_score=n_score))

def _ref_ksw_extend2(opt, q, t, w, h0):
    o = [C.c_int() for _ in range(5)]
    sc = REF.ref_ksw_extend2(C.byref(opt), len(q), q.ctypes.data, len(t), t.ctypes.data, w, h0, *[C.byref(x) for x in o])
    return sc, o[1].value, o[2].value, o[0].value, o[3].value, o[4].value


def test_restatement_equals_reference_ksw_extend2():
    """ksw_extend2 (ksw.cpp:432) is the routine the banded-SW spec descends from."""
    pairs, ref, qer = make_pairs(300, seed=99)
    opt = loader.default_sw_opt()
    ours, _ = loader.bsw_pairs(pairs, ref, qer, 100, opt)
    ans = Answers(REF is not None)
    for i, p in enumerate(pairs):
        q = np.ascontiguousarray(qer[p["idq"]: p["idq"] + p["len2"]])
        t = np.ascontiguousarray(ref[p["idr"]: p["idr"] + p["len1"]])
        got = tuple(int(x) for x in ans(lambda: _ref_ksw_extend2(opt, q, t, 100, int(p["h0"]))))
        want = tuple(int(ours[i][f]) for f in OUT_FIELDS)
        assert got == want, (i, got, want)


def test_reference_simd16_agrees_with_its_scalar_spec():
    """The reference's inter-task SIMD kernel and its scalar routine return the same six
    integers (SURVEY.md §8c measured 0 differing SAM lines across ISAs); this is why the
    scalar routine can serve as the specification for the HIP kernel."""
    pairs, ref, qer = make_pairs(512, seed=3)
    opt = loader.default_sw_opt()
    ans = Answers(REF is not None)
    a = ans(lambda: loader.ref_bsw(REF, "scalar", pairs, ref, qer, 100, opt))
    b = ans(lambda: loader.ref_bsw(REF, "vec16", pairs, ref, qer, 100, opt))
    same = np.ones(len(a), bool)
    for f in OUT_FIELDS:
        same &= a[f] == b[f]
    # the vector kernels are documented to follow the scalar semantics; report, do not hide, any drift
    assert same.mean() > 0.99, f"only {same.mean():.3f} of pairs agree between reference scalar and vec16"


def test_edge_cases_without_reference():
    opt = loader.default_sw_opt()
    from oracle.loader import SEQPAIR_DTYPE
    # identical sequences: score = h0 + len, reaches the query end
    q = np.array([0, 1, 2, 3] * 10, np.uint8)
    p = np.zeros(1, SEQPAIR_DTYPE)
    p["len1"], p["len2"], p["h0"] = len(q), len(q), 20
    out, cells = loader.bsw_pairs(p, q, q, 100, opt)
    assert out["score"][0] == 60 and out["qle"][0] == 40 and out["tle"][0] == 40
    assert out["gscore"][0] == 60 and out["gtle"][0] == 40 and out["max_off"][0] == 0
    # all-N target: nothing extends; score stays h0, ends at 0
    t = np.full(30, 4, np.uint8)
    out, _ = loader.bsw_pairs(p, t, q, 100, opt)
    assert out["score"][0] == 20 and out["qle"][0] == 0 and out["tle"][0] == 0
    # zero-length target
    p["len1"] = 0
    out, _ = loader.bsw_pairs(p, t, q, 100, opt)
    assert out["score"][0] == 20 and out["gscore"][0] == -1
