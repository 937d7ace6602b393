"""bwams/recal_apply.py, the restatement of the quality model and of apply rules A to C (include/bwams.h above
bwams_recal_model_create): the two constant tables against their defining inequalities in Python's big integers, phred() against the
rounded logarithm, the header's worked example and the zero and extreme tables by literal values, every refusal with its record and
reason.  tests/test_recal_model_host.py and tests/test_gpu_recal_apply.py take their tables and records from here.

The header's example: record 1 (forward) holds cycle 6 at stored index 5, and DC[a][30][cycle 6] = -1, so rule C gives it 24 there
and 25 elsewhere; record 2 (reverse) holds cycle 6 at stored index 2, where the context AA takes another 1: 23."""
import math
import struct

import numpy as np
import pytest

from bwams import bam, recal
from bwams import recal_apply as A
import test_recal as T
from test_recal import rrec

MOST = (1 << 40) - 1


def zero_tables(n_rg: int, max_cycle: int):
    return recal.Recal([1], [b"g%d" % k for k in range(n_rg)] if n_rg else None, max_cycle=max_cycle).tables


def base(t, max_cycle, g, q, cyc, ctx, err):
    """one observed base in all four tables (ctx < 0: no context)"""
    add = np.array([1, err], np.int64)
    t[recal.RG][g] += add
    t[recal.QUAL][g, q] += add
    t[recal.CYCLE][g, q, cyc + max_cycle] += add
    if ctx >= 0:
        t[recal.CONTEXT][g, q, ctx] += add


def extreme_tables():
    """max_cycle 3, one read group and the row behind it: both clamps of rule C and both ends of a delta"""
    t = zero_tables(1, 3)
    t[recal.RG][0] = t[recal.QUAL][0, 60] = [MOST, MOST]                                 # a group of nothing but errors
    t[recal.CYCLE][0, 60, 3 + 1] = [MOST, 0]                                             # ... with one clean cycle: + 60
    t[recal.CYCLE][1, 50, 3 + 2] = t[recal.CONTEXT][1, 50, 5] = [MOST, 0]                # 50 + 10 + 10
    t[recal.CYCLE][1, 93, 3 - 2] = [MOST, MOST]                                          # - 93
    return t


def two_tables():
    """max_cycle 4, two read groups and the row behind them"""
    t = zero_tables(2, 4)
    for k in range(5000):
        base(t, 4, 0, 20, 1 + k % 4, k % 16, int(k % 50 == 0))
    for k in range(3000):
        base(t, 4, 1, 35, -(1 + k % 3), -1 if k % 7 == 0 else k % 16, int(k % 1000 == 0))
    for k in range(40):
        base(t, 4, 2, 12, 2, 3, int(k % 4 == 0))
    return t


def example_model(**opt) -> A.Model:
    return A.Model(T.example().tables, T.EX_OPT["max_cycle"], **opt)


def quals(data: bytes):
    """the QUAL bytes of every record of data"""
    out = []
    for r in bam.split_records(data):
        _, l_seq, _, at, _ = A._head(r)
        out.append(list(r[at:at + l_seq]))
    return out


def test_constants():
    assert len(A.S) == 61 and len(A.P) == 94
    for k in range(1, 61):
        bound = (1 << 320) * 10 ** (2 * k - 1)
        assert A.S[k] ** 20 <= bound < (A.S[k] + 1) ** 20
    for q in range(94):
        assert A.P[q] ** 10 * 10 ** q <= 1 << 400 < (A.P[q] + 1) ** 10 * 10 ** q
    assert (A.S[1], A.S[30], A.S[60]) == (73532, 58409021, 58409021481)
    assert (A.P[0], A.P[30], A.P[93]) == (1 << 40, 1099511627, 551)


def test_phred_is_the_rounded_logarithm():
    rng = np.random.default_rng(11)
    n = np.concatenate([rng.integers(0, 10 ** 12, 14000), rng.integers(0, 3000, 6000)])
    e = (n * rng.random(len(n)) ** 4).astype(np.int64)
    e[::7] = 0
    e[3::11] = n[3::11]
    for nn, ee in zip(n.tolist(), e.tolist()):
        want = min(60, math.floor(-10 * math.log10((ee + 1) / (nn + 2)) + 0.5))
        assert A.phred(ee + 1, nn + 2, 60) == want, (nn, ee)


def test_a_cell_without_data_keeps_its_prior():
    for m in (1, 1024, 1 << 20):
        for q in range(94):
            assert A.post(0, 0, q, m, 60) == min(q, 60)


def test_worked_example():
    m = example_model()
    assert m.table(recal.RG).tolist() == [[30, 27, -3], [-1, -1, 0]]                      # Qrep, QG, G of a; the row behind it
    b = m.table(recal.QUAL)
    assert (b[0, 30], b[0, 37], b[1, 30]) == (25, 34, 30)
    dc, dx = m.table(recal.CYCLE), m.table(recal.CONTEXT)
    assert dc[0, 30, 10 + 6] == -1 and np.count_nonzero(dc) == 1
    assert dx[0, 30, 0] == -1 and np.count_nonzero(dx) == 1                               # AA
    assert dc.dtype == np.int16 and dc.shape == (2, 94, 21) and dx.shape == (2, 94, 16) and b.shape == (2, 94)
    out, n = A.apply(b"".join(T.EX_RECS), m, [b"a"])
    assert n == 2 and quals(out) == [[25, 25, 25, 25, 25, 24, 25, 25], [25, 25, 23, 25, 25, 25, 25, 25]]
    mask = bytearray(b"".join(T.EX_RECS))                                                # nothing but QUAL bytes changes
    same = [x == y for x, y in zip(out, mask)]
    assert len(out) == len(mask) and same.count(False) == 16
    again, _ = A.apply(out, m, [b"a"])                                                   # not idempotent, and rule C says so
    assert again != out


def test_zero_tables():
    m = A.Model(zero_tables(0, 8), 8)
    assert m.table(recal.RG).tolist() == [[-1, -1, 0]] and m.table(recal.QUAL)[0].tolist() == list(range(94))
    assert not m.table(recal.CYCLE).any() and not m.table(recal.CONTEXT).any()
    q = [0, 5, 6, 7, 59, 60, 61, 200]
    out, n = A.apply(rrec(0, 0, "8M", "ACGTACGT", q), m)
    assert n == 1 and quals(out) == [[0, 5, 6, 7, 59, 60, 60, 60]]                        # below 6 kept; min(b, 93, max_q)
    out, _ = A.apply(rrec(0, 0, "3M", "ACG", [3, 50, 255]), A.Model(zero_tables(0, 8), 8, max_q=40, preserve_below=0))
    assert quals(out) == [[3, 40, 40]]
    out, _ = A.apply(rrec(0, 0, "2M", "AC", [0, 9]), A.Model(zero_tables(0, 8), 8, preserve_below=0))
    assert quals(out) == [[1, 9]]                                                        # a sum below 1 becomes 1


def test_clamps_and_delta_extremes():
    m = A.Model(extreme_tables(), 3)
    assert m.table(recal.RG).tolist() == [[60, 0, -60], [-1, -1, 0]]
    b, dc, dx = m.table(recal.QUAL), m.table(recal.CYCLE), m.table(recal.CONTEXT)
    assert b[0, 60] == 0 and b[0, :61].tolist() == [0] * 61 and b[0, 93] == 33 and b[1].tolist() == list(range(94))
    assert dc[0, 60, 3 + 1] == 60 and dc[1, 93, 3 - 2] == -93 and dc[1, 50, 3 + 2] == 10 and dx[1, 50, 5] == 10
    assert dc.min() == -93 and dc.max() == 60
    # group 0 (RG:Z:g0), forward: cycle 1 at q 60 gets 0 + 60; cycle 2 gets 0, which becomes 1
    out, _ = A.apply(rrec(0, 0, "2M", "AC", [60, 60], rg="g0"), m, [b"g0"])
    assert quals(out) == [[60, 1]]
    # the row behind it: q 50 at cycle 2 with the context CC = 5: 50 + 10 + 10 becomes 60
    out, _ = A.apply(rrec(0, 0, "3M", "CCC", [50, 50, 50]), m, [b"g0"])                  # cycle 3: 50 + 0 + 10
    assert quals(out) == [[50, 60, 60]]
    out, _ = A.apply(rrec(0, 0, "2M", "GG", [50, 50], flag=0x10), m, [b"g0"])            # reverse: cycles 2, 1; the machine read CC
    assert quals(out) == [[60, 50]]
    out, _ = A.apply(rrec(0, 0, "2M", "AA", [50, 50], flag=0x10), m, [b"g0"])            # the machine read TT: 50 + 10 + 0
    assert quals(out) == [[60, 50]]
    out, _ = A.apply(rrec(0, 0, "2M", "AC", [93, 200], flag=0x81), m, [b"g0"])           # cycles -1, -2: 93 - 93 becomes 1
    assert quals(out) == [[60, 1]]


def test_refused_tables_and_options():
    for cell in ([MOST + 1, 0], [3, 4], [3, -1], [-1, -1]):
        t = zero_tables(0, 2)
        t[recal.QUAL][0, 7] = cell
        with pytest.raises(A.ModelRefusal) as e:
            A.Model(t, 2)
        assert e.value.code == "unsupported"
    t = zero_tables(0, 2)
    t[recal.CONTEXT][0, 93, 15] = [MOST, MOST]
    A.Model(t, 2)
    for opt in (dict(exclude=0x10000), dict(preserve_below=-1), dict(preserve_below=94), dict(max_q=0), dict(max_q=61), dict(prior_obs=0),
                dict(prior_obs=(1 << 20) + 1), dict(reserved=1)):
        with pytest.raises(A.ModelRefusal) as e:
            A.Model(zero_tables(0, 2), 2, **opt)
        assert e.value.code == "arg"
    A.Model(zero_tables(0, 2), 2, exclude=0xFFFF, preserve_below=0, max_q=1, prior_obs=1 << 20)


GOOD = rrec(0, 5, "3M", "ACG", rg="a")


def refusals():
    """(tag, records, index of the refused record, reason, whether the model has read groups), each bad record behind good ones;
    the model is over max_cycle = 20"""
    short = bytearray(rrec(0, 5, "9M", "ACGTACGTA")[:-3])
    short[0:4] = struct.pack("<I", len(short) - 4)                                       # QUAL ends behind the record
    first = bytearray(rrec(0, 5, "9M", "ACGTACGTA", [0xFF] + [30] * 8)[:-3])             # ... before the look at its first byte
    first[0:4] = struct.pack("<I", len(first) - 4)
    out = [("bounds", bytes(short), "bounds", False),
           ("bounds_ff", bytes(first), "bounds", False),
           ("cycle", rrec(0, 5, "21M", "A" * 21), "cycle", False),
           ("cycle_unmapped", rrec(-1, -1, "", "A" * 21, flag=0x4), "cycle", False),     # MAPQ, refID and the CIGAR are not looked at
           ("aux", rrec(0, 5, "3M", "ACG", aux=b"XXq\0"), "aux", True),
           ("aux_z", rrec(0, 5, "3M", "ACG", rg="a", aux=b"XXZabc"), "aux", True)]
    return [(tag, GOOD * k + bad + GOOD, k, why, groups) for k, (tag, bad, why, groups) in enumerate(out, 1)]


@pytest.mark.parametrize("tag,data,at,why,groups", refusals(), ids=[r[0] for r in refusals()])
def test_refusals(tag, data, at, why, groups):
    m = A.Model(zero_tables(1 if groups else 0, 20), 20)
    before = bytes(data)
    with pytest.raises(A.ApplyRefusal) as e:
        A.apply(data, m, [b"a"] if groups else None)
    assert (e.value.record, e.value.why) == (at, why) and data == before
    if why == "aux":                                                                     # without read groups the aux fields are not read
        assert A.apply(data, A.Model(zero_tables(0, 20), 20))[1] == at + 2


def test_skipped_records_stay():
    m = A.Model(zero_tables(0, 20), 20, exclude=0x400)
    skipped = [rrec(0, 5, "4M", "ACGT", [0xFF, 30, 30, 30]), rrec(0, 5, "4M", "ACGT", 77, flag=0x400), rrec(0, 5, "2M", "", []),
               rrec(0, 5, "30M", "A" * 30, 77, flag=0x410)]                              # the last: excluded, so its length is not looked at
    data = b"".join(skipped)
    assert A.apply(data, m) == (data, 0)
    taken = [rrec(-1, -1, "", "ACGT", 77, flag=0x4), rrec(0, 5, "4M", "ACGT", 77, flag=0x100, mapq=0), rrec(0, 5, "4M", "ACGT", [77, 0xFF, 3, 6])]
    out, n = A.apply(b"".join(taken), m)                                                 # unmapped, secondary; 0xFF behind the first byte
    assert n == 3 and quals(out) == [[60] * 4, [60] * 4, [60, 60, 3, 6]]
