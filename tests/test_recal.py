"""bwams/recal.py, the numpy restatement of the base-recalibration rules (include/bwams.h above bwams_recal_open), against the worked
example of the header by literal values, against a planted truth that is written down in machine orientation and never goes through
recal.py's walk, and against the sum identities between the four tables; every refusal of rule 5 with its record and reason.
tests/test_gpu_recal.py and tests/test_recal_text_host.py take their records and expectations from here."""
import struct

import numpy as np
import pytest

from bwams import recal
from test_qc import qrec

HEADER = b"@HD\tVN:1.6\n@RG\tID:a\tLB:x\n"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rrec(refid, pos, cigar, seq, qual=30, flag=0, mapq=60, rg=None, aux: bytes = b"", name: bytes = b"r") -> bytes:
    """One BAM record: qual an int (every base) or a list or None (0xFF bytes); rg: an RG:Z field in front of `aux`."""
    n = len(seq)
    q = [qual] * n if isinstance(qual, int) else qual
    field = b"" if rg is None else b"RGZ" + (rg if isinstance(rg, bytes) else rg.encode()) + b"\0"
    return qrec(flag, refid, pos, mapq, -1, -1, 0, cigar, seq, q, aux=field + aux, name=name)


def codes_of(text: str) -> np.ndarray:
    return np.array(["ACGTN".index(c) for c in text], np.uint8)


# ---- the header's example ----
EX_REF = "ACGTACGT"
EX_RECS = [rrec(0, 0, "8M", "ACGTACGT", rg="a"), rrec(0, 0, "8M", "ACTTACGT", flag=0x10, rg="a")]
EX_OPT = dict(max_cycle=10)
EX_TEXT = ("RG\ta\t16\t1\n" "QUAL\ta\t30\t16\t1\n"
           "CYCLE\ta\t30\t1\t2\t0\n" "CYCLE\ta\t30\t2\t2\t0\n" "CYCLE\ta\t30\t3\t2\t0\n" "CYCLE\ta\t30\t4\t2\t0\n" "CYCLE\ta\t30\t5\t2\t0\n"
           "CYCLE\ta\t30\t6\t2\t1\n" "CYCLE\ta\t30\t7\t2\t0\n" "CYCLE\ta\t30\t8\t2\t0\n"
           "CONTEXT\ta\t30\tAA\t1\t1\n" "CONTEXT\ta\t30\tAC\t3\t0\n" "CONTEXT\ta\t30\tAG\t1\t0\n" "CONTEXT\ta\t30\tCG\t3\t0\n"
           "CONTEXT\ta\t30\tGT\t4\t0\n" "CONTEXT\ta\t30\tTA\t2\t0\n")
EX_TEXT_KNOWN = ("RG\ta\t14\t0\n" "QUAL\ta\t30\t14\t0\n"
                 "CYCLE\ta\t30\t1\t2\t0\n" "CYCLE\ta\t30\t2\t2\t0\n" "CYCLE\ta\t30\t3\t1\t0\n" "CYCLE\ta\t30\t4\t2\t0\n"
                 "CYCLE\ta\t30\t5\t2\t0\n" "CYCLE\ta\t30\t6\t1\t0\n" "CYCLE\ta\t30\t7\t2\t0\n" "CYCLE\ta\t30\t8\t2\t0\n"
                 "CONTEXT\ta\t30\tAC\t3\t0\n" "CONTEXT\ta\t30\tAG\t1\t0\n" "CONTEXT\ta\t30\tCG\t2\t0\n" "CONTEXT\ta\t30\tGT\t4\t0\n"
                 "CONTEXT\ta\t30\tTA\t2\t0\n")


def example(known: bool = False) -> recal.Recal:
    r = recal.Recal([8], [b"a"], **EX_OPT)
    r.set_ref(0, codes_of(EX_REF))
    if known:
        r.add_known([(0, 2, 3)])
    assert r.add(b"".join(EX_RECS)) == 2
    return r


def test_worked_example():
    r = example()
    assert r.table(recal.RG).tolist() == [[16, 1], [0, 0]]
    assert r.table(recal.QUAL)[0, 30].tolist() == [16, 1] and r.table(recal.QUAL).sum() == 17
    cyc = r.table(recal.CYCLE)
    assert cyc[0, 30, 10 + 6].tolist() == [2, 1] and cyc[0, 30, 11:19, 0].tolist() == [2] * 8 and cyc[..., 0].sum() == 16
    ctx = r.table(recal.CONTEXT)
    assert ctx[0, 30, 0].tolist() == [1, 1] and ctx[..., 0].sum() == 14                  # AA: record 2 reads ACGTAAGT on the machine
    assert cyc[..., 1].sum() == 1 and ctx[..., 1].sum() == 1                             # no other error anywhere
    assert cyc[:, :, 10].sum() == 0 and r.n_bases == 16                                  # the middle column stays 0
    assert r.text() == EX_TEXT
    k = example(known=True)
    assert k.table(recal.RG).tolist() == [[14, 0], [0, 0]] and k.table(recal.CYCLE)[0, 30, [13, 16], 0].tolist() == [1, 1]
    assert k.table(recal.CONTEXT)[0, 30, 0].tolist() == [0, 0] and k.text() == EX_TEXT_KNOWN
    r.reset()
    assert r.text() == "" and r.add(EX_RECS[0]) == 1 and r.table(recal.RG)[0].tolist() == [8, 0]      # the reference stayed


# ---- a planted truth, in machine orientation ----
def planted(seed: int = 5, n_reads: int = 400, length: int = 40, l_ref: int = 1500, max_cycle: int = 48):
    """-> (l_ref list, rg ids, reference codes, known intervals, records, expected tables, bases without a context).  Reads are
    error-free copies of a random reference but for planted mismatches; reads 0..5 carry an N; positions in `known` drop out.  The
    expectation is written in the machine's orientation: cycle = machine index + 1, context = the two machine bases."""
    rng = np.random.default_rng(seed)
    ref = "".join("ACGT"[k] for k in rng.integers(0, 4, l_ref))
    ids = [b"g0", b"g1"]
    known_pos = sorted(int(p) for p in rng.choice(l_ref, 25, replace=False))
    want = [np.zeros((3, 2), np.int64), np.zeros((3, 94, 2), np.int64), np.zeros((3, 94, 2 * max_cycle + 1, 2), np.int64),
            np.zeros((3, 94, 16, 2), np.int64)]
    recs, no_ctx = [], 0
    for k in range(n_reads):
        pos = int(rng.integers(0, l_ref - length))
        g = int(rng.integers(0, 3))                                                      # 2: no RG field
        q = int(rng.choice([7, 20, 30, 41]))
        rev, last = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        seq = list(ref[pos:pos + length])
        for i in rng.choice(length, int(rng.integers(0, 3)), replace=False):             # the planted mismatches
            seq[i] = "ACGT"[("ACGT".index(seq[i]) + int(rng.integers(1, 4))) % 4]
        if k < 6:
            seq[int(rng.integers(0, length))] = "N"
        seq = "".join(seq)
        flag = (0x10 if rev else 0) | (0x81 if last else 0x41)
        recs.append(rrec(0, pos, "%dM" % length, seq, q, flag=flag, rg=None if g == 2 else ids[g], name=b"p%d" % k))
        machine = "".join(COMP[c] for c in reversed(seq)) if rev else seq
        mref = "".join(COMP[c] for c in reversed(ref[pos:pos + length])) if rev else ref[pos:pos + length]
        for m in range(length):
            p = pos + (length - 1 - m if rev else m)
            if machine[m] == "N" or p in known_pos:
                continue
            add = np.array([1, machine[m] != mref[m]], np.int64)
            want[0][g] += add
            want[1][g, q] += add
            want[2][g, q, (-(m + 1) if last else m + 1) + max_cycle] += add
            if m > 0 and machine[m - 1] != "N":
                want[3][g, q, 4 * "ACGT".index(machine[m - 1]) + "ACGT".index(machine[m])] += add
            else:
                no_ctx += 1
    known = [(0, p, p + 1) for p in known_pos]
    return [l_ref], ids, codes_of(ref), known, recs, want, no_ctx


def test_planted_truth_and_sum_identities():
    l_ref, ids, ref, known, recs, want, no_ctx = planted()
    r = recal.Recal(l_ref, ids, max_cycle=48)
    r.set_ref(0, ref)
    r.add_known(known[10:])
    r.add_known(known[:12])                                                              # the union, overlapping
    assert r.add(b"".join(recs[:150])) == 150 and r.add(b"".join(recs[150:])) == len(recs) - 150
    for what in range(4):
        assert np.array_equal(r.table(what), want[what]), what
    assert want[0][:, 1].min() > 20 and want[3][..., 1].sum() > 100 and no_ctx > len(recs) // 2
    rg, qual, cyc, ctx = (r.table(k) for k in range(4))
    assert np.array_equal(qual.sum(1), rg) and np.array_equal(cyc.sum(2), qual)
    assert (ctx.sum(2) <= qual).all() and int((qual - ctx.sum(2))[..., 0].sum()) == no_ctx


# ---- rule 5 ----
GOOD = rrec(0, 5, "3M", "ACG", rg="a")


def refusals():
    """(tag, records, index of the refused record, reason, whether the handle needs a groups table), each bad record behind good ones;
    the handle is Recal([100], ..., max_cycle=20)"""
    short = bytearray(rrec(0, 5, "9M", "ACGTACGTA")[:-3])
    short[0:4] = struct.pack("<I", len(short) - 4)                                       # QUAL ends behind the record
    out = [("op", rrec(0, 5, [(3, 9)], "ACG", flag=0x400), "op", False),                 # op 9, in a record the filter would skip
           ("length", rrec(0, 5, "2M1D2I1S", "ACGT"), "length", False),                  # a query length of 5
           ("bounds", bytes(short), "bounds", False),
           ("cycle", rrec(0, 5, "21M", "A" * 21), "cycle", False),
           ("first", rrec(0, 5, [(2, 0), (1, 11)], "ACGT" * 6), "op", False),            # the op comes first
           ("aux", rrec(0, 5, "3M", "ACG", aux=b"XXq\0"), "aux", True),
           ("aux_z", rrec(0, 5, "3M", "ACG", rg="a", aux=b"XXZabc"), "aux", True)]
    return [(tag, GOOD * k + bad + GOOD, k, why, groups) for k, (tag, bad, why, groups) in enumerate(out, 1)]


@pytest.mark.parametrize("tag,data,at,why,groups", refusals(), ids=[r[0] for r in refusals()])
def test_refusals(tag, data, at, why, groups):
    r = recal.Recal([100], [b"a"] if groups else None, max_cycle=20)
    r.set_ref(0, np.zeros(100, np.uint8))
    with pytest.raises(recal.RecalRefusal) as e:
        r.add(data)
    assert (e.value.record, e.value.why) == (at, why)
    assert not any(t.any() for t in r.tables)                                            # nothing of the call is added
    if why == "aux":                                                                     # without a table the aux fields are not read
        assert recal.Recal([100], None, max_cycle=20).add(data) == at + 2


def test_skipped_not_refused():
    r = recal.Recal([100], None, max_cycle=20)
    r.set_ref(0, np.zeros(100, np.uint8))
    skipped = [rrec(0, 5, "2M", "ACGT", flag=0x4), rrec(0, 5, "2M", "ACGT", mapq=0), rrec(1, 5, "2M", "ACGT"), rrec(-1, 5, "2M", "ACGT"),
               rrec(0, 5, "", "ACGT"), rrec(0, 5, "2M", ""), rrec(0, 5, "3M", "ACGT", None), rrec(0, 5, "30M", "A" * 30, flag=0x100)]
    assert r.add(b"".join(skipped)) == 0 and not r.table(recal.RG).any()
    assert r.add(rrec(0, 5, "4M", "AAAA", flag=0x800)) == 1 and r.table(recal.RG)[0].tolist() == [4, 0]      # supplementary counts
