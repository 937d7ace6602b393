"""Reads for the trimming tests (test_trim.py on the restatement, test_gpu_trim.py on the device): one hand-computed case per rule
of bwams_fastq_trim, and simulated pairs / reads with a planted insert."""
import numpy as np

from bwams import trim

ADAPTER = b"AGATCGGAAGAGC"


def codes(s) -> np.ndarray:
    return np.array([b"ACGTN".index(c) for c in (s.encode() if isinstance(s, str) else bytes(s))], np.uint8)


def rc(c: np.ndarray) -> np.ndarray:
    r = np.asarray(c, np.uint8)[::-1]
    return np.where(r == 4, 4, 3 - r).astype(np.uint8)


def rd(seq, q=None, name=b"r", comment=None):
    """a read: seq a string or codes, q a list of Phred values (default 40 everywhere), False for none"""
    c = codes(seq) if isinstance(seq, (str, bytes)) else np.asarray(seq, np.uint8)
    if q is False:
        return (name, comment, c, None)
    q = np.full(len(c), 40) if q is None else np.asarray(q)
    assert len(q) == len(c)
    return (name, comment, c, (q + 33).astype(np.uint8))


def named(reads, paired=False, stem=b"t"):
    return [(stem + b"%d" % (i // 2 if paired else i),) + tuple(r[1:]) for i, r in enumerate(reads)]


def pair_of(rng, I, n1, n2, mism1=(), n_at1=(), n_at2=()):
    """the two ends of a random insert of I bases: end 1 its first n1 bases, end 2 the first n2 of its reverse complement, random
    bases behind an insert that is shorter; mism1 / n_at1: positions of end 1 changed to another base / to N; n_at2: of end 2"""
    F = rng.integers(0, 4, I).astype(np.uint8)
    a = np.concatenate([F, rng.integers(0, 4, max(0, n1 - I)).astype(np.uint8)])[:n1]
    b = np.concatenate([rc(F), rng.integers(0, 4, max(0, n2 - I)).astype(np.uint8)])[:n2]
    for p in mism1:
        a[p] = (a[p] + 1) % 4
    for p in n_at1:
        a[p] = 4
    for p in n_at2:
        b[p] = 4
    return [rd(a), rd(b)]


def hand_cases():
    """(name, reads, opt, paired, want): want[i] = (start, len, insert, reason) of read i, computed by hand from the rules"""
    I = trim.identity_opt
    K, L, N, Q, M = trim.KEPT, trim.LEN, trim.N, trim.QUAL, trim.MATE
    tail = I(cut_tail=1, cut_window=4, cut_quality=20)
    front = I(cut_front=1, cut_window=4, cut_quality=20)
    both = I(cut_front=1, cut_tail=1, cut_window=4, cut_quality=20)
    out = []

    def case(name, reads, opt, paired, want):
        out.append((name, named(reads, paired), opt, paired, want))

    # T1
    case("t1", [rd("ACGTACGTAC"), rd("ACGT"), rd("ACGTA")], I(trim_front=2, trim_tail=3), False, [(2, 5, 0, K), (2, 0, 0, L), (2, 0, 0, L)])
    # T2, cut_tail: w = min(4, n), a window passes at S >= 20 w
    case("t2_n_below_w", [rd("ACG", [30, 30, 10])], tail, False, [(0, 2, 0, K)])                 # w = 3: 70 >= 60 at e = 3; q[2] = 10 walks to 2
    case("t2_n_is_w_fails", [rd("ACGT", [20, 20, 20, 19])], tail, False, [(0, 0, 0, L)])          # 79 < 80: no window
    case("t2_sum_equal", [rd("ACGTAC", [25, 15, 25, 15, 0, 0])], tail, False, [(0, 3, 0, K)])     # e = 4: S = 80 passes; q[3] = 15 walks to 3
    case("t2_all_low", [rd("ACGTACGTAC", [5] * 10)], tail, False, [(0, 0, 0, L)])
    case("t2_all_high", [rd("ACGTACGTAC", [40] * 10)], tail, False, [(0, 10, 0, K)])
    case("t2_walk_one", [rd("ACGTACGTAC", [30] * 9 + [2])], tail, False, [(0, 9, 0, K)])          # e = 10 passes (92), the last base walks off
    case("t2_front_walk", [rd("ACGTACGT", [2] + [30] * 7)], front, False, [(1, 7, 0, K)])         # s = 0 passes (92), q[0] = 2 walks on
    case("t2_front_then_tail", [rd("ACGTACGT", [5, 5, 30, 30, 30, 30, 5, 5])], both, False, [(2, 4, 0, K)])
    case("t2_no_qualities", [rd("ACGTACGT", False)], both, False, [(0, 8, 0, K)])
    # T3 geometry
    rng = np.random.default_rng(11)
    ov = I(overlap=1)
    case("t3_below_both", pair_of(rng, 60, 100, 100), ov, True, [(0, 60, 60, K), (0, 60, 60, K)])
    case("t3_between", pair_of(rng, 100, 80, 120), ov, True, [(0, 80, 100, K), (0, 100, 100, K)])
    case("t3_above_both", pair_of(rng, 150, 100, 100), ov, True, [(0, 100, 150, K), (0, 100, 150, K)])
    # (AC)30 against (GT)30: every even I passes with no mismatch, up to 90 = n1 + n2 - overlap_min
    case("t3_repeat_takes_largest", [rd("AC" * 30), rd("GT" * 30)], ov, True, [(0, 60, 90, K), (0, 60, 90, K)])
    case("t3_max_diff", pair_of(rng, 100, 100, 100, mism1=(3, 20, 41, 77, 99)), ov, True, [(0, 100, 100, K), (0, 100, 100, K)])
    case("t3_max_diff_plus_one", pair_of(rng, 100, 100, 100, mism1=(3, 20, 41, 64, 77, 99)), ov, True, [(0, 100, 0, K), (0, 100, 0, K)])
    pct = I(overlap=1, overlap_diff_pct=10)                # ov = 30: 100 d <= 300
    case("t3_pct_binds_pass", pair_of(rng, 30, 100, 100, mism1=(0, 15, 29)), pct, True, [(0, 30, 30, K), (0, 30, 30, K)])
    case("t3_pct_binds_fail", pair_of(rng, 30, 100, 100, mism1=(0, 9, 15, 29)), pct, True, [(0, 100, 0, K), (0, 100, 0, K)])
    case("t3_n_counts_pass", pair_of(rng, 100, 100, 100, mism1=(1, 50, 98), n_at1=(10,), n_at2=(20,)), ov, True, [(0, 100, 100, K)] * 2)
    case("t3_n_counts_fail", pair_of(rng, 100, 100, 100, mism1=(1, 50, 70, 98), n_at1=(10,), n_at2=(20,)), ov, True, [(0, 100, 0, K)] * 2)
    # T4: adapter_min_match 4, one mismatch per 8 compared
    ad = I(adapter1=ADAPTER)
    case("t4_remnant_3_kept", [rd("T" * 36 + "AGA")], ad, False, [(0, 39, 0, K)])
    case("t4_remnant_4_cut", [rd("T" * 36 + "AGAT")], ad, False, [(0, 36, 0, K)])
    case("t4_cmp7_one_mismatch_kept", [rd("T" * 36 + "AGTTCGG")], ad, False, [(0, 43, 0, K)])
    case("t4_cmp8_one_mismatch_cut", [rd("T" * 36 + "AGTTCGGA")], ad, False, [(0, 36, 0, K)])
    case("t4_at_p0", [rd(ADAPTER.decode() + "T" * 10)], ad, False, [(0, 0, 0, L)])
    # T3 found an insert: T4 is not run on either end; no insert: adapter1 on end 1, adapter2 on end 2
    pa = I(overlap=1, adapter1=ADAPTER, adapter2=b"CCCCCCCC")
    F = rng.integers(0, 4, 100).astype(np.uint8)
    F[50:63] = codes(ADAPTER)                               # the insert itself spells the adapter
    case("t4_not_after_insert", [rd(F), rd(rc(F))], pa, True, [(0, 100, 100, K), (0, 100, 100, K)])
    case("t4_when_overlap_off", [rd(F), rd(rc(F))], I(adapter1=ADAPTER), True, [(0, 50, 0, K), (0, 100, 0, K)])
    # end 2 against adapter2: at p = 39 one G and seven C are compared with eight C, one mismatch in 8 passes
    case("t4_adapter2_for_end2", [rd("T" * 50 + ADAPTER.decode()), rd("G" * 40 + "CCCCCCCC")], pa, True, [(0, 50, 0, K), (0, 39, 0, K)])
    # T5
    case("t5", [rd("ACGTACGTAC"), rd("ACG")], I(max_len=4), False, [(0, 4, 0, K), (0, 3, 0, K)])
    # T6: the first filter that fails is the reason; the boundary of the quality filter (400 > 400 is false)
    flt = I(min_len=10, n_limit=2, qual_floor=15, low_qual_pct=40)
    case("t6_order", [rd("ACGNNNN", [2] * 7), rd("ACGTNNNACGTA", [2] * 12), rd("ACGTACGTACGT", [2] * 5 + [30] * 7),
                      rd("ACGTACGTAC", [14] * 4 + [15] * 6), rd("ACGTNNACGTAC")], flt, False,
         [(0, 7, 0, L), (0, 12, 0, N), (0, 12, 0, Q), (0, 10, 0, K), (0, 12, 0, K)])
    case("t6_mate", [rd("ACGTNNNACGTA"), rd("ACGTACGTACGT"), rd("ACGTACGTACGT"), rd("ACGTACG"), rd("ACGTACGTACGT"), rd("ACGTACGTACGA")],
         I(min_len=10, n_limit=2), True, [(0, 12, 0, N), (0, 12, 0, M), (0, 12, 0, M), (0, 7, 0, L), (0, 12, 0, K), (0, 12, 0, K)])
    return out


def sim_pair(rng, I, n1=150, n2=150, err=0.01, n_frac=0.0, tail_q=False, max_planted=None, adapters=(ADAPTER, b"AGATCGGAAGAGCGTCGTGTAGG")):
    """two ends of an insert of I bases with the adapters read through behind a short insert, errors at rate err (at most max_planted
    of them inside the overlap when given), N at rate n_frac, and (tail_q) quality falling along the read"""
    F = rng.integers(0, 4, I).astype(np.uint8)
    ends = []
    for k, n in enumerate((n1, n2)):
        src = F if k == 0 else rc(F)
        fill = np.concatenate([codes(adapters[k]), rng.integers(0, 4, n).astype(np.uint8)])
        ends.append(np.concatenate([src, fill])[:n].copy())
    a, b = ends
    lo, hi = max(0, I - n2), min(n1, I)
    e1 = np.nonzero(rng.random(n1) < err)[0]
    e2 = np.nonzero(rng.random(n2) < err)[0]
    if max_planted is not None:                          # errors inside the overlap, counted on end 1's axis
        in1 = [p for p in e1 if lo <= p < hi]
        in2 = [p for p in e2 if lo <= I - 1 - p < hi]
        keep = max_planted
        drop1, drop2 = in1[keep:], in2[max(0, keep - len(in1)):]
        e1 = np.array([p for p in e1 if p not in drop1], int)
        e2 = np.array([p for p in e2 if p not in drop2], int)
    for x, e in ((a, e1), (b, e2)):
        for p in e:
            x[p] = (x[p] + 1 + rng.integers(0, 3)) % 4
        x[rng.random(len(x)) < n_frac] = 4
    out = []
    for x in (a, b):
        if tail_q:
            q = np.clip(38 - (np.arange(len(x)) * 30 // max(len(x), 1)) * rng.integers(0, 2) + rng.integers(-6, 3, len(x)), 2, 41)
        else:
            q = np.full(len(x), 40)
        out.append(rd(x, q))
    return out


def bulk(seed, n_pairs, paired=True):
    """simulated reads for the bulk comparison: inserts 20..400, 1 % errors, falling tail quality, 2 % N, a tenth of them short"""
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(n_pairs):
        n1 = n2 = 150
        if rng.random() < 0.1:
            n1, n2 = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        p = sim_pair(rng, int(rng.integers(20, 401)), n1, n2, err=0.01, n_frac=0.02, tail_q=True)
        reads += p if paired else p[:1]
    return [(b"s%d" % (i // 2 if paired else i), b"c:%d" % i if i % 3 == 0 else None) + tuple(r[2:]) for i, r in enumerate(reads)]
