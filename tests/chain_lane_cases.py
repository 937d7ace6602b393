"""Planted reads for the lane tier of the chaining stage (csrc/chain_lane.hip): reads of at most 32 seeds, which one lane chains
with the B-tree's root leaf in registers and the chain records in LDS for as long as the read has at most nine chains, and which
the same lane chains again through chain_dev.h's chain_read<false> when a tenth chain appears.  Built from tests/chain_cases.py's
blocks; tests/test_chain_lane_cases.py proves under the oracle alone that every case has the property it is built for, and
tests/test_gpu_chain_lane.py runs them through bwams_chain_run_ert.

`expect` maps a read's note to what the oracle must say about it: ("chains", n) chains before the filter, ("kept", n) chains
after it, ("seeds", n) seeds in its chains before the filter, ("repeat",) a chain position held twice."""
import functools

import numpy as np

import chain_cases as cc
from oracle import loader

LEAF_CHAINS = 9                                                  # KB_MAXK: keys of the B-tree's root while it is a leaf
FAR = cc.grid(480, room=480)                                     # positions further apart than any ladder here is long


class LaneCase(cc.Case):
    def __init__(self, name, reads, notes, expect, opts=None, contigs=None):
        super().__init__(name, reads, notes, opts, contigs)
        self.expect = expect


def lane_model(case):
    """(reads of the lane tier, those that give the leaf form up): at most 32 seeds, and among them more than nine chains
    before the filter — chains only ever get more, so a read reaches a tenth iff it ends with at least ten."""
    ns = cc.seeds_per_read(case)
    _, _, off = case.oracle(do_flt=False)
    nk = np.diff(off)
    lane = ns <= cc.LANE_SEEDS
    return int(lane.sum()), int((lane & (nk > LEAF_CHAINS)).sum())


def one(case, note):
    """The read `note` of the case as a batch of its own."""
    r = case.read(note)
    return LaneCase(case.name + "_" + note, [case.reads[r]], [note], {note: case.expect[note]} if note in case.expect else {}, case.opts, case.contigs)


SEED_COUNTS = (0, 1, 2, 9, 10, 31, 32, 33)


@functools.lru_cache(maxsize=None)
def seed_counts():
    """Reads of 0, 1, 2, 9, 10, 31 and 32 seeds over five base positions, a read whose only MEM has no hit, and one of 33 seeds,
    which a wavefront chains."""
    reads = [cc.ladder(FAR[10 * i:10 * i + 5], n) for i, n in enumerate(SEED_COUNTS)]
    notes = ["seeds%d" % n for n in SEED_COUNTS]
    reads.append([(0, 20, FAR[:0], "f")])
    notes.append("empty_mem")
    return LaneCase("seed_counts", reads, notes, {"seeds%d" % n: ("chains", min(n, 5)) for n in SEED_COUNTS})


@functools.lru_cache(maxsize=None)
def leaf_full():
    """Nine chains (the leaf full) and ten (given up at the tenth), from 10 seeds and from 32: in the latter three rows of a
    ladder have linked 27 seeds into nine chains before the last seeds come."""
    reads = [cc.singles(FAR[:9]) + [(cc.STEP, 19, FAR[:1] + cc.STEP, "f")],
             cc.singles(FAR[:10]),
             cc.ladder(FAR[20:29], 32),
             cc.ladder(FAR[40:49], 31) + [(100, 19, FAR[60:61], "f")]]
    notes = ["nine_of_10", "ten_of_10", "nine_of_32", "ten_of_32"]
    return LaneCase("leaf_full", reads, notes, dict(nine_of_10=("chains", 9), ten_of_10=("chains", 10), nine_of_32=("chains", 9), ten_of_32=("chains", 10)))


@functools.lru_cache(maxsize=None)
def equal_keys():
    """A second and a third chain at a position the leaf already holds (cc.repeat_of: the same position, too far off in the query to
    merge): in a leaf of five keys, and at the first, a middle and the last slot of a leaf that the repeat fills to nine, keys
    inserted in ascending, descending and random order."""
    rng = np.random.default_rng(21)
    reads, notes, expect = [], [], {}
    p5 = np.sort(FAR[100:105])
    reads.append(cc.singles(p5) + [cc.repeat_of(int(p5[2]))]); notes.append("two_same")
    reads.append(cc.singles(p5) + [cc.repeat_of(int(p5[2])), cc.repeat_of(int(p5[2]), qbeg=500)]); notes.append("three_same")
    p8 = np.sort(FAR[120:128])
    for how in ("asc", "desc", "rand"):
        for slot, at in (("first", 0), ("mid", 4), ("last", 7)):
            reads.append(cc.singles(cc.ordered(p8, how, rng)) + [cc.repeat_of(int(p8[at]))])
            notes.append("%s_%s" % (slot, how))
    reads.append(cc.singles(p8[:7]) + [cc.repeat_of(int(p8[3])), cc.repeat_of(int(p8[3]), qbeg=500)]); notes.append("three_same_full")
    for n in notes:
        expect[n] = ("repeat",)
    return LaneCase("equal_keys", reads, notes, expect)


@functools.lru_cache(maxsize=None)
def decisions():
    """test_and_merge's branches on three sequences, default options (w = 100): a contained seed; a seed on another sequence inside
    the band; a seed across two sequences (skipped); a seed at and beyond l_pac behind a forward-strand chain; x - y and y - x at
    w and w + 1."""
    c = np.zeros(3, loader.CONTIG_DTYPE)
    c["offset"], c["len"] = [0, cc.THREE[0], cc.THREE[1]], [cc.THREE[0], cc.THREE[1] - cc.THREE[0], cc.L_PAC - cc.THREE[1]]
    P, S0, LP = 20000, cc.THREE[0], cc.L_PAC
    at = lambda p: np.array([p], np.int64)
    reads = [[(0, 40, at(P), "f"), (10, 20, at(P + 10), "f")],
             [(0, 20, at(S0 - 25), "f"), (30, 20, at(S0 + 5), "f")],
             [(0, 20, at(P), "f"), (30, 20, at(S0 - 10), "f")],
             [(0, 20, at(LP - 40), "f"), (40, 20, at(LP), "f")],
             [(0, 20, at(LP - 40), "f"), (45, 20, at(LP + 5), "f")],
             [(0, 20, at(P), "f"), (200, 20, at(P + 100), "f")],
             [(0, 20, at(P), "f"), (200, 20, at(P + 99), "f")],
             [(0, 20, at(P), "f"), (200, 20, at(P + 300), "f")],
             [(0, 20, at(P), "f"), (200, 20, at(P + 301), "f")]]
    notes = ["contained", "other_seq", "two_seqs", "at_lpac", "beyond_lpac", "x_minus_y_w", "x_minus_y_w1", "y_minus_x_w", "y_minus_x_w1"]
    expect = dict(contained=("seeds", 1), other_seq=("chains", 2), two_seqs=("seeds", 1), at_lpac=("chains", 2), beyond_lpac=("chains", 2),
                  x_minus_y_w=("chains", 1), x_minus_y_w1=("chains", 2), y_minus_x_w=("chains", 1), y_minus_x_w1=("chains", 2))
    return LaneCase("decisions", reads, notes, expect, contigs=c)


GAP = 150


@functools.lru_cache(maxsize=None)
def gap_limits():
    """x - last_len and y - last_len at max_chain_gap - 1 (merged) and max_chain_gap (a chain of its own), max_chain_gap = 150."""
    P = 20000
    at = lambda p: np.array([p], np.int64)
    reads = [[(0, 20, at(P), "f"), (20 + GAP - 1, 20, at(P + 20 + GAP - 1), "f")],
             [(0, 20, at(P), "f"), (20 + GAP, 20, at(P + 20 + GAP), "f")],
             [(0, 20, at(P), "f"), (100, 20, at(P + 20 + GAP - 1), "f")],
             [(0, 20, at(P), "f"), (100, 20, at(P + 20 + GAP), "f")]]
    notes = ["both_below", "both_at", "y_below", "y_at"]
    return LaneCase("gap_limits", reads, notes, dict(both_below=("chains", 1), both_at=("chains", 2), y_below=("chains", 1), y_at=("chains", 2)),
                    dict(max_chain_gap=GAP))


@functools.lru_cache(maxsize=None)
def weight_floor(which):
    """Six one-seed chains of weights 19, 19, 20, 20, 21, 21 at query 0 and three of 30 at query 300: min_chain_weight drops all of
    them ("all": a_[0] stays), the four lightest ("some") or none ("none")."""
    reads = [cc.singles(FAR[200:206], per_mem=2) + [(300, 30, FAR[210:213], "f")], cc.singles(FAR[220:222])]
    opts = dict(all=dict(min_chain_weight=1000), some=dict(min_chain_weight=21), none={})[which]
    return LaneCase("weight_floor_" + which, reads, ["nine", "two"], {}, opts)


@functools.lru_cache(maxsize=None)
def overlaps():
    """Two one-seed chains inside the query span of a two-seed chain of weight wj, default options (drop_ratio 0.5, min_seed_len
    19).  The heavier of the two (45) is never dropped and becomes the dominant chain's first shadowed one (the filter keeps
    that one whatever its weight, which is why the lighter one is the one under test); the lighter, wi, is dropped iff
    wi < wj / 2 and wj - wi >= 38.  wi = 39 / 40 under wj = 80 are drop_ratio's two sides; wi = 36 under wj = 74 / 73 has the
    weight difference at 38 / 37."""
    at = lambda p: np.array([p], np.int64)
    P, Q, R = int(FAR[300]), int(FAR[310]), int(FAR[320])

    def trio(wj, wi):
        return [(100, 40, at(P), "f"), (140, wj - 40, at(P + 40), "f"), (100, 45, at(R), "f"), (101, wi, at(Q), "f")]
    reads = [trio(80, 39), trio(80, 40), trio(74, 36), trio(73, 36)]
    notes = ["ratio_below", "ratio_at", "diff_at", "diff_below"]
    return LaneCase("overlaps", reads, notes, dict(ratio_below=("kept", 2), ratio_at=("kept", 3), diff_at=("kept", 2), diff_below=("kept", 3)))


@functools.lru_cache(maxsize=None)
def tie_sort():
    """The filter's sort of three to nine chains: the weights McIlroy's adversary (cc.antiquicksort) fixes against ksort's
    median of three, nine equal weights, and blocks of three equal weights in three orders.  The chains share a query start, so
    they overlap, and which chain shadows which (`first`, the kept codes) follows the sort's tie order."""
    rng = np.random.default_rng(22)
    reads, notes = [], []
    for n in range(3, LEAF_CHAINS + 1):
        keys, _ = cc.antiquicksort(n)
        wts = 19 + (n - 1 - keys)
        b = np.sort(FAR[400:400 + n])
        reads.append([(0, int(wts[i]), b[i:i + 1], "f") for i in range(n)])
        notes.append("adversary%d" % n)
    b = np.sort(FAR[420:429])
    reads.append([(0, 19, rng.permutation(b), "f")]); notes.append("nine_equal")
    for k, how in enumerate(("asc", "desc", "rand")):
        p = cc.ordered(b, how, rng)
        order = (0, 1, 2) if k == 0 else (2, 1, 0) if k == 1 else (1, 2, 0)
        reads.append([(0, 19 + 6 * j, p[3 * j:3 * j + 3], "f") for j in order]); notes.append("blocks_" + how)
    # ... and under a dominant chain over the same span, which drops some of the tied ones: its first shadowed chain is the sort's choice
    reads.append([(0, 25, rng.permutation(b)[:8], "f")] + [(40 * k, 40, FAR[440:441] + 40 * k, "f") for k in range(3)]); notes.append("tied_under_dominant")
    return LaneCase("tie_sort", reads, notes, {})


def _mixed_reads(n, rng, wave_every=0):
    """n reads of 0 .. 32 seeds in shuffled order over one to ten base positions each (so a few reach a tenth chain), reads
    without a seed first, last and scattered; with wave_every, every such read has 33 .. 100 seeds instead."""
    cnt = rng.integers(1, cc.LANE_SEEDS + 1, size=n)
    cnt[[0, n - 1]] = 0
    cnt[rng.permutation(np.arange(1, n - 1))[:max(3, n // 10)]] = 0
    reads = []
    for i in range(n):
        c = int(cnt[i])
        if wave_every and i % wave_every == wave_every // 2 and 0 < i < n - 1:
            c = int(rng.integers(33, 101))
        k = int(rng.integers(1, 11)) if c <= cc.LANE_SEEDS else 40
        reads.append(cc.ladder(rng.permutation(FAR)[:min(max(c, 1), k)], c, order=("rand", "asc", "desc")[i % 3], rng=rng) if c else
                     ([] if i % 2 else [(0, 20, FAR[:0], "f")]))
    return reads, ["read%d" % i for i in range(n)]


@functools.lru_cache(maxsize=None)
def batch(n, wave_every=0):
    """63, 64, 65 and 200 reads: one wavefront short of a lane, full, one lane into the second, four blocks."""
    reads, notes = _mixed_reads(n, np.random.default_rng(300 + n + wave_every), wave_every)
    return LaneCase("batch%d%s" % (n, "_mixed" if wave_every else ""), reads, notes, {})


CASES = dict(seed_counts=seed_counts, leaf_full=leaf_full, equal_keys=equal_keys, decisions=decisions, gap_limits=gap_limits,
             overlaps=overlaps, tie_sort=tie_sort)
CASES.update({"weight_floor_" + w: (lambda w=w: weight_floor(w)) for w in ("all", "some", "none")})
CASES.update({"batch%d" % n: (lambda n=n: batch(n)) for n in (63, 64, 65, 200)})
CASES["batch200_mixed"] = lambda: batch(200, 7)
