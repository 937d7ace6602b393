"""Hand-made final regions for the tests of the paired-end tail (tests/test_gpu_pair_limits.py, tests/test_pair_cases.py):
mate rescue, mem_mark_primary_se, mem_reorder_primary5 and mem_pair of csrc/pair.hip at the list sizes where one kernel path
hands over to the next.

The setting is a random genome of 24 kb into which four mutated copies of one 150-base segment S are planted (2, 4, 6 and 8
substitutions: a read of S finds them with scores 140, 130, 120 and 110), once as a single sequence and once as three sequences
with the middle one ALT.  Reads 2p, 2p + 1 are the ends of pair p.  In a rescue pair the first end holds the anchors - regions
that only supply rb, re, rid and score, placed so that the FR window of each covers one copy - and the second end is S (or its
reverse complement) with N filler regions: score-descending as de-duplication leaves them, with reference spans of 8 bases on a
grid that keeps clear of every copy and of every anchor's insert-size range, so that the pairwise pass keeps them and no
orientation is consistent before the rescue, except where a case says otherwise.

`routes` restates what decides a read's way through the kernels from the inputs (pool capacity = regions + 4 per anchor of the
mate: pair_cap_kernel; kPostLight, kPostLds, the ERT variant's single form) and from the final region counts (kMarkLight and
the two pair_mark_wave_kernel instances); `planned` restates pair_plan_kernel (which orientations lack a consistent hit, the
window arithmetic of mem_matesw and the clip of bns_fetch_seq).  They are written from bwamem_pair.cpp and the constants of
pair.hip, not from oracle/pair_oracle.c; tests/test_pair_cases.py holds them against loader.pair_pe."""
import functools
import math

import numpy as np

from bwams import fmindex, simulate
from oracle import loader

POST_LIGHT, POST_LDS, RANK_MAX = 16, 1024, 96                  # pair.hip: kPostLight, kPostLds, kPostRankMax
MARK_LIGHT, MARK_SMALL, MARK_LDS = 24, 256, 2048               # kMarkLight, kMarkLdsSmall, kMarkLdsMax
L_PAC, SEG = 24000, 150
COPIES = ((3000, 0), (6000, 2), (11000, 4), (17000, 6), (21000, 8))      # (position, substitutions); the first is S itself
COPY_SCORE = tuple(SEG - 5 * k for _, k in COPIES)             # a = 1, b = 4: every substitution costs 5
BOUNDS = (9000, 15000)                                         # the three sequences: [0, 9000) [9000, 15000) ALT [15000, 24000)
ROUTE_KEYS = ("post_lane", "post_wave", "post_one_lane", "post_ert", "mark_lane", "mark_wave256", "mark_wave2048", "mark_one_lane")
REG_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "alt_sc", "csub", "sub_n", "w", "seedcov", "secondary",
              "secondary_all", "seedlen0", "n_comp_is_alt", "frac_rep", "hash", "flg")
PAIR_FIELDS = ("score", "sub", "n_sub", "z", "n_pri", "n_matesw")


def pes_of(low=100, high=500, avg=300.0, std=50.0, failed=(1, 0, 1, 1)):
    p = np.zeros(4, loader.PESTAT_DTYPE)
    p["low"], p["high"], p["avg"], p["std"], p["failed"] = low, high, avg, std, failed
    return p


PES_FR, PES_ALL = pes_of(), pes_of(failed=(0, 0, 0, 0))
PES_RF_FAILED = pes_of(failed=(0, 0, 1, 0))


@functools.lru_cache(maxsize=None)
def setting():
    """(genome with the copies planted, its index)."""
    g = simulate.make_genome(L_PAC, seed=17, repeat_frac=0.0).copy()
    s = g[COPIES[0][0]:COPIES[0][0] + SEG].copy()
    for i, (c, k) in enumerate(COPIES[1:], 1):
        t = s.copy()
        for j in range(k):
            t[20 + 13 * j + i] = (t[20 + 13 * j + i] + 1) & 3
        g[c:c + SEG] = t
    return g, fmindex.build_fmindex(g)


def contigs_of(alt):
    if not alt:
        return loader.single_contig(L_PAC)
    c = np.zeros(3, loader.CONTIG_DTYPE)
    c["offset"], c["len"], c["is_alt"] = [0, BOUNDS[0], BOUNDS[1]], [BOUNDS[0], BOUNDS[1] - BOUNDS[0], L_PAC - BOUNDS[1]], [0, 1, 0]
    return c


def rid_of(contigs, pos):
    f = pos if pos < L_PAC else 2 * L_PAC - 1 - pos
    return int(np.searchsorted(contigs["offset"], f, side="right") - 1)


@functools.lru_cache(maxsize=None)
def grid(clear=True):
    """Starts of the 8-base filler spans: every 10 bases on both strands, none across a sequence boundary or the strand junction;
    clear=True keeps away from the copies and from where an anchor of a copy has its insert-size range (either strand)."""
    ok = np.ones(2 * L_PAC, bool)
    for x in (0, L_PAC) + BOUNDS + tuple(2 * L_PAC - b for b in BOUNDS) + (2 * L_PAC,):
        ok[max(x - 12, 0):x + 12] = False
    if clear:
        for c, _ in COPIES:
            ok[c - 900:c + 1000] = False
            ok[2 * L_PAC - (c + 1000):2 * L_PAC - (c - 900)] = False
    return tuple(x for x in range(4, 2 * L_PAC - 12, 10) if ok[x:x + 8].all())


def reg(contigs, rb, re, qb, qe, score, alt=None, **fields):
    ar = np.zeros(1, loader.ALNREG_DTYPE)[0]
    ar["rb"], ar["re"], ar["qb"], ar["qe"], ar["score"] = rb, re, qb, qe, score
    ar["truesc"], ar["secondary"], ar["seedlen0"], ar["w"] = score, -1, 19, 100
    ar["seedcov"] = min(re - rb, qe - qb) >> 1
    ar["rid"] = rid_of(contigs, rb)
    is_alt = int(contigs["is_alt"][ar["rid"]]) if alt is None else alt
    ar["n_comp_is_alt"] = (is_alt << 30) | 1
    for k, v in fields.items():
        ar[k] = v
    return ar


class Cases:
    """Pairs of reads (code arrays) with their regions; tags[p] names pair p."""

    def __init__(self, alt=False, seed=1):
        self.alt, self.contigs = alt, contigs_of(alt)
        self.g = setting()[0]
        self.rng = np.random.default_rng(seed)
        self.reads, self.regs, self.tags = [], [], []

    def pair(self, read0, regs0, read1, regs1, tag):
        self.reads += [np.asarray(read0, np.uint8), np.asarray(read1, np.uint8)]
        self.regs += [list(regs0), list(regs1)]
        self.tags.append(tag)

    def extend(self, other):
        assert other.alt == self.alt
        self.reads += other.reads; self.regs += other.regs; self.tags += other.tags
        return self

    def flat(self):
        enc, cum = simulate.flatten_reads(self.reads) if self.reads else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
        regs = np.array([x for rs in self.regs for x in rs], loader.ALNREG_DTYPE) if any(self.regs) else np.zeros(0, loader.ALNREG_DTYPE)
        off = np.concatenate([[0], np.cumsum([len(rs) for rs in self.regs])]).astype(np.int64)
        return enc, cum, regs, off

    def tag_of_read(self, r):
        return self.tags[r >> 1]

    def acceptable(self):
        """What bwams_debug_pair_regs_upload asks of every region."""
        enc, cum, regs, off = self.flat()
        lens = np.repeat(np.diff(cum), np.diff(off))
        return bool(((regs["qb"] >= 0) & (regs["qb"] <= regs["qe"]) & (regs["qe"] <= lens) & (regs["rid"] >= 0) & (regs["rid"] < len(self.contigs))
                     & (regs["rb"] >= 0) & (regs["rb"] < regs["re"]) & (regs["re"] <= 2 * L_PAC) & (regs["score"] >= 0)).all())

    # ---- the parts of a rescue pair -------------------------------------------------------------------------------
    def anchor(self, c, strand, score, shift=0):
        """A region whose FR window covers the copy at c: 200 bases upstream of it on the strand given."""
        rb = c - 200 + shift if strand == 0 else 2 * L_PAC - (c + SEG) - 200 + shift
        return reg(self.contigs, rb, rb + SEG, 0, SEG, score)

    def qspan(self, L):
        """A query span: mostly short ones on a raster of 5 (many non-overlapping: the z list of the marking grows), some long."""
        k = int(self.rng.integers(0, 8))
        if k == 0:
            qb = int(self.rng.integers(0, L // 2)); return qb, int(self.rng.integers(qb + L // 3, L + 1))
        qb = 5 * int(self.rng.integers(0, (L - 12) // 5))
        return qb, qb + int(self.rng.choice([8, 10, 12]))

    def fillers(self, n, hi=0, L=SEG, eq=0, eq_score=COPY_SCORE[0], clear=True, alt_third=False, slots=None):
        """n regions, score-descending: `hi` of them score above any rescued region (30000, 29980, ...: only the first is
        within pen_unpaired of the best), `eq` score eq_score exactly, the rest 100 and then 70 downwards (again one anchor)."""
        if slots is None:
            slots = self.rng.choice(np.array(grid(clear)), size=n, replace=False)
        out = []
        for i, x in enumerate(slots):
            if i < hi:
                sc = 30000 - 20 * i
            elif i < hi + eq:
                sc = eq_score
            else:
                j = i - hi - eq
                sc = 100 if j == 0 else max(70 - j // 40, 20)
            qb, qe = self.qspan(L)
            a = reg(self.contigs, int(x), int(x) + 8, qb, qe, sc)
            if alt_third and i % 3 == 1:
                a["n_comp_is_alt"] |= 1 << 30
            out.append(a)
        return out

    def rescue_pair(self, tag, n, copies=(0,), strand=0, hi=0, eq=0, more_anchors=0, ties=0, swap=False, extra=(), eq_score=COPY_SCORE[0]):
        """Anchors at the copies named (scores 200, 199, ...), `more_anchors` further ones on grid places; the mate is S read from
        the other strand, with n fillers (+ `extra` regions, + `ties` pairs of fillers that share re, query span and score and are
        redundant with one another; swap: the two of each pair in the other order)."""
        s = self.g[COPIES[0][0]:COPIES[0][0] + SEG]
        anchors = [self.anchor(COPIES[ci][0], strand, 200 - j // 4, shift=j) for j, ci in enumerate(copies)]
        slots = self.rng.choice(np.array(grid(True)), size=n + ties + more_anchors, replace=False)     # distinct places for all
        for j in range(more_anchors):
            x = int(slots[n + ties + j])
            x = min(x, (L_PAC if x < L_PAC else 2 * L_PAC) - SEG)      # within its strand
            anchors.append(reg(self.contigs, x, x + SEG, 0, SEG, 200 - (len(copies) + j) // 4))
        fl = self.fillers(n, hi, eq=eq, eq_score=eq_score, slots=slots[:n])
        for t in range(ties):
            x = int(slots[n + t])
            pair = [reg(self.contigs, x, x + 8, 20, 60, 25, w=7), reg(self.contigs, x + 3, x + 8, 20, 60, 25, w=9)]
            fl += pair[::-1] if swap else pair
        fl += list(extra)
        fl.sort(key=lambda a: -int(a["score"]))               # stable: equal scores keep their order
        a0 = int(anchors[0]["rb"])
        read0 = np.concatenate([self.g, simulate.revcomp(self.g)])[a0:a0 + SEG]
        self.pair(read0, anchors, simulate.revcomp(s) if strand == 0 else s, fl, tag)


# ---- the restatement ------------------------------------------------------------------------------------------------
def infer_dir(b1, b2):                                         # bwamem_pair.cpp:57-65
    r1, r2 = b1 >= L_PAC, b2 >= L_PAC
    p2 = b2 if r1 == r2 else 2 * L_PAC - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def window(opt, contigs, pes, a_rb, a_rid, r4, l_ms):
    """mem_matesw's window of orientation r4 after bns_fetch_seq's clip -> (rb, re) or None when it is not aligned."""
    is_rev, is_larger = (r4 >> 1) != (r4 & 1), not (r4 >> 1)
    low, high = int(pes["low"][r4]), int(pes["high"][r4])
    if not is_rev:
        rb = a_rb + low if is_larger else a_rb - high
        re = (a_rb + high if is_larger else a_rb - low) + l_ms
    else:
        rb = (a_rb + low if is_larger else a_rb - high) - l_ms
        re = a_rb + high if is_larger else a_rb - low
    rb, re = max(rb, 0), min(re, 2 * L_PAC)
    if rb >= re:
        return None
    mid = (rb + re) >> 1
    rid = rid_of(contigs, mid)
    beg, end = int(contigs["offset"][rid]), int(contigs["offset"][rid]) + int(contigs["len"][rid])
    if mid >= L_PAC:
        beg, end = 2 * L_PAC - end, 2 * L_PAC - beg
    rb, re = max(rb, beg), min(re, end)
    return (rb, re) if rid == a_rid and re - rb >= opt.min_seed_len else None


def anchors_of(opt, regs, off, r):
    """Indices (within read r) of the regions that serve as anchors: within pen_unpaired of the best, at most max_matesw."""
    rs = regs[off[r]:off[r + 1]]
    return [j for j in range(len(rs)) if rs["score"][j] >= rs["score"][0] - opt.pen_unpaired][:opt.max_matesw]


def caps(opt, regs, off, no_rescue=False):
    """Per read its pool capacity (pair_cap_kernel): its regions, and room for four rescued ones per anchor of its mate (a run
    without rescue, a single-end run included, has no anchors)."""
    n = len(off) - 1
    return [int(off[r + 1] - off[r]) + (0 if no_rescue else 4 * len(anchors_of(opt, regs, off, r ^ 1))) for r in range(n)]


def planned(opt, contigs, pes, regs, off, cum, every=False):
    """Per read m: the windows pair_plan_kernel plans for the anchors of its mate against m's list as it is before any rescue
    (every=True: the second pass's plan, all orientations that have not failed)."""
    out = []
    for m in range(len(off) - 1):
        r, l_ms = m ^ 1, int(cum[m + 1] - cum[m])
        ws = []
        for j in anchors_of(opt, regs, off, r):
            a = regs[off[r] + j]
            skip = [bool(pes["failed"][k]) for k in range(4)]
            if not every:
                for i in range(off[m], off[m + 1]):
                    d, dist = infer_dir(int(a["rb"]), int(regs["rb"][i]))
                    if pes["low"][d] <= dist <= pes["high"][d]:
                        skip[d] = True
            ws += [(j, k, w) for k in range(4) if not skip[k] for w in [window(opt, contigs, pes, int(a["rb"]), int(a["rid"]), k, l_ms)] if w]
        out.append(ws)
    return out


def post_route(cap, use_ert):
    return "post_ert" if use_ert else "post_lane" if cap <= POST_LIGHT else "post_wave" if cap <= POST_LDS else "post_one_lane"


def mark_route(n_fin):
    return "mark_lane" if n_fin <= MARK_LIGHT else "mark_wave256" if n_fin <= MARK_SMALL else "mark_wave2048" if n_fin <= MARK_LDS else "mark_one_lane"


def routes(opt, regs, off, want_off, use_ert=False, redone=(), no_rescue=False):
    """What bwams_debug_pair_counts must say about the reads per route: every read once by its capacity, the reads in `redone`
    (those the second pass visits) once more; every read once by its final region count."""
    c = dict.fromkeys(ROUTE_KEYS, 0)
    cp = caps(opt, regs, off, no_rescue)
    for r in range(len(off) - 1):
        c[post_route(cp[r], use_ert)] += 1 + (r in redone)
        c[mark_route(int(want_off[r + 1] - want_off[r]))] += 1
    c["post_second"] = len(redone)
    return c


def insert_q(pes, want, want_off, pairs, opt):
    """The unrounded insert-size scores of every candidate of mem_pair (bwamem_pair.cpp:392-404) over the marked lists:
    pairs of primaries of different ends on one sequence whose distance lies within an orientation that has not failed."""
    qs = []
    for p in range(len(pairs)):
        xs = []
        for e in range(2):
            o = int(want_off[2 * p + e])
            for i in range(int(pairs["n_pri"][p][e])):
                rb, rid = int(want["rb"][o + i]), int(want["rid"][o + i])
                xs.append(((rid << 32) | (rb if rb < L_PAC else 2 * L_PAC - 1 - rb), int(rb >= L_PAC), e, int(want["score"][o + i])))
        if not xs or not pairs["n_pri"][p].all():
            continue
        xs.sort()
        x, st, en, sc = (np.array(v, np.int64) for v in zip(*xs))
        for d in range(1, len(xs)):
            dist = x[d:] - x[:-d]
            if dist.min() > max(int(h) for h in pes["high"]):
                break
            dr = st[:-d] << 1 | st[d:]                         # the earlier one's strand decides r, the later one's the low bit
            ok = (en[d:] != en[:-d]) & (pes["failed"][dr] == 0) & (dist >= pes["low"][dr]) & (dist <= pes["high"][dr])
            for i in np.flatnonzero(ok):
                ns = (float(dist[i]) - float(pes["avg"][dr[i]])) / float(pes["std"][dr[i]])
                qs.append(float(sc[i] + sc[i + d]) + .721 * math.log(2. * math.erfc(abs(ns) * 0.70710678118654752440)) * opt.a + .499)
    return np.array(qs)


# ---- rescue: the case files ---------------------------------------------------------------------------------------------
VARIANTS = tuple((ci, st) for ci in range(4) for st in (0, 1))      # copy x strand: eight reads per size


def capacity_cases(alt):
    """Capacity 16 | 17 and 1024 | 1025 around a one-anchor mate, lists of 0 and 1, and mates with 50 anchors of which six
    stand at copies; pairs whose second and last anchor stands where the first did (`idle`: consistent by then)."""
    c = Cases(alt, seed=11)
    for n in (0, 1, 12, 13, 1020, 1021):
        for ci, st in VARIANTS:
            c.rescue_pair("cap%d" % (n + 4), n, (ci,), st)
    for ci, st in VARIANTS:                                    # the second anchor finds the first one's region in place: it consumes nothing
        c.rescue_pair("idle_lane", 4, (ci, ci), st)
        c.rescue_pair("idle_wave", 30, (ci, ci), st)
    for ci, st in VARIANTS:
        c.rescue_pair("anchors50", 30, (ci, (ci + 1) % 5, (ci + 2) % 5, (ci + 3) % 5, (ci + 4) % 5, ci), st, more_anchors=44 + st)
    return c


def sort_cases(alt):
    """List lengths at the first sort (fillers + the rescued region) of 96 | 97 and around the network's paddings."""
    c = Cases(alt, seed=12)
    for n in (95, 96, 126, 127, 128, 511, 512, 1019):
        for ci, st in VARIANTS:
            c.rescue_pair("sort%d" % (n + 1), n, (ci, (ci + 1) % 4) if n < 1000 else (ci,), st)      # 1019 + 4: the last capacity in LDS
    return c


def insertion_cases(alt):
    """Where the rescued region goes: in front of everything with n = 64 and 128 (the shift moves whole chunks), behind
    everything, just before and after a multiple of 64, behind fillers of its own score."""
    c = Cases(alt, seed=13)
    for tag, n, hi, eq in (("at0_64", 64, 0, 0), ("at0_128", 128, 0, 0), ("atn_64", 64, 64, 0), ("atn_130", 130, 130, 0), ("at63", 130, 63, 0),
                           ("at64", 130, 64, 0), ("at65", 130, 65, 0), ("at127", 200, 127, 0), ("at128", 200, 128, 0), ("eq", 10, 5, 3), ("eq_wave", 130, 61, 3)):
        for ci, st in VARIANTS:
            c.rescue_pair(tag, n, (ci,), st, hi=hi, eq=eq, eq_score=COPY_SCORE[ci])
    return c


def tie_cases(alt, swap=False):
    """Fillers that share re (equal keys in the sort by end: lane 0's introsort decides), three pairs per read that are mutually
    redundant with equal scores, so that the order the introsort leaves them in decides which of each pair survives."""
    c = Cases(alt, seed=14)
    for tag, n in (("tie_rank", 40), ("tie_net", 200)):
        for ci, st in VARIANTS:
            c.rescue_pair(tag, n, (ci,), st, ties=3, swap=swap)
    return c


PES_NARROW = pes_of(low=300, high=400, avg=350.0, std=20.0)


def dedup_cases(alt):
    """Under a narrow insert-size range (300 .. 400; the rescued region lies at 349): a filler over the copy that starts outside
    the range and is redundant with the rescued region, winning (`filler_wins`) or losing (`rescued_wins`); a filler that shares
    the rescued region's end and starts far outside the range (`same_re`: the ERT variant's resort); a filler inside the range
    (`consistent`: no window is planned)."""
    c = Cases(alt, seed=15)
    for ci, st in VARIANTS:
        cp = COPIES[ci][0]
        b_rb, b_re = (2 * L_PAC - cp - SEG, 2 * L_PAC - cp) if st == 0 else (cp, cp + SEG)       # where the rescued region lands
        for tag, d, q, sc in (("filler_wins", 60, (0, SEG), 400), ("rescued_wins", 60, (0, SEG), 90), ("same_re", 300, (0, 5), 60),
                              ("consistent", 0, (0, SEG), 90)):
            c.rescue_pair(tag, 20, (ci,), st, extra=[reg(c.contigs, b_rb - d, b_re, q[0], q[1], sc)])
    return c


PES_WIDE = pes_of(low=200, high=500, avg=350.0, std=50.0, failed=(0, 0, 0, 0))


def window_cases(alt):
    """One anchor, an empty mate list, all four orientations with low = 200: anchors near coordinate 0, near 2 l_pac, on both sides
    of each sequence boundary and of the strand junction; a window clipped to min_seed_len bases and to one less."""
    c = Cases(alt, seed=16)
    s = c.g[COPIES[0][0]:COPIES[0][0] + SEG]
    spots = [("clip19_lo", 69), ("clip18_lo", 68), ("clip19_hi", 2 * L_PAC - 219), ("clip18_hi", 2 * L_PAC - 218)]
    for b in (0, L_PAC) + BOUNDS + tuple(2 * L_PAC - x for x in BOUNDS):
        spots += [("edge", b + d) for d in (-420, -260, -151, -30, 5, 120, 310)]
    for tag, rb in spots:
        rb = min(max(rb, 0), 2 * L_PAC - SEG)
        c.pair(s, [reg(c.contigs, rb, rb + SEG, 0, SEG, 100)], s, [], tag)
    return c


def matelen_cases(alt):
    """Mates of 249 and 250 bases (KSW_XBYTE set or not at a = 1) and of 512, each a stretch of the genome with a few
    substitutions, 200 bases downstream of its anchor."""
    c = Cases(alt, seed=17)
    ref2 = np.concatenate([c.g, simulate.revcomp(c.g)])
    for L in (249, 250, 512):
        for v in range(8):
            pos = (1000, 4000, 9800, 12000, 16000, 19000, 22000, 7000)[v] + (0 if v % 2 == 0 else L_PAC)
            m = ref2[pos:pos + L].copy()
            for j in range(v):
                m[30 + 17 * j] = (m[30 + 17 * j] + 1) & 3
            a = reg(c.contigs, pos - 200, pos - 50, 0, SEG, 100)
            far = [x for x in grid(True) if min(abs(x - (pos - 200)), abs(2 * L_PAC - 1 - x - (pos - 200))) > 1500]
            fl = [reg(c.contigs, int(x), int(x) + 8, *c.qspan(L), 90 - 20 * (i > 0) - i) for i, x in enumerate(c.rng.choice(np.array(far), size=20, replace=False))]
            c.pair(ref2[pos - 200:pos - 50], [a], simulate.revcomp(m), fl, "len%d" % L)
    return c


PES_LONG = pes_of(low=100, high=900, avg=500.0, std=100.0)
def fuzz_cases(alt, seed):
    """Some 200 reads whose list sizes are drawn around every limit of the rescue and of the marking, one to three anchors at
    copies drawn at random, the rescued regions landing anywhere in the list, some fillers of the rescued score, some tied pairs."""
    c = Cases(alt, seed=100 + seed)
    rng = np.random.default_rng(seed)
    for lo, hi, k in ((0, 30, 40), (85, 140, 24), (240, 270, 10), (500, 520, 10), (1008, 1023, 28)):
        for _ in range(k):
            n = int(rng.integers(lo, hi + 1))
            copies = tuple(int(x) for x in rng.choice(5, size=int(rng.integers(1, 4)), replace=False))
            c.rescue_pair("fuzz%d" % hi, n, copies, int(rng.integers(0, 2)), hi=int(rng.integers(0, n + 1)), eq=int(rng.integers(0, 3)) if n > 8 else 0,
                          eq_score=COPY_SCORE[copies[0]], ties=int(rng.integers(0, 3)))
    return c


RESCUE_FILES = {"capacity": capacity_cases, "sort": sort_cases, "insertion": insertion_cases, "tie": tie_cases, "dedup": dedup_cases,
                "window": window_cases, "matelen": matelen_cases}
RESCUE_PES = {"dedup": PES_NARROW, "window": PES_WIDE, "matelen": PES_LONG}


# ---- marking and mem_pair -------------------------------------------------------------------------------------------------
MARK_SIZES = (0, 1, 24, 25, 96, 97, 128, 129, 256, 257, 2048, 2049, 2600)
MARK_FORMS = ("pri", "mixed", "alt", "one_pri")


def mark_cases(alt=False):
    """Reads of every size in MARK_SIZES in four forms (all primary, ALT on a third, all ALT, exactly one primary), two more
    all-primary reads of 2049 and a 55th read of 300 regions: regions on the whole grid, both strands, runs of equal scores, query spans that overlap and that do
    not.  As a single-end chunk the read count is odd; as pairs (the first 54) reads 2p, 2p + 1 have the same size."""
    c = Cases(alt, seed=21)
    slots_all = np.array(grid(False))
    for n in MARK_SIZES + (2049, 300):
        for form in MARK_FORMS if len(c.reads) < 52 else ("pri", "pri") if n == 2049 else ("mixed",):
            slots = c.rng.choice(slots_all, size=n, replace=False)
            one = int(c.rng.integers(0, n)) if n else 0
            rs = []
            for i, x in enumerate(slots):
                qb, qe = c.qspan(SEG)
                is_alt = {"pri": 0, "mixed": int(i % 3 == 1), "alt": 1, "one_pri": int(i != one)}[form]
                rs.append(reg(c.contigs, int(x), int(x) + 8, qb, qe, max(120 - (i // 7) * (1 + i % 2), 20), alt=is_alt))
            rs.sort(key=lambda a: -int(a["score"]))
            c.reads.append(c.g[100:100 + SEG]); c.regs.append(rs)
            if len(c.reads) % 2 == 0:
                c.tags.append("mark%d" % n)
    c.tags.append("mark300")
    return c


def survivors(regs, off, want, want_off):
    """Per read: does every region given appear in the result (no filler was dropped)?  Then no orientation that was consistent
    when the first pass planned can have stopped being so, and no read needs the second pass."""
    out = []
    for r in range(len(off) - 1):
        have = {(int(a["rb"]), int(a["re"]), int(a["qb"])) for a in want[want_off[r]:want_off[r + 1]]}
        out.append(all((int(a["rb"]), int(a["re"]), int(a["qb"])) in have for a in regs[off[r]:off[r + 1]]))
    return out
