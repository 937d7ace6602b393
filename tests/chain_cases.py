"""Planted seeds for the tests of the chaining stage (tests/test_gpu_chain_limits.py, tests/test_chain_cases.py): reads whose
MEMs and hit positions are written by hand and fed to bwams_chain_run_ert, at the seed counts, chain counts and sequence counts
where csrc/chain.hip hands a read from one kernel path to the next.

The setting is test_gpu_chain.py's 120 kb genome.  Chaining reads positions, query spans and the sequence table only, so a seed
may be put at any position of the doubled text; reads stay below 700 bases (mem_flt_chained_seeds, which does read bases,
starts at 5.5 ln L <= 0.05 L) except where a case says otherwise.  A read is a list of MEMs `(qbeg, len, positions, how)`; `how`
is "f" (forward = 1: the hit is the position), "b" (found by backward search: the hit is the reverse-complemented match's
position off by an end_correction, mem_chain_new maps it back) or "l" (fetch_leaves = 1).

Two building blocks make the chain count of a read exact whatever the options:
  * seeds of one query start never merge when their positions are more than `w` apart (x = 0, y > w in test_and_merge) and never
    contain each other when the positions differ: one chain per position;
  * MEM k of a "ladder" starts at query k * STEP and hits every base position + k * STEP: seed k extends the chain of its base
    position (x = y = STEP) as long as the base positions are further apart than the ladder is long.

`model` restates what decides a read's way through the kernels — the constants below are copied from the chaining sources
(chain_dev.h, chain_wave.h, chain.hip), and test_chain_cases.py checks that those still hold them, each in one file — from the
inputs (seeds per read after mem_chain_new's stride pick) and from the oracle's chains before the filter (loader.chain_new_ert(do_flt=False): chains per read, repeated positions, and
mem_chain_weight restated here).  It is written from the order of tests at the end of chain_read and in chain_heavy_kernel."""
import functools
import re

import numpy as np

from bwams import fmindex, simulate
from oracle import loader

L_PAC = 120000
LANE_SEEDS = 32                                                # kLaneSeeds: more seeds than this -> a wave per read
LDS_CLASSES = (128, 256, 512, 665, 850, 1275, 1700)            # kClassS, M1, M, M2, L1, L2, L: chain records + ordered array in LDS
CLASS_XL, CLASS_XL2 = 4096, 13000                              # kClassXL, kClassXL2: the ordered array only; beyond: B-tree in HBM
CLASS_ORDER = (1700, 850, 512, 256, 128, 32, 4096, 1275, 665, 13000)      # chain_count_kernel's thr[]: counts[0 .. 9]
LIGHT_CHAINS = 16                                              # kLightChains: more chains than this -> chain_heavy_kernel
HEAVY_CAP = (64, 128, 256, 512, 960, 3840)                     # kHeavyCap: beyond the last, the sequential form
HIST_EDGES = (32, 64, 128, 256, 512, 960)                      # heavy_read's size histogram
REC_BYTES, ARR_BYTES, FLT_BYTES = 48, 12, 41                   # sizeof(ChainRec), ordered-array entry, filter bytes per chain
SOURCE_CONSTANTS = (
    r"constexpr int kLaneSeeds = 32;", r"constexpr int kLightChains = 16;",
    r"constexpr int kClassS = 128, kClassM1 = 256, kClassM = 512, kClassL1 = 850, kClassL = 1700;",
    r"constexpr int kClassM2 = 665, kClassL2 = 1275;", r"constexpr int kClassXL = 4096;", r"constexpr int kClassXL2 = 13000;",
    r"const int thr\[10\] = \{kClassL, kClassL1, kClassM, kClassM1, kClassS, kLaneSeeds, kClassXL, kClassL2, kClassM2, kClassXL2\};",
    r"constexpr int kHeavyCap\[6\] = \{64, 128, 256, 512, 960, 3840\};",
    r"static_assert\(sizeof\(ChainRec\) == 48,", r"return \(size_t\)K \* \(sizeof\(ChainRec\) \+ 12\) \+ 64;",
    r"lds_bytes_xl\(int K\) \{ return \(size_t\)K \* 12 \+ 64; \}", r"const int cap_f = \(int\)\(\(bytes - 64\) / 41\);",
    r"heavy_lds_bytes\(int cap\) \{ return \(size_t\)cap \* 41 \+ 64; \}",
    r"n_chn <= 32 \? 0 : n_chn <= 64 \? 1 : n_chn <= 128 \? 2 : n_chn <= 256 \? 3 : n_chn <= 512 \? 4 : n_chn <= 960 \? 5 : 6;",
    r"if \(n_chn > kLightChains\) \{", r"if \(__popcll\(__ballot\(com\)\) <= 1\) one_by_one = 8;",
)
STEP = 16                                                      # a ladder's step in the query and in the reference
COUNT_KEYS = ("gt_L", "gt_L1", "gt_M", "gt_M1", "gt_S", "gt_lane", "gt_XL", "gt_L2", "gt_M2", "gt_XL2", "n_heavy", "redo",
              "flt32", "flt64", "flt128", "flt256", "flt512", "flt960", "flt_more", "flt_seq", "in_wave", "lane_seq")


def missing_constants(text):
    """The entries of SOURCE_CONSTANTS that `text` (the chaining sources' text) does not hold."""
    return [c for c in SOURCE_CONSTANTS if not re.search(c, text)]


@functools.lru_cache(maxsize=None)
def setting():
    """(genome, its FM-index): the repeat-rich toy of test_gpu_chain.py."""
    g = simulate.make_genome(L_PAC, seed=31, repeat_frac=0.45, repeat_len=260, n_families=4)
    return g, fmindex.build_fmindex(g)


def mem_opts(**kw):
    """(oracle's, library's) mem_opt_t with the same fields changed."""
    from bwams import capi
    o, g = loader.default_mem_opt(), capi.default_mem_opt()
    for k, v in kw.items():
        setattr(o, k, v)
        setattr(g, k, v)
    return o, g


def grid(spacing, room=64, first=0):
    """Every position first + k * spacing of the doubled text at which a seed of up to `room` bases lies on one strand."""
    p = np.arange(first, 2 * L_PAC - room, spacing, dtype=np.int64)
    return p[(p + room <= L_PAC) | (p >= L_PAC)]


def ordered(pos, how, rng):
    pos = np.sort(np.asarray(pos, np.int64))
    return pos if how == "asc" else pos[::-1].copy() if how == "desc" else rng.permutation(pos)


def singles(pos, qbeg=0, len0=19, per_mem=500, how="f"):
    """MEMs of one query start over `pos` in the given order, `per_mem` hits each, lengths len0, len0 + 1, ..: a chain per position
    (positions more than w apart)."""
    return [(qbeg, len0 + k, pos[i:i + per_mem], how) for k, i in enumerate(range(0, len(pos), per_mem))]


def ladder(base, n_seeds, len0=19, how="f", order="asc", rng=None):
    """n_seeds seeds over the base positions: MEM k (query k * STEP) hits base + k * STEP, the last MEM only the first few bases.
    One chain per base position touched; the bases must be more than (MEMs) * STEP apart."""
    base = np.asarray(base, np.int64)
    out, k = [], 0
    while n_seeds > 0:
        m = min(n_seeds, len(base))
        out.append((k * STEP, len0, ordered(base[:m] + k * STEP, order, rng), how))
        n_seeds -= m
        k += 1
    return out


def repeat_of(pos, qbeg=300, length=19):
    """One more seed AT a held position, too far off in the query to merge or be contained: a second chain at that position."""
    return (qbeg, length, np.array([pos], np.int64), "f")


class Case:
    """A batch: reads (lists of MEMs), their lengths, options, the sequence table (None = one sequence) and what each read is for."""

    def __init__(self, name, reads, notes, opts=None, contigs=None, read_len=640, seed=1):
        self.name, self.reads, self.notes, self.opts, self.contigs = name, reads, notes, dict(opts or {}), contigs
        self.lens = [read_len] * len(reads) if np.isscalar(read_len) else list(read_len)
        assert len(notes) == len(reads) == len(self.lens)
        rng = np.random.default_rng(seed)
        mems, hits, mem_off, hit_off = [], [], [0], [0]
        for rd in reads:
            hb = 0
            for j, (qbeg, length, pos, how) in enumerate(rd):
                pos = np.asarray(pos, np.int64)
                m = np.zeros(1, loader.ERT_MEM_DTYPE)[0]
                m["start"], m["end"], m["hitbeg"], m["hitcount"] = qbeg, qbeg + length, hb, len(pos)
                if how == "b":
                    m["forward"], m["end_correction"] = 0, (j % 4)
                    pos = 2 * L_PAC - pos - length + (j % 4)
                    assert (pos >= 0).all()
                elif how == "l":
                    m["forward"], m["fetch_leaves"] = 0, 1
                else:
                    m["forward"] = 1
                mems.append(m)
                hits.append(pos.astype(np.uint64))
                hb += len(pos)
            mem_off.append(len(mems))
            hit_off.append(hit_off[-1] + hb)
        self.mems = np.array(mems, dtype=loader.ERT_MEM_DTYPE) if mems else np.zeros(0, loader.ERT_MEM_DTYPE)
        self.hits = np.concatenate(hits) if hits else np.zeros(0, np.uint64)
        self.mem_off, self.hit_off = np.array(mem_off, np.int64), np.array(hit_off, np.int64)
        self.enc = rng.integers(0, 4, size=int(sum(self.lens)), dtype=np.uint8)
        self.cum = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)

    def read(self, note):
        """Index of the read with this note."""
        return self.notes.index(note)

    def oracle(self, do_flt=True, **kw):
        """(chains, seeds, chain_off) of loader.chain_new_ert under the case's options (kw overrides)."""
        g, _ = setting()
        oopt, _ = mem_opts(**{**self.opts, **kw})
        ref = np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])
        return loader.chain_new_ert(self.mems, self.mem_off, self.hits, self.hit_off, self.cum, L_PAC, contigs=self.contigs, opt=oopt,
                                    do_flt=do_flt, ref_string=ref, enc=self.enc)

    def with_read(self, r, mems):
        """The case with read r replaced (the perturbation tests)."""
        reads = list(self.reads)
        reads[r] = mems
        return Case(self.name, reads, self.notes, self.opts, self.contigs, self.lens)


# ---- the route model ------------------------------------------------------------------------------------------------------------

def seeds_per_read(case):
    """Seeds as chain_count_kernel counts them: mem_chain_new's pick k = 0, step, .. (at most max_occ) of every MEM, skipped ones included."""
    max_occ = mem_opts(**case.opts)[0].max_occ
    hc = case.mems["hitcount"].astype(np.int64)
    step = np.where(hc > max_occ, hc // max_occ, 1)
    picks = np.minimum((hc + step - 1) // step, max_occ)
    c = np.concatenate([[0], np.cumsum(picks)])
    return c[case.mem_off[1:]] - c[case.mem_off[:-1]]


def tier_of(n_seeds):
    """("lane" | "lds" | "xl" | "hbm", the class's seed capacity)."""
    if n_seeds <= LANE_SEEDS:
        return "lane", 0
    for k in LDS_CLASSES:
        if n_seeds <= k:
            return "lds", k
    if n_seeds <= CLASS_XL:
        return "xl", CLASS_XL
    if n_seeds <= CLASS_XL2:
        return "xl", CLASS_XL2
    return "hbm", 0


def cap_f(tier, k):
    """Chains the in-wave filter holds in the LDS of a chaining wave of this class."""
    return (k * (ARR_BYTES if tier == "xl" else REC_BYTES + ARR_BYTES) - 64) // FLT_BYTES


def chain_weights(chains, seeds):
    """mem_chain_weight (bwamem.cpp:451-470) of every chain."""
    w = np.zeros(len(chains), np.int64)
    for i, c in enumerate(chains):
        s = seeds[int(c["seed_off"]):int(c["seed_off"]) + int(c["n"])]
        if len(s) == 1:
            w[i] = int(s["len"][0])
            continue
        tot = []
        for beg in (s["qbeg"].astype(np.int64), s["rbeg"].astype(np.int64)):
            t, end = 0, 0
            for b, ln in zip(beg.tolist(), s["len"].tolist()):
                if b >= end:
                    t += ln
                elif b + ln > end:
                    t += b + ln - end
                end = max(end, b + ln)
            tot.append(t)
        w[i] = min(min(tot), (1 << 30) - 1)
    return w


def model(case):
    """dict over COUNT_KEYS of what bwams_debug_chain_counts must report, plus "reads": per read (seeds, chains, chains at or above
    min_chain_weight, tier, redo, route) with route in None (no chain), "lane_seq", "in_wave", "heavy", "seq"."""
    oopt = mem_opts(**case.opts)[0]
    ch, sd, off = case.oracle(do_flt=False)
    w = chain_weights(ch, sd)
    ns = seeds_per_read(case)
    out = dict.fromkeys(COUNT_KEYS, 0)
    for i, t in enumerate(CLASS_ORDER):
        out[COUNT_KEYS[i]] = int((ns > t).sum())
    reads = []
    for r in range(len(case.reads)):
        n, lo, hi = int(ns[r]), int(off[r]), int(off[r + 1])
        tier, k = tier_of(n)
        nk = hi - lo
        redo = tier in ("lds", "xl") and len(np.unique(ch["pos"][lo:hi])) < nk
        out["redo"] += int(redo)
        if nk == 0:
            reads.append((n, 0, 0, tier, redo, None))
            continue
        n_chn = max(int((w[lo:hi] >= oopt.min_chain_weight).sum()), 1)
        hist = COUNT_KEYS[12 + sum(n_chn > e for e in HIST_EDGES)]
        if tier in ("lds", "xl") and not redo and n_chn <= cap_f(tier, k):
            route = "in_wave"
            out["in_wave"] += 1
            out[hist] += 1
        elif n_chn > LIGHT_CHAINS:
            out["n_heavy"] += 1
            route = "seq" if n_chn > HEAVY_CAP[-1] else "heavy"
            out["flt_seq" if route == "seq" else hist] += 1
        else:
            route = "lane_seq"
            out["lane_seq"] += 1
        reads.append((n, nk, n_chn, tier, redo, route))
    out["reads"] = reads
    return out


# ---- ksort.h's introsort against an adversary (the filter's sort at its depth limit) ----------------------------------------------

def ks_introsort_trace(n, lt):
    """ksort.h's introsort (src/ksort.h: ks_introsort) over the indices 0..n-1 with a caller-supplied `lt(i, j)` on ELEMENT ids;
    returns True when the depth limit sent a range to the comb-sort fallback.  Used only to BUILD an adversarial input."""
    a = list(range(n))
    hit = [False]
    if n < 1:
        return False
    if n == 2:
        return False
    d = 2
    while (1 << d) < n:
        d += 1
    d <<= 1
    stack, s, t = [], 0, n - 1
    while True:
        if s < t:
            d -= 1
            if d == 0:
                hit[0] = True
                t = s
                continue
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if lt(a[k], a[i]):
                if lt(a[k], a[j]):
                    k = j
            else:
                k = i if lt(a[j], a[i]) else j
            rp = a[k]
            if k != t:
                a[k], a[t] = a[t], a[k]
            while True:
                i += 1
                while lt(a[i], rp):
                    i += 1
                j -= 1
                while i <= j and lt(rp, a[j]):
                    j -= 1
                if j <= i:
                    break
                a[i], a[j] = a[j], a[i]
            a[i], a[t] = a[t], a[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
        else:
            if not stack:
                return hit[0]
            s, t, d = stack.pop()


def antiquicksort(n):
    """McIlroy's adversary ("A killer adversary for quicksort", 1999) against the introsort above: values are fixed only when
    a comparison needs them, so that every pivot turns out to be among the smallest of its range.  -> keys (a permutation)."""
    GAS = n
    val = [GAS] * n
    state = {"nsolid": 0, "cand": 0}

    def lt(x, y):
        if val[x] == GAS and val[y] == GAS:
            if x == state["cand"]:
                val[x] = state["nsolid"]
            else:
                val[y] = state["nsolid"]
            state["nsolid"] += 1
        if val[x] == GAS:
            state["cand"] = x
        elif val[y] == GAS:
            state["cand"] = y
        return val[x] < val[y]

    hit = ks_introsort_trace(n, lt)
    rest = state["nsolid"]
    for i in range(n):
        if val[i] == GAS:
            val[i] = rest
            rest += 1
    return np.array(val, np.int64), hit


# ---- the families ---------------------------------------------------------------------------------------------------------------

SMALL_W = dict(w=4, max_chain_gap=100)                         # 8 bases apart is another chain: thousands fit a strand


def straddlers(n):
    """n positions at which a 20-base seed lies across l_pac (skipped: bns_intv2rid says -2), repeated as needed."""
    return L_PAC - 1 - (np.arange(n, dtype=np.int64) % 19)


@functools.lru_cache(maxsize=None)
def class_limits():
    """(a) For every limit T of chain_count_kernel a read of T seeds and one of T + 1, default options: ladders over at most 500
    base positions 480 apart, in ascending, descending and random order, stored forward and backward.  Plus a read that is over
    the lane limit only thanks to skipped seeds, and one over it whose every seed is skipped."""
    rng = np.random.default_rng(5)
    base = grid(480, room=480)
    reads, notes = [], []
    for i, t in enumerate(sorted(CLASS_ORDER)):
        for n in (t, t + 1):
            sel = rng.permutation(base)[:min(n, 500)]
            reads.append(ladder(sel, n, how="fb"[(i + n) % 2], order=("rand", "asc", "desc")[(i + n) % 3], rng=rng))
            notes.append("seeds%d" % n)
    reads.append(singles(base[:30]) + [(40, 20, straddlers(5), "f")])
    notes.append("over_by_skipped")
    reads.append([(0, 20, straddlers(40), "f")])
    notes.append("all_skipped")
    return Case("class_limits", reads, notes)


def _array_reads(g, rng, sizes):
    """The ordered-array reads over the position grid g: `sizes` chains in random order, every insertion at the front, at the end, a
    pass whose 64 new chains fall between the 64 of the pass before, and insertions AT the 64-entry chunk edges: over 192 entries
    (three passes) the fourth pass inserts at indices 128, 127, 64 and 63 (highest first, so that none shifts another)."""
    reads, notes = [], []
    for n in sizes:
        reads.append(singles(rng.permutation(g)[:n]))
        notes.append("chains%d" % n)
    reads.append(singles(ordered(g[100:400], "desc", rng)))
    notes.append("front")
    reads.append(singles(ordered(g[100:400], "asc", rng)))
    notes.append("end")
    reads.append(singles(np.concatenate([g[1000:1128:2], g[1001:1128:2], g[1500:1700]])))
    notes.append("interleave")
    reads.append(singles(np.concatenate([g[0:384:2], g[[255, 253, 127, 125]]])))
    notes.append("chunk_edges")
    return reads, notes


@functools.lru_cache(maxsize=None)
def ordered_array():
    """(b) The wave tiers' ordered array under w = 4: 64 / 65 and 4096 / 4097 chains (the second level of sarr_lower; min_chain_weight
    = 23 drops the chains of the first four MEMs, a_[0] alone stays of the small reads) and the reads of _array_reads."""
    reads, notes = _array_reads(grid(8), np.random.default_rng(6), (64, 65, 4096, 4097))
    return Case("ordered_array", reads, notes, dict(SMALL_W, min_chain_weight=23))


@functools.lru_cache(maxsize=None)
def ordered_default():
    """(b) under default options: the same reads but the 4096 / 4097 ones, positions 120 apart."""
    reads, notes = _array_reads(grid(120), np.random.default_rng(16), (64, 65))
    return Case("ordered_default", reads, notes)


def _displaced(seed_i, seed_j, P=None, fill=None):
    """A chain C at P (query 0, 20 bases) settled in the first pass of 64 seeds; in the second pass seed i = (query, length, position)
    starts a chain between C and seed j, which looked C up."""
    far = grid(480, room=480)
    P = int(far[40]) if P is None else P
    fill = far[100:163] if fill is None else fill
    mems = [(0, 20, np.concatenate([[P], fill]), "f")]                            # 64 seeds: the first pass
    return mems + [(q, ln, np.array([pos]), "f") for q, ln, pos in (seed_i, seed_j)]


@functools.lru_cache(maxsize=None)
def settling():
    """(c) One read per settling rule of chain_seeds_batch, default options."""
    rng = np.random.default_rng(7)
    far = grid(480, room=480)
    P = int(far[10])
    reads, notes = [], []
    reads.append(singles(rng.permutation(far)[:300]))                              # nothing touches anything: passes only
    notes.append("independent")
    reads.append([(0, 20, P + 5 * np.arange(200), "f"), (100, 20, rng.permutation(far[200:300]), "f")])
    notes.append("tandem")                                                          # every hit extends the previous one's chain
    reads.append(ladder(far[20:40], 80))                                            # seeds 20 .. 39 extend the chains seeds 0 .. 19 start in the same pass,
    notes.append("touched")                                                         # 40 .. 59 the chains 20 .. 39 have just extended
    Q = int(far[40])                                                                # _displaced's C
    reads.append(_displaced((10, 40, Q + 150), (121, 20, Q + 160))); notes.append("displaced_new")          # x - y = 101 against i: a chain of its own (C would have merged it)
    reads.append(_displaced((10, 40, Q + 150), (120, 20, Q + 160))); notes.append("displaced_unsettled")    # x - y = 100 against i: extends the chain born in the pass
    reads.append(_displaced((10, 40, Q + 150), (15, 20, Q + 155))); notes.append("displaced_noop")          # contained in i's seed
    # C on the forward strand, j beyond l_pac: C alone makes j a chain of its own (no chain crosses l_pac) ...
    reads.append(_displaced((10, 40, L_PAC + 50), (45, 20, L_PAC + 85), P=L_PAC - 600)); notes.append("displaced_across_lpac")   # ... but i, beyond l_pac too, takes it
    reads.append(_displaced((10, 40, L_PAC - 300), (20, 20, L_PAC + 10), P=L_PAC - 600)); notes.append("displaced_lpac_between")  # i before l_pac: j stays alone either way
    reads.append(singles(far[50:90]) + [repeat_of(int(far[60]))])
    notes.append("equal_in_pass")                                                   # 41 seeds, one pass: a second chain at far[60]
    reads.append(singles(far[50:150]) + [repeat_of(int(far[60]))])
    notes.append("equal_on_key")                                                    # the second chain's seed comes two passes later
    reads.append(singles(far[50:150]) + [(0, 19, far[60:61], "f"), (2, 10, far[61:62] + 2, "f"), (0, 25, far[62:63], "f")])
    notes.append("equal_contained")                                                 # the same seed again, one inside a seed, a longer one at a held position
    for n in (64, 65):                                                              # MEMs in a read: the lanes hold 64 (sm_regs)
        reads.append([(k, 19 + (k % 3), far[3 * k:3 * k + 2] + (k % 3), "f") for k in range(n)])
        notes.append("mems%d" % n)
    reads.append([(0, 20, far[300:340], "f"), (STEP, 30, far[300:340] + STEP, "f")])
    notes.append("two_smems")                                                       # one pass, two spans; the second's seeds extend the first's chains
    return Case("settling", reads, notes)


THREE = (40000, 80000)                                           # alt_tables: the three sequences [0, 40000) [40000, 80000) [80000, 120000)


@functools.lru_cache(maxsize=None)
def alt_tables(which):
    """(c), (e) on three sequences, none ALT ("none"), the middle one ("mid") or the first ("first").
    displaced_other_seq: C and seed i on the first sequence, seed j — 55 bases after i, inside the band — on the second: i's
    sequence makes j a chain of its own (on one sequence j would extend i's chain).
    alt_lane / alt_wave (6 and 46 seeds): a chain H of weight 67 on the middle sequence over the query span of two chains of
    weights 19 and 40 on the first.  All primary, H drops the 19.  H ALT ("mid"): an ALT chain does not shadow a primary one, both
    are kept free of it.  The light ones ALT ("first"): a primary chain shadows an ALT one as it would a primary one."""
    far = grid(480, room=480)
    c = np.zeros(3, loader.CONTIG_DTYPE)
    c["offset"], c["len"] = [0, THREE[0], THREE[1]], [THREE[0], THREE[1] - THREE[0], L_PAC - THREE[1]]
    c["is_alt"] = dict(none=[0, 0, 0], mid=[0, 1, 0], first=[1, 0, 0])[which]
    third = far[(far >= THREE[1] + 1000) & (far < L_PAC - 1000)]
    alt = [(0, 19, np.array([50000, 10000]), "f"), (0, 40, np.array([20000]), "f")] + [(STEP * k, 19, np.array([50000 + STEP * k]), "f") for k in (1, 2, 3)]
    reads = [_displaced((10, 40, THREE[0] - 50), (15, 20, THREE[0] + 5), P=THREE[0] - 200, fill=third[:63]), alt, alt + singles(third[:40], qbeg=300)]
    return Case("alt_" + which, reads, ["displaced_other_seq", "alt_lane", "alt_wave"], contigs=c)


def _tiling(n_seqs, rng):
    """n_seqs sequences tiling [0, L_PAC): lengths around L_PAC / n_seqs, a few of exactly 20 bases, every fifth ALT."""
    if n_seqs == 1:
        return loader.single_contig(L_PAC)
    mean = L_PAC // n_seqs
    ln = np.full(n_seqs, mean, np.int64)
    if mean > 24:
        odd = rng.permutation(n_seqs - 1)[:min(8, n_seqs // 4)]
        ln[odd] = 20
    ln[-1] += L_PAC - ln.sum()
    c = np.zeros(n_seqs, loader.CONTIG_DTYPE)
    c["len"], c["offset"] = ln, np.concatenate([[0], np.cumsum(ln)[:-1]])
    c["is_alt"] = (np.arange(n_seqs) % 5 == 3)
    return c


@functools.lru_cache(maxsize=None)
def sequences(n_seqs):
    """(d) 20-base seeds against n_seqs sequences: at a sequence's first base, ending at its last, filling a 20-base sequence,
    across two sequences and across l_pac (both skipped), on the reverse strand at both ends of the text; a wave-tier read with
    more than 64 seeds, one with 33 and a lane-tier read."""
    rng = np.random.default_rng(100 + n_seqs)
    c = _tiling(n_seqs, rng)
    off, ln = c["offset"].astype(np.int64), c["len"].astype(np.int64)
    pick = rng.permutation(n_seqs)[:min(n_seqs, 60)]
    first, last = off[pick], (off + ln - 20)[pick]
    exact = off[ln == 20]
    across = off[1:][:20] - 10 if n_seqs > 1 else np.zeros(0, np.int64)
    inner = rng.integers(0, L_PAC - 20, size=40)                 # anywhere: inside a sequence or across two
    fwd = np.concatenate([first, last, exact, across, inner, [L_PAC - 10, L_PAC - 20, 0]])
    rev = 2 * L_PAC - (fwd + 20)                               # the same intervals on the reverse strand
    ends = np.array([L_PAC, 2 * L_PAC - 20], np.int64)
    allp = np.concatenate([fwd, rev, ends])
    reads = [[(0, 20, rng.permutation(allp), "f"), (30, 20, rng.permutation(allp), "b")],
             [(5, 20, rng.permutation(allp)[:33], "f")],
             [(0, 20, np.concatenate([first[:8], last[:8], across[:4], inner[:2], ends]), "f"), (40, 20, rev[:8], "b")]]
    return Case("sequences%d" % n_seqs, reads, ["wave", "wave33", "lane"], contigs=c)


def _with_dominant(n_light, pos, qbeg=0):
    """n_light one-seed chains (weights 19 ..) under one chain of five 40-base seeds over the same query span: the filter drops a
    light chain at its first comparison, so that its pairwise pass stays linear."""
    P = int(pos[-1])
    dom = [(qbeg + 40 * k, 40, np.array([P + 40 * k]), "f") for k in range(5)]
    return singles(pos[:n_light], qbeg=qbeg) + dom


@functools.lru_cache(maxsize=None)
def filter_limits():
    """(e) Chains at or above min_chain_weight on both sides of the filter's limits, default options: 16 / 17 on a lane-tier read and
    on a redo read; the many-chain kernel's classes 64 .. 960 and heavy_read's 64-candidate batches (65, 66, 129) on redo reads
    (one repeated position: no LDS, so more than 16 chains means the list); 1197 / 1198 in class XL.  The light chains of a read
    share one query start: they overlap, weights tie in blocks, kept codes 1, 2 and 3 occur, and the reads with a second query
    group and a dominant chain have dropped chains too."""
    rng = np.random.default_rng(8)
    g120 = grid(120)
    far, rev = rng.permutation(g120[(g120 >= 480) & (g120 < L_PAC)]), rng.permutation(g120[g120 >= L_PAC])
    reads, notes = [], []
    for n in (16, 17):
        reads.append(singles(far[:n], per_mem=6))
        notes.append("lane%d" % n)
        reads.append(ladder(np.sort(grid(480, room=480)[:n - 1]), 3 * (n - 1)) + [repeat_of(int(grid(480, room=480)[0]))])
        notes.append("redo%d" % n)
    for n in (64, 65, 66, 128, 129, 256, 257, 512, 513, 960, 961):
        # a second query group on the other strand (a forward chain never takes a seed beyond l_pac): the two groups do not meet
        body = singles(far[:n - 1 - n // 3], per_mem=100) + singles(rev[:n // 3], qbeg=200, len0=30, per_mem=40)
        reads.append(body + [repeat_of(int(far[0]), qbeg=400)])
        notes.append("redo%d" % n)
    for n in (1197, 1198):
        b = np.sort(grid(120)[:n])
        reads.append([(0, 19, b[:500], "f"), (0, 20, b[500:1000], "f"), (0, 21, b[1000:], "f"),
                      (STEP, 19, b[:500] + STEP, "f"), (STEP, 20, b[500:1000] + STEP, "f"), (STEP, 21, b[1000:] + STEP, "f")])
        notes.append("xl%d" % n)
    # blocks of 16, 17 and 47 equal weights, twice: under a chain of weight 160 over the same query span (dropped; which of them
    # becomes the dominant chain's first shadowed one is the sort's tie order) and at query 300 on the other strand (kept, in tie order)
    reads.append([(0, 19, far[:16], "f"), (0, 25, far[16:33], "f"), (0, 31, far[33:80], "f")] +
                 [(40 * k, 40, far[200:201] + 40 * k, "f") for k in range(4)] +
                 [(300, 22, rev[:16], "f"), (300, 28, rev[16:33], "b"), (300, 34, rev[33:80], "f")] +
                 # below every other position: A, B inside A (A's first shadowed chain, code 1), C inside A beside B (code 2 stays)
                 [(400, 40, np.array([0]), "f"), (400, 20, np.array([150]), "f"), (422, 18, np.array([300]), "f")])
    notes.append("tie_blocks")
    keys, hit = antiquicksort(200)
    assert hit
    wts = 19 + (199 - keys)                                     # descending order: the sort makes the comparisons the adversary answered
    b = np.sort(grid(120)[:200])
    reads.append([(0, int(wts[i]), b[i:i + 1], "f") for i in range(200)])
    notes.append("depth_limit")
    return Case("filter_limits", reads, notes)


@functools.lru_cache(maxsize=None)
def filter_big():
    """(e) under w = 4: 3840 / 3841 chains on redo reads (the largest class of chain_heavy_kernel, and the sequential form beyond
    it) and 3803 / 3804 in class XL2 (the in-wave filter's capacity there), each under a dominant chain."""
    rng = np.random.default_rng(9)
    g8 = rng.permutation(grid(8)[:-200])
    tail = grid(8)[-100:-99]                                    # the dominant chain's place, clear of every other seed and of the text's end
    reads, notes = [], []
    for n in (3840, 3841):
        reads.append(_with_dominant(n - 2, np.concatenate([g8[:n - 2], tail])) + [repeat_of(int(g8[0]), qbeg=400)])
        notes.append("redo%d" % n)
    for n in (3803, 3804):
        b = np.concatenate([g8[:n - 1], tail])
        reads.append(_with_dominant(n - 1, b) + singles(g8[5000:5400], len0=10))      # 400 seeds below min_chain_weight: over 4096 seeds
        notes.append("xl2_%d" % n)
    return Case("filter_big", reads, notes, dict(SMALL_W, min_chain_weight=19))


@functools.lru_cache(maxsize=None)
def filter_options(which):
    """(e) The filter's options on the reads of filter_limits that have every kept code: max_chain_extend below the chain count
    ("extend"), min_chain_weight above every chain ("floor_all": a_[0] is kept) and above some ("floor_some")."""
    c = filter_limits()
    keep = [c.read(n) for n in ("lane16", "lane17", "redo17", "redo65", "redo257", "xl1197", "tie_blocks")]
    opts = dict(extend=dict(max_chain_extend=5), floor_all=dict(min_chain_weight=1000), floor_some=dict(min_chain_weight=21))[which]
    return Case("filter_" + which, [c.reads[r] for r in keep], [c.notes[r] for r in keep], opts)


@functools.lru_cache(maxsize=None)
def stride_pick():
    """(f) ert_pick's stride around max_occ = 50: hit counts 50, 51, 99, 100 and 151, MEMs without hits, duplicated MEMs."""
    rng = np.random.default_rng(10)
    far = rng.permutation(grid(480, room=480))
    reads, notes = [], []
    for hc in (50, 51, 99, 100, 151):
        reads.append([(0, 20, far[:hc], "fb"[hc % 2])])
        notes.append("hits%d" % hc)
    reads.append([(0, 20, far[:0], "f"), (5, 20, far[:40], "f"), (9, 25, far[:0], "b")])
    notes.append("empty_mems")
    reads.append([(0, 20, far[:0], "f")])
    notes.append("only_empty")
    reads.append([(7, 20, far[:30], "f"), (7, 20, far[30:60], "f"), (7, 20, far[:30], "b"), (3, 22, far[100:110], "f")])
    notes.append("duplicates")
    return Case("stride_pick", reads, notes, dict(max_occ=50))


@functools.lru_cache(maxsize=None)
def coordinates():
    """(g) A read of 32767 bases (the 16-bit query fields of ChainRec) with seeds whose end is the read's: long enough for
    mem_flt_chained_seeds, so its bases matter — it is a stretch of the genome with a few substitutions, and its seeds are where
    that stretch lies."""
    g, _ = setting()
    L, P = 32767, 40000
    c = Case("coordinates", [[(L - 60, 60, np.array([P + L - 60]), "f"), (L - 25, 25, np.array([P + L - 25, 2000]), "f"),
                              (100, 30, np.array([P + 100]), "b"), (32000, 19, np.array([P + 32000, 90000]), "f")]], ["long"], read_len=L)
    c.enc = g[P:P + L].copy()
    c.enc[::997] = (c.enc[::997] + 1) & 3
    return c


def all_cases():
    return ([class_limits(), ordered_array(), ordered_default(), settling()] + [alt_tables(w) for w in ("none", "mid", "first")] + [sequences(n) for n in (1, 64, 65, 4096, 4097)] +
            [filter_limits(), filter_big()] + [filter_options(w) for w in ("extend", "floor_all", "floor_some")] + [stride_pick(), coordinates()])
