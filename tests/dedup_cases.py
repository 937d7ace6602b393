"""Hand-made extension-stage regions for the tests of de-duplication (tests/test_gpu_dedup_limits.py, tests/test_dedup_cases.py).

Reads are edited windows of the toy genome; their slots are built with them, every field under the test's control.  `model`
restates what decides a read's and a pair's way through csrc/dedup.hip: the tier by slot count (dedup_triage_kernel, kLightN,
the three dedup_wave_kernel instances, kLdsN), mem_sort_dedup_patch's pairwise pass (bwamem.cpp:314-375), mem_patch_reg's
coordinate tests and acceptance test (bwamem.cpp:199-250), the band of bwa_gen_cigar2 (bwa.cpp:413-420) and the choice among the
four statements of the global alignment.  It is written from those sources, not from oracle/dedup_oracle.c, runs the pinned
ksw_global2 per candidate and takes the two sort orders from the pinned ks_introsort; tests/test_dedup_cases.py holds it against
loader.regs_finish region by region."""
import collections
import fractions

import numpy as np

import aln_cases as ac
from oracle import loader

LIGHT_N, SMALL_N, MID_N, LDS_N, EH_LDS_LEN = 16, 128, 512, 2048, 1000      # dedup.hip: kLightN, kSmallN, kMidN, kLdsN, kEhLdsLen
ALT = dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1)
OPTS = ({}, ALT)
MIN_RATIO = float(np.float32(0.90))                                         # PATCH_MIN_SC_RATIO, a float constant compared as double
MAX_R_BW = (float(np.float32(0.05)), float(np.float32(0.05) * np.float32(2)))
COUNT_KEYS = ("triage", "lane", "wave128", "wave512", "wave2048", "one_lane", "shortcut", "hbm", "lds", "reg1", "reg2", "reg3", "reg4")
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "sub", "csub", "w", "seedcov", "n_comp_is_alt")


def contigs_of(l_pac):
    """Three sequences, the middle one ALT."""
    c = np.zeros(3, loader.CONTIG_DTYPE)
    c["offset"], c["len"], c["is_alt"] = [0, 9000, 15000], [9000, 6000, l_pac - 15000], [0, 1, 0]
    return c


# ---- the restatement -----------------------------------------------------------------------------------------------
class Reg:
    __slots__ = FIELDS + ("slot",)

    def __init__(self, rec, slot):
        for f in FIELDS:
            setattr(self, f, int(rec[f]))
        self.slot = slot


def patch_geom(opt, l_pac, a, b):                             # bwamem.cpp:205-217
    if a.rb < l_pac and b.rb >= l_pac:
        return False
    if a.qb >= b.qb or a.qe >= b.qe or a.re >= b.re:
        return False
    w = abs((a.re - b.rb) - (a.qe - b.qb))
    r = abs((a.re - b.rb) / (b.re - a.rb) - (a.qe - b.qb) / (b.qe - a.qb))
    if a.re < b.rb or a.qe < b.qb:
        return not (w > opt.w << 1 or r >= MAX_R_BW[0])
    return not (w > opt.w << 2 or r >= MAX_R_BW[1])


def patch_w(opt, a, b):                                        # bwamem.cpp:218-219
    return min(abs((a.re - b.rb) - (a.qe - b.qb)) + a.w + b.w, opt.w << 2)


def predicted(a, b):
    """(q_s, r_s) as C evaluates them without contraction: the product is rounded, then the sum (bwamem.cpp:236-237)."""
    s = b.score + a.score
    q_s = int(float(b.qe - a.qb) / ((b.qe - b.qb) + (a.qe - a.qb)) * s + .499)
    r_s = int(float(b.re - a.rb) / ((b.re - b.rb) + (a.re - a.rb)) * s + .499)
    return q_s, r_s


def predicted_fused(a, b):
    """The same with the product and the sum in one fused multiply-add: one rounding, of the exact value."""
    s = b.score + a.score
    f = lambda num, den: int(float(fractions.Fraction(float(num) / den) * s + fractions.Fraction(.499)))   # noqa: E731
    return f(b.qe - a.qb, (b.qe - b.qb) + (a.qe - a.qb)), f(b.re - a.rb, (b.re - b.rb) + (a.re - a.rb))


def accepts(score, mx):
    return not score / mx < MIN_RATIO                          # bwamem.cpp:238


def need_of(mx):
    """The smallest score the acceptance test takes against the prediction mx."""
    need = int(MIN_RATIO * mx)
    while not accepts(need, mx):
        need += 1
    while accepts(need - 1, mx):
        need -= 1
    return need


def align(opt, l_pac, ref, read, a, b):
    """bwa_gen_cigar2 as mem_patch_reg calls it -> (variant 'none' | 'shortcut' | 'dp', score, band, l_query, rlen)."""
    w = patch_w(opt, a, b)
    lq, rb, re = b.qe - a.qb, a.rb, b.re
    if lq <= 0 or rb >= re or (rb < l_pac and re > l_pac):
        return "none", 0, None, lq, re - rb
    q, t = read[a.qb:b.qe], ref[rb:re]
    if rb >= l_pac:
        q, t = q[::-1], t[::-1]
    if lq == re - rb and w == 0:
        mat = np.array(opt.mat[:25], np.int64)
        return "shortcut", int(mat[t.astype(np.int64) * 5 + q].sum()), None, lq, re - rb
    ww = ac.band(opt, lq, re - rb, w)
    return "dp", loader.ksw_global2_score(q, t, ww, ac.sw_opt(opt)), ww, lq, re - rb


def _gt_f32(x, c, m):
    """(float)x > c * (float)m in single precision (bwamem.cpp:347: int64 operands converted to float)."""
    d = x - c * m
    if abs(d) > 1e-3 * (abs(m) + 1):
        return d > 0
    return bool(np.float32(x) > np.float32(c) * np.float32(m))


def tier_of(n_slots, n_live, force_seq=False):
    if n_live <= 1:
        return "triage"
    if n_slots <= LIGHT_N:
        return "lane"
    if n_slots > LDS_N or force_seq:
        return "one_lane"
    return "wave128" if n_slots <= SMALL_N else "wave512" if n_slots <= MID_N else "wave2048"


def variant_of(tier, max_read_len, kind, lq):
    """Which statement of the alignment a candidate of a read of this tier runs through."""
    if kind != "dp":
        return kind
    if tier in ("lane", "one_lane") or max_read_len > EH_LDS_LEN:
        return "hbm"
    return "lds" if lq >= 256 else "reg%d" % (1 + (lq >> 6))


def model(opt, regs, reg_off, enc, cum, ref, l_pac, contigs, force_seq=False):
    """Per read a dict: tier, out (the final regions as tuples over FIELDS, in order), cands (per patch candidate that reaches
    bwa_gen_cigar2: slots of a and b, variant, l_query, score, need, merged), merges, red (redundant drops), same (identical-hit
    drops).  `counts` turns the list into what bwams_debug_dedup_counts must return."""
    mlr = float(np.float32(opt.mask_level_redun))
    max_len = int(np.diff(cum).max()) if len(cum) > 1 else 1
    is_alt = [int(x) for x in contigs["is_alt"]]
    out = []
    for r in range(len(cum) - 1):
        read = enc[cum[r]:cum[r + 1]]
        slots = [Reg(regs[k], k - int(reg_off[r])) for k in range(int(reg_off[r]), int(reg_off[r + 1]))]
        a = [x for x in slots if x.qe > x.qb]
        tier = tier_of(len(slots), len(a), force_seq)
        st = dict(tier=tier, cands=[], merges=0, red=0, same=0, n_slots=len(slots))
        if len(a) > 1:
            a = [a[i] for i in loader.ars_sort(0, [x.re for x in a])]
            for x in a:
                x.n_comp_is_alt = 1
            for i in range(1, len(a)):
                p = a[i]
                if p.rid != a[i - 1].rid or p.rb >= a[i - 1].re + opt.max_chain_gap:
                    continue
                j = i - 1
                while j >= 0 and p.rid == a[j].rid and p.rb < a[j].re + opt.max_chain_gap:
                    q = a[j]
                    j -= 1
                    if q.qe == q.qb:
                        continue
                    or_ = q.re - p.rb
                    oq = q.qe - p.qb if q.qb < p.qb else p.qe - q.qb
                    mr = min(q.re - q.rb, p.re - p.rb)
                    mq = min(q.qe - q.qb, p.qe - p.qb)
                    if _gt_f32(or_, mlr, mr) and _gt_f32(oq, mlr, mq):
                        st["red"] += 1
                        if p.score < q.score:
                            p.qe = p.qb
                            break
                        q.qe = q.qb
                    elif q.rb < p.rb and patch_geom(opt, l_pac, q, p):
                        kind, score, ww, lq, rlen = align(opt, l_pac, ref, read, q, p)
                        mx = max(predicted(q, p))
                        ok = accepts(score, mx) and score > 0
                        if kind != "none":
                            st["cands"].append(dict(a=q.slot, b=p.slot, variant=variant_of(tier, max_len, kind, lq), lq=lq, rlen=rlen,
                                                    band=ww, score=score, need=need_of(mx), merged=ok))
                        if ok:
                            st["merges"] += 1
                            p.n_comp_is_alt = (p.n_comp_is_alt + q.n_comp_is_alt + 1) & 0x3fffffff
                            p.seedcov, p.sub, p.csub = max(p.seedcov, q.seedcov), max(p.sub, q.sub), max(p.csub, q.csub)
                            p.w = patch_w(opt, q, p)
                            p.qb, p.rb, p.truesc, p.score = q.qb, q.rb, score, score
                            q.qb = q.qe
            a = [x for x in a if x.qe > x.qb]
            a = [a[i] for i in loader.ars_sort(1, [x.score for x in a], [x.rb for x in a], [x.qb for x in a])]
            keep = [i == 0 or (a[i].score, a[i].rb, a[i].qb) != (a[i - 1].score, a[i - 1].rb, a[i - 1].qb) for i in range(len(a))]
            st["same"] = len(a) - sum(keep)
            a = [x for x, k in zip(a, keep) if k]
        for x in a:
            if x.rid >= 0 and is_alt[x.rid]:
                x.n_comp_is_alt = (x.n_comp_is_alt & 0x3fffffff) | (1 << 30)
        st["out"] = [tuple(getattr(x, f) for f in FIELDS) for x in a]
        out.append(st)
    return out


def counts(m, force_seq=False):
    """force_seq: the same batch under BWAMS_DEDUP_SEQ=1 (the wave tier's reads through the one-lane form, row in global memory)."""
    seq = lambda st: force_seq and st["tier"].startswith("wave")                                   # noqa: E731
    c = collections.Counter("one_lane" if seq(st) else st["tier"] for st in m)
    c.update("hbm" if seq(st) and k["variant"] != "shortcut" else k["variant"] for st in m for k in st["cands"])
    return {k: c.get(k, 0) for k in COUNT_KEYS}


def rid_of(contigs, l_pac, rb, re):
    pos = rb if rb < l_pac else 2 * l_pac - re
    return int(np.searchsorted(contigs["offset"], pos, side="right") - 1)


# ---- reads and slots ---------------------------------------------------------------------------------------------------
class Cases:
    """Reads (code arrays) and their slots.  Coordinates are given on the forward strand of the forward read; rev=True at
    `close` turns the read into its reverse complement and its slots onto the second strand."""

    def __init__(self, g, seed=1):
        self.g, self.l_pac = np.asarray(g, np.uint8), len(g)
        self.rng = np.random.default_rng(seed)
        self.contigs = contigs_of(self.l_pac)
        self.reads, self.slots, self.tags = [], [], []

    def read(self, bases, tag=""):
        self.reads.append(np.asarray(bases, np.uint8).copy()); self.slots.append([]); self.tags.append(tag)
        return len(self.reads) - 1

    def reg(self, r, rb, re, qb, qe, score, rid=None, **fields):
        ar = np.zeros(1, loader.ALNREG_DTYPE)[0]
        ar["rb"], ar["re"], ar["qb"], ar["qe"], ar["score"] = rb, re, qb, qe, score
        ar["truesc"], ar["secondary"], ar["seedlen0"] = score, -1, 19
        ar["rid"] = rid_of(self.contigs, self.l_pac, rb, re) if rid is None else rid
        for k, v in fields.items():
            ar[k] = v
        self.slots[r].append(ar)
        return len(self.slots[r]) - 1

    def purged(self, r, how=0):
        ar = np.zeros(1, loader.ALNREG_DTYPE)[0]
        ar["qb"] = ar["qe"] = -1 if how == 0 else 5
        ar["rb"], ar["re"], ar["rid"] = (-1, -1, -1) if how == 0 else (100, 90, 0)     # nothing about a purged slot is read
        self.slots[r].append(ar)

    def close(self, r, rev=False, shuffle=False):
        if rev:
            L = len(self.reads[r])
            self.reads[r] = ac.comp(self.reads[r])[::-1].copy()
            for ar in self.slots[r]:
                if ar["qe"] > ar["qb"]:
                    ar["rb"], ar["re"] = 2 * self.l_pac - ar["re"], 2 * self.l_pac - ar["rb"]
                    ar["qb"], ar["qe"] = L - ar["qe"], L - ar["qb"]
        if shuffle:
            self.slots[r] = [self.slots[r][i] for i in self.rng.permutation(len(self.slots[r]))]

    def pads(self, r, n, rid, at=2):
        """n slots that take part in no event: the whole read as query span, disjoint one-base reference spans from `at` on, on
        another sequence than the read's other regions (and with smaller ends than any of them: no scan is cut short)."""
        L = len(self.reads[r])
        for k in range(n):
            self.reg(r, at + 2 * k, at + 2 * k + 1, 0, L, 1 + k % 3, rid=rid)

    def extend(self, other):
        self.reads += other.reads; self.slots += other.slots; self.tags += other.tags
        return self

    def flat(self):
        cum = np.zeros(len(self.reads) + 1, np.int64)
        cum[1:] = np.cumsum([len(x) for x in self.reads])
        enc = np.concatenate(self.reads + [np.zeros(0, np.uint8)]).astype(np.uint8)
        regs = [ar for s in self.slots for ar in s]
        off = np.zeros(len(self.reads) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in self.slots])
        return enc, cum, (np.array(regs, loader.ALNREG_DTYPE) if regs else np.zeros(0, loader.ALNREG_DTYPE)), off


def subst(rng, x, at):
    x[at] = (x[at] + 1 + rng.integers(0, 3, size=np.size(at))) & 3


def _other_rid(c, rb, re):
    return (rid_of(c.contigs, c.l_pac, rb, re) + 1) % 3


def split_pair(c, p, lq, kind, d, rev, tag, aw=0, bw=0, pad=0, n_at=None, fit=True, clip=(0, 0), extra_edit=None):
    """A read whose two regions are the halves of its placement at g[p ..): between them d substituted bases ('mis'), d
    reference bases missing from the read ('del'), d bases inserted ('ins'), or nothing, the halves overlapping by d ('ovl').
    l_query of the merged pair is lq.  fit: the two scores are chosen so that the prediction about equals the merged score (the
    pair merges and the alignment's score shows in the output).  pad: that many more slots that take part in no event."""
    g, rng = c.g, c.rng
    n = lq + d if kind == "del" else lq - d if kind == "ins" else lq
    h = lq // 2 - (d if kind == "ins" else 0) // 2
    W = g[p:p + n].copy()
    if kind == "mis":
        subst(rng, W, np.arange(h, h + d))
        body, a, b = W, (p, p + h, 0, h), (p + h + d, p + n, h + d, n)
    elif kind == "del":
        body, a, b = np.concatenate([W[:h], W[h + d:]]), (p, p + h, 0, h), (p + h + d, p + n, h, n - d)
    elif kind == "ins":
        body, a, b = np.concatenate([W[:h], rng.integers(0, 4, size=d).astype(np.uint8), W[h:]]), (p, p + h, 0, h), (p + h, p + n, h + d, n + d)
    else:
        body, a, b = W, (p, p + h + d, 0, h + d), (p + h, p + n, h, n)
    if extra_edit:                                            # ('D', at): a reference base missing inside the second half
        at = extra_edit[1]
        body = np.concatenate([body[:at], body[at + 1:]])
        b = (b[0], b[1], b[2], b[3] - 1)
    if n_at is not None:
        body[n_at] = 4
    read = np.concatenate([rng.integers(0, 4, size=clip[0]).astype(np.uint8), body, rng.integers(0, 4, size=clip[1]).astype(np.uint8)])
    r = c.read(read, tag)
    sh = clip[0]
    ia = c.reg(r, a[0], a[1], a[2] + sh, a[3] + sh, max(a[3] - a[2], 1), w=aw, sub=int(rng.integers(0, 20)), csub=int(rng.integers(0, 9)),
               seedcov=int(rng.integers(10, 40)))
    ib = c.reg(r, b[0], b[1], b[2] + sh, b[3] + sh, max(b[3] - b[2], 1), w=bw, sub=int(rng.integers(0, 20)), csub=int(rng.integers(0, 9)),
               seedcov=int(rng.integers(10, 40)))
    if pad:
        c.pads(r, pad, _other_rid(c, a[0], a[1]))
    c.close(r, rev)
    return r, ia, ib


def pair_regs(c, r, ia=0, ib=1):
    """(a, b) of read r as the pass meets them: a upstream (the smaller end)."""
    x, y = Reg(c.slots[r][ia], ia), Reg(c.slots[r][ib], ib)
    return (x, y) if x.re < y.re else (y, x)


def merged_score(c, opt, r, ia=0, ib=1):
    a, b = pair_regs(c, r, ia, ib)
    ref = np.concatenate([c.g, ac.comp(c.g)[::-1]])
    assert patch_geom(opt, c.l_pac, a, b), (c.tags[r], vars_of(a), vars_of(b))
    return align(opt, c.l_pac, ref, c.reads[r], a, b)[1]


def vars_of(x):
    return {f: getattr(x, f) for f in FIELDS}


def set_need(c, r, target, ia=0, ib=1):
    """Choose the two scores so that the smallest merged score the acceptance test takes is `target`."""
    a, b = pair_regs(c, r, ia, ib)
    for s in range(2, 8 * max(target, 8)):
        a.score, b.score = s // 2, s - s // 2
        if need_of(max(predicted(a, b))) == target:
            c.slots[r][ia]["score"] = c.slots[r][ia]["truesc"] = a.score if a.slot == ia else b.score
            c.slots[r][ib]["score"] = c.slots[r][ib]["truesc"] = b.score if b.slot == ib else a.score
            return True
    return False                                             # the ratio of spans skips the prediction that would give it


def set_accepted(c, opt, r, slack=0):
    """Scores under which the pair merges, the threshold as close below its merged score less `slack` as the spans allow."""
    s = merged_score(c, opt, r)
    assert any(set_need(c, r, s - slack - k) for k in range(6)), c.tags[r]


def drop_last(c):
    c.reads.pop(); c.slots.pop(); c.tags.pop()


PAD = 17                                                     # slots beyond the pair: the read goes to the wave tier's smallest instance
SPOTS = tuple(400 + 2300 * i for i in range(8))


def variant_cases(g, opt, pad=0, long_read=False):
    """One patchable pair per read; tags: 'lq<n>' (l_query at the edges of the four statements of the alignment, an insertion, a
    deletion or a mismatch block between the halves, band dl + 3 or capped by 4 opt.w), 'shortcut', 'short_w1', 'short_len1' (the
    gap-free shortcut and each of its conditions off by one), 'n' (code 4 in the read).  pad: see split_pair; long_read: one
    more read of 1001 bases, so that the wave tier aligns on one lane with the row in global memory."""
    c = Cases(g, 21)
    k = 0
    for lq in (63, 64, 127, 128, 191, 192, 255, 256, 999):
        di, dm = max(1, lq // 40), max(1, lq // 60)
        for rev in (False, True):
            for kind, d, aw, bw in (("ins", di, 0, 0), ("del", di, 0, 0), ("mis", dm, 10, 0), ("ins", di, 300, 300)):
                p = SPOTS[k % 8] + k
                k += 1
                clip = (1, 0) if lq == 999 else (k % 3, k % 2)
                r, _, _ = split_pair(c, p, lq, kind, d, rev, "lq%d" % lq, aw, bw, pad, clip=clip)
                set_accepted(c, opt, r, k % 2)
    for i in range(8):
        rev, lq = bool(i & 1), (40, 100, 150, 260)[i // 2]
        p = SPOTS[i] + 77
        for tag, kind, d, aw, ee in (("shortcut", "mis", 2, 0, None), ("shortcut", "ovl", 5, 0, None), ("short_w1", "mis", 2, 1, None),
                                     ("short_len1", "ovl", 5, 0, ("D", lq - 9))):
            r, _, _ = split_pair(c, p, lq, kind, d, rev, tag, aw, 0, pad, extra_edit=ee)
            set_accepted(c, opt, r)
        r, _, _ = split_pair(c, p + 300, lq, "del", 2, rev, "n", 0, 3, pad, n_at=lq // 4)
        set_accepted(c, opt, r, 1)
    if long_read:
        c.read(c.rng.integers(0, 4, size=1001).astype(np.uint8), "long")
    return c


def max_gap_of(lq, kind):
    """The longest gap between the halves of a pair with this merged query span that mem_patch_reg's coordinate tests let through
    (the two relative offsets must differ by less than PATCH_MAX_R_BW: gap / merged span < 0.05f)."""
    d = lq // 10
    while not (d / (lq + d if kind == "del" else lq) < MAX_R_BW[0]):
        d -= 1
    return d


def threshold_cases(g, opt, pad=PAD):
    """Pairs with l_query < 256 whose merged score is the smallest the acceptance test takes ('at'), one less ('minus') and one
    more ('plus'), the damage all in the first quarter of the rows ('first'), all in the last ('last'), or one gap followed by perfect matches ('gap'; deletions and insertions in
    turn).  The band of such a pair is its gap plus 3, so no gap is too long for it; the gap is the longest that the coordinate
    tests of mem_patch_reg allow (max_gap_of; one or two bases shorter where the spans skip the threshold).  Tags: '<where>/<delta>'.  The damage is made by substituting bases until the score (re-scored by the pinned
    ksw_global2) has lost about seven per cent; the two regions' scores are then searched for the prediction whose threshold
    sits at, one above and one below that score."""
    c = Cases(g, 22)
    k = 0
    for lq in (60, 100, 150, 200, 250):
        for rev in (False, True):
            for where in ("first", "last", "gap"):
                for delta, name in ((0, "at"), (1, "minus"), (-1, "plus")):
                    k += 1
                    tag = "%s/%s" % (where, name)
                    for bump in range(6):                     # a shorter gap or one more substitution where the spans skip the threshold
                        p = SPOTS[k % 8] + 3 * k + 40 * bump
                        if where == "gap":
                            kind = "del" if k % 2 else "ins"
                            r, _, _ = split_pair(c, p, lq, kind, max_gap_of(lq, kind) - bump, rev, tag, 0, 0, pad)
                        else:
                            r, _, _ = split_pair(c, p, lq, "ovl", 4, rev, tag, 10, 10, pad)
                            n_mis = max(1, round(0.07 * lq * opt.a / (opt.a + opt.b))) + bump % 2
                            lo = 1 if where == "first" else lq - lq // 4
                            at = lo + c.rng.choice(lq // 4 - 1, size=n_mis, replace=False)
                            x = ac.comp(c.reads[r][::-1]) if rev else c.reads[r].copy()     # rows run along the forward read on both strands
                            subst(c.rng, x, at)
                            c.reads[r] = ac.comp(x)[::-1].copy() if rev else x
                        if set_need(c, r, merged_score(c, opt, r) + delta):
                            break
                        drop_last(c)
                    else:
                        raise ValueError(tag)
    return c


# (span sum, merged span, a.score + b.score) -> the prediction without | with contraction, and the merged score at which the
# acceptance test flips between them
ROUNDING_ROWS = ((1000, 1007, 643), (1000, 563, 127), (1000, 689, 709), (1000, 1011, 591))


def _damage_to(c, opt, r, target):
    """One block of Ns (a path gains nothing by going round it) and up to a few substitutions elsewhere, so that the merged
    score is exactly `target`."""
    clean = c.reads[r].copy()
    lq = len(clean)
    lose = merged_score(c, opt, r) - target
    assert lose >= 0, (c.tags[r], lose)
    n_s = next(m for m in range(opt.a + 2) if (lose - m * (opt.a + opt.b)) % (opt.a + 1) == 0 and lose >= m * (opt.a + opt.b))
    n_n = (lose - n_s * (opt.a + opt.b)) // (opt.a + 1)
    assert n_n + 60 < lq, (c.tags[r], n_n)
    for attempt in range(20):
        rd = clean.copy()
        at = int(c.rng.integers(45, lq - n_n - 5))
        rd[at:at + n_n] = 4
        free = np.concatenate([np.arange(5, at - 3), np.arange(at + n_n + 3, lq - 5)])
        subst(c.rng, rd, c.rng.choice(free, size=n_s, replace=False))
        c.reads[r] = rd
        if merged_score(c, opt, r) == target:
            return
    raise ValueError((c.tags[r], target))


def rounding_cases(g, opt, pad=0, long_rows=False):
    """Pairs from ROUNDING_ROWS: the exact value of ratio * score sum + .499 is an integer, so that rounding the product first
    and rounding once give predictions one apart, and the merged score is the one at which the acceptance test tells them apart.
    Tags 'q<row>' (the geometry on the query side and on the reference side: q_s = r_s decide) and 'r<row>' (on the reference
    side alone, seven reference bases missing from the read: r_s decides).  long_rows: the rows whose merged query span exceeds
    1000 bases (their reads put the whole batch on the one-lane alignment of the wave tier) instead of the others."""
    c = Cases(g, 23)
    k = 0
    for row, (ssum, span, sc) in enumerate(ROUNDING_ROWS):
        ha = ssum // 2
        v = ssum - span                                       # overlap of the two spans (negative: a gap between them)
        for side in ("q", "r"):
            if ((span if side == "q" else span - 7) > EH_LDS_LEN) != long_rows:
                continue
            for rev in (False, True):
                for rep in range(4):
                    p = SPOTS[k % 8] + 11 * k
                    k += 1
                    tag = "%s%d" % (side, row)
                    ra, rb_ = (p, p + ha), (p + ha - v, p + span)
                    if side == "q":                           # the same geometry on both sides
                        qa, qb_ = (0, ha), (ha - v, span)
                        read = g[p:p + span].copy()
                    else:                                     # seven reference bases missing from the read: the merged query span is the shorter
                        qa, qb_ = (0, ha), (span - 7 - (ssum - ha), span - 7)
                        read = np.concatenate([g[p:p + 30], g[p + 37:p + span]])
                    r = c.read(read, tag)
                    s1 = sc // 2 - rep
                    c.reg(r, ra[0], ra[1], qa[0], qa[1], s1, w=3 + rep)
                    c.reg(r, rb_[0], rb_[1], qb_[0], qb_[1], sc - s1, w=2)
                    if pad:
                        c.pads(r, pad, _other_rid(c, ra[0], ra[1]))
                    c.close(r, rev)
                    a, b = pair_regs(c, r)
                    un, fu = max(predicted(a, b)), max(predicted_fused(a, b))
                    assert un != fu, (tag, un, fu)
                    lo, hi = sorted((need_of(un), need_of(fu)))
                    assert hi == lo + 1, (tag, lo, hi)
                    _damage_to(c, opt, r, lo)                 # accepted against the smaller prediction, refused against the larger
    return c


def busy_read(c, n_slots, form, L=150, rev=None, n_cluster=None):
    """A read with n_slots slots: a cluster of jittered sub-intervals of the read's true placement (redundant pairs, patchable
    pairs, one split pair that merges), copies of some of them on another sequence (identical score, rb, qb), and for the rest
    slots that take part in hardly any event (the whole read as query span, short disjoint reference spans all over the text,
    sequences changing every 40 of them; a few of them in pairs with equal ends).  form 0: all live; 1, 2: all but one, two
    purged (the survivors are the split pair's halves)."""
    rng, g, l_pac = c.rng, c.g, c.l_pac
    p = int(rng.integers(300, l_pac - 600))
    read = g[p:p + L].copy()
    subst(rng, read, rng.choice(L, size=2, replace=False))
    r = c.read(read, "busy%d/%d" % (n_slots, form))
    rev = bool(rng.integers(0, 2)) if rev is None else rev
    todo = []
    if n_slots >= 2:
        h = L // 2 - 5
        todo += [(p, p + h, 0, h, h - 2), (p + h + 3, p + L, h + 3, L, L - h - 5)]
    if form == 0 and n_slots >= 6:                           # the same halves where the read does not match: always met, never merged
        p2 = p + 2000 if p + 2000 + L < l_pac - 10 else p - 2000
        todo += [(p2, p2 + h, 0, h, h - 2), (p2 + h + 3, p2 + L, h + 3, L, L - h - 5)]
    live = n_slots if form == 0 else min(form, n_slots)
    m = min(max(live - len(todo) - 4, 0), int(rng.integers(4, 13)) if n_cluster is None else n_cluster)
    for _ in range(m):
        qb = int(rng.integers(0, L - 40))
        qe = int(rng.integers(qb + 25, L + 1))
        j1, j2 = (int(x) for x in rng.integers(-1, 2, size=2))
        todo.append((p + qb + j1, p + qe + j2, qb, qe, qe - qb - int(rng.integers(0, 7))))
    for t in todo[:live]:
        c.reg(r, *t, rid=rid_of(c.contigs, l_pac, t[0], t[1]), w=int(rng.integers(0, 9)), sub=int(rng.integers(0, 30)), csub=int(rng.integers(0, 9)),
              seedcov=int(rng.integers(5, 60)))
    rest = live - len(c.slots[r])
    n_dup = min(rest // 2, 3 + n_slots // 200)
    if rest > 0:
        x = np.arange(10, (2 * l_pac - 10) // 3)
        cells = x[~(((3 * x >= p - 6) & (3 * x <= p + L + 6)) | (np.abs(3 * x - l_pac) < 6))]
        prev, plain = 0, []
        for i, x in enumerate(np.sort(rng.choice(cells, size=rest - n_dup, replace=False))):
            rb = 3 * int(x)
            if i % 25 == 7:                                  # this one and the next end at the same base: a tie of the first sort, a redundant pair
                c.reg(r, rb - 1, rb + 1, 0, L, 2 + i % 3, rid=(i // 40) % 3)
            elif i % 25 == 8:
                c.reg(r, prev, prev + 1, 0, L, 1 + i % 4, rid=(i // 40) % 3)
            else:
                plain.append(c.reg(r, rb, rb + 1 + i % 2, 0, L, 1 + i % 4, rid=(i // 40) % 3 if i % 97 else -1))
            prev = rb
        for k in rng.choice(plain, size=n_dup, replace=False):            # the same (score, rb, qb) on another sequence: an identical hit
            ar = c.slots[r][int(k)].copy()
            ar["rid"] = (int(ar["rid"]) + 2) % 3
            c.slots[r].append(ar)
    while len(c.slots[r]) < n_slots:
        c.purged(r, len(c.slots[r]) & 1)
    c.close(r, rev, shuffle=True)
    return r


TIER_SLOTS = (0, 1, 2, 16, 17, 128, 129, 512, 513, 2048, 2049, 2600)


TIER_MORE = 3                                                # further all-live reads per slot count of two and more


def tier_cases(g):
    """Every slot count of TIER_SLOTS all live, all but one purged and all but two purged; then, for the counts of two and more,
    TIER_MORE further all-live reads each (other placements, other clusters): ten reads per tier, eight of them all live."""
    c = Cases(g, 24)
    for n in TIER_SLOTS:
        for form in (0, 1, 2):
            busy_read(c, n, form)
    for _ in range(TIER_MORE):
        for n in TIER_SLOTS[2:]:
            busy_read(c, n, 0)
    return c


def fuzz_cases(g, seed):
    """Some 210 reads whose slot counts are drawn across all tiers."""
    c = Cases(g, 100 + seed)
    rng = c.rng
    ns = [int(x) for x in rng.integers(0, 17, size=130)] + [int(x) for x in rng.integers(17, 129, size=40)] + \
         [int(x) for x in rng.integers(129, 513, size=14)] + [int(x) for x in rng.integers(513, 2049, size=7)] + \
         [int(x) for x in rng.integers(2049, 2400, size=7)] + list(TIER_SLOTS[3:11])
    for i in rng.permutation(len(ns)):                       # the largest reads keep at least two live regions: eight reads or more per tier
        form = 0 if rng.random() < 0.85 else 2 if ns[i] > MID_N else int(rng.integers(1, 3))
        busy_read(c, ns[i], form, L=int(rng.integers(100, 250)))
    return c


# ---- the order of events in the wave tier ------------------------------------------------------------------------------------------
def _quiet(c, r, ends, rb0, q0, rid):
    """Slots between and around the regions of a scenario that take part in no event: two query bases of their own behind the
    scenario's part of the read (no overlap on the query with anything: never redundant), reference spans nested round the
    scenario's (a span that ends later starts earlier, and all start before the scenario's regions: never the second region of a
    patchable pair, and as the first one its query span lies behind the other's), ends as given.  rid: a number or a function of k."""
    for k, re in enumerate(sorted(ends)):
        c.reg(r, rb0 - k, re, q0 + 2 * k, q0 + 2 * k + 2, 2, rid=rid(k) if callable(rid) else rid)


ORDER_LE = 380                                               # the scenario's part of a read; the quiet slots' bases follow


def order_read(c, p, d, what, rid=None, d2=3, n_above=2):
    """A read of the wave tier whose regions lie within max_chain_gap of each other: the scenario's regions among quiet slots,
    the upper region d sort ranks above the lower one (lane d - 1 of the scan: 1 and 65 are a chunk's first lane, 64 and 128 its
    last).  p: where on the text (either strand) the scenario's part of the read was taken.
      'merge': q d ranks below p merges into it; 'merge_end': the same with q the lowest region of all (the scan ends with the
      merge); 'merge_rid': ... with a region of another sequence right below q; 'p_loses' / 'q_loses': a redundant pair (after
      'q_loses' the scan goes on to a region d2 ranks further down that merges); 'cascade': c <- b <- a with b d ranks below c
      and a d2 ranks below b, (a, c) failing the coordinate tests until c has taken b in."""
    l_pac, Le = c.l_pac, ORDER_LE
    ref = np.concatenate([c.g, ac.comp(c.g)[::-1]])
    body = ref[p:p + Le].copy()
    rid = rid_of(c.contigs, l_pac, p, p + Le) if rid is None else rid
    if what == "cascade":                                     # a [0, 60), b [60, 140) with 30 bases inserted at 100, c the rest
        body = np.concatenate([ref[p:p + 100], c.rng.integers(0, 4, size=30).astype(np.uint8), ref[p + 100:p + Le]])
        regs = [(p, p + 60, 0, 60, 60, 0), (p + 60, p + 140, 60, 170, 44, 40), (p + 140, p + Le, 170, Le + 30, Le - 140, 0)]
    elif what in ("merge", "merge_end", "merge_rid"):
        subst(c.rng, body, np.arange(60, 63))
        regs = [(p, p + 60, 0, 60, 60, 2), (p + 63, p + Le, 63, Le, Le - 63, 2)]
    elif what == "p_loses":                                   # q inside p, d bases shorter at the end, the better score
        regs = [(p + 1, p + Le - d, 1, Le - d, Le, 0), (p, p + Le, 0, Le, Le - 5, 0)]
    elif what == "q_loses":                                   # a, then q (its query span starts where a's does: the two are no pair), then p
        subst(c.rng, body, np.arange(60, 63))
        regs = [(p, p + 60, 0, 60, 60, 2), (p + 64, p + Le - d, 0, Le - 1, Le - 70, 0), (p + 63, p + Le, 63, Le, Le - 63, 2)]
    else:
        raise ValueError(what)
    L = len(body)
    lo, top = regs[0][1], regs[-1][1]
    below = [lo - (2 if what == "merge_rid" else 1) - k for k in range(0 if what == "merge_end" else 3)]
    if what == "cascade":                                     # ranks: a, d2 - 1 quiet, b, d - 1 quiet, c
        between = list(range(lo + 1, lo + d2)) + list(range(regs[1][1] + 1, regs[1][1] + d))
        assert lo + d2 <= regs[1][1] and regs[1][1] + d <= top, (d, d2)
    elif what == "q_loses":                                   # ranks: a, d2 - 1 quiet, q, d - 1 quiet, p
        between = list(range(lo + 1, lo + d2)) + list(range(regs[1][1] + 1, top))
        assert lo + d2 <= regs[1][1] and regs[1][1] - regs[1][0] > 20, (d, d2)
    else:
        between = list(range(lo + 1, lo + d))
        assert lo + d <= top, (what, d)
    ends = below + between + [top + 1 + k for k in range(n_above)]
    read = np.concatenate([body, c.rng.integers(0, 4, size=2 * len(ends) + 2).astype(np.uint8)])
    r = c.read(read, "%s/%d" % (what, d))
    for rb, re, qb, qe, sc, w in regs:
        c.reg(r, rb, re, qb, qe, sc, rid=rid, w=w, sub=int(c.rng.integers(0, 30)), seedcov=int(c.rng.integers(5, 60)))
    _quiet(c, r, ends, min(x[0] for x in regs) - 5, L, rid)
    if what == "merge_rid":                                   # right below q in the order of ends, on another sequence
        c.reg(r, p - 3, lo - 1, L, L + 1, 3, rid=(rid + 1) % 3 if rid >= 0 else 0)
    c.close(r, False, shuffle=True)
    return r


ORDER_LANES = (1, 2, 63, 64, 65, 128, 129, 200, 290)
ORDER_KINDS = ("merge", "merge_end", "merge_rid", "p_loses", "q_loses", "cascade")


def order_cases(g):
    """Reads of 65 to 300 live regions for the wave tier's pairwise pass; see order_read.  Both strands; among them a sequence
    of rid -1, the ALT sequence, two sequences interleaved by end, a pair across the strands, a region that spans l_pac."""
    c = Cases(g, 25)
    l_pac = len(g)
    k = 0
    for d in ORDER_LANES:
        for what in ORDER_KINDS:
            k += 1
            p = (700 + 1700 * (k % 8) + 13 * k) if k % 5 else 9400 + 37 * (k % 90)       # every fifth on the ALT sequence
            if k & 1:
                p = 2 * l_pac - p - 1000                      # the second strand
            order_read(c, p, d if what != "cascade" or d < 200 else d - 100, what, rid=-1 if k % 7 == 3 else None,
                       d2=(1, 3, 64, 70)[k % 4] if what in ("cascade", "q_loses") else 3, n_above=max(2, 70 - d))
    for i in range(8):                                        # two sequences interleaved by end: every scan ends at its first region
        r = c.read(np.concatenate([g[700 + i:900 + i], c.rng.integers(0, 4, size=200).astype(np.uint8)]), "interleaved")
        c.reg(r, 700 + i, 760 + i, 0, 60, 60, rid=0, w=2)
        c.reg(r, 763 + i, 900 + i, 63, 200, 137, rid=0, w=2)  # its partner is right below it in the order of ends: they merge
        _quiet(c, r, [759 + i - 3 * k for k in range(70)], 400, 200, lambda k: k & 1)
        c.close(r, bool(i & 1), shuffle=True)
    for i in range(8):                                        # a forward, b on the second strand, one sequence, within the gap
        r = c.read(c.rng.integers(0, 4, size=400).astype(np.uint8), "cross")
        c.reg(r, l_pac - 300 - i, l_pac - 200 - i, 0, 100, 100, rid=2, w=2)
        c.reg(r, l_pac + 100 + i, l_pac + 200 + i, 103, 203, 100, rid=2, w=2)
        _quiet(c, r, [l_pac - 150 + 3 * k for k in range(70)], l_pac - 400, 204, 2)
        c.close(r, False, shuffle=True)
    for i in range(8):                                        # b spans l_pac: the pair passes the coordinate tests, nothing is aligned
        r = c.read(np.concatenate([g[l_pac - 200:], ac.comp(g)[::-1][:10], c.rng.integers(0, 4, size=200).astype(np.uint8)]), "lpac")
        c.reg(r, l_pac - 200 + i, l_pac - 100, i, 100, 100, rid=2, w=2)
        c.reg(r, l_pac - 97, l_pac + 3 + i % 3, 103, 203 + i % 3, 100, rid=2, w=2)
        _quiet(c, r, [l_pac - 102 - 3 * k for k in range(70)], l_pac - 500, 210, 2)
        c.close(r, False, shuffle=True)
    return c
