"""Hand-made final regions for the tests of mem_reg2aln (tests/test_gpu_aln_limits.py, tests/test_oracle_aln.py).

A read is an edited copy of a window of the genome and its region is built with it, every field under the test's control.
`model` restates what decides a region's way through the library: the band inference and the retry loop of mem_reg2aln
(bwamem.cpp:2553-2567), the band of bwa_gen_cigar2 (bwa.cpp:400, 413-420) and the rule by which aln_plan_kernel sends a region
to one of its launches (csrc/reg2aln.hip).  It is written from those sources, not from oracle/aln_oracle.c, and runs the pinned
ksw_global2 per try."""
import numpy as np

from oracle import loader

RING_COLS, WAVE_COLS, WAVE_TGT = 32, 512, 1024      # reg2aln.hip: the ring's columns, kWaveCols, kWaveTgt


def opts(**kw):
    """(oracle options, library options) with the same fields set; a / b also refill the scoring matrix."""
    from bwams import capi
    a, b = kw.pop("a", 1), kw.pop("b", 4)
    o, g = loader.default_mem_opt(a, b), capi.default_mem_opt(a, b)
    for k, v in kw.items():
        setattr(o, k, v); setattr(g, k, v)
    return o, g


def sw_opt(opt):
    o = loader.default_sw_opt(5, opt.a, opt.b)
    o.o_del, o.e_del, o.o_ins, o.e_ins = opt.o_del, opt.e_del, opt.o_ins, opt.e_ins
    for i in range(25):
        o.mat[i] = opt.mat[i]
    return o


def comp(x):
    x = np.asarray(x, np.uint8)
    return np.where(x < 4, 3 - x, x).astype(np.uint8)


# ---- the restatement -----------------------------------------------------------------------------------------------
def infer_bw(l1, l2, score, a, q, r):                     # bwamem.cpp:2630-2637
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = int(float(min(l1, l2) * a - score - q) / r + 2.)  # the (int) of C truncates towards zero, as int() does
    return max(w, abs(l1 - l2))


def inferred_w2(opt, lq, lr, truesc, ar_w):                # bwamem.cpp:2553-2557
    w2 = max(infer_bw(lq, lr, truesc, opt.a, opt.o_del, opt.e_del), infer_bw(lq, lr, truesc, opt.a, opt.o_ins, opt.e_ins))
    if w2 > opt.w:
        w2 = min(w2, ar_w)
    return w2


def band(opt, lq, lr, w2):                                 # bwa.cpp:413-420
    max_ins = int(float(((lq + 1) >> 1) * opt.mat[0] - opt.o_ins) / opt.e_ins + 1.)
    max_del = int(float(((lq + 1) >> 1) * opt.mat[0] - opt.o_del) / opt.e_del + 1.)
    max_gap = max(max_ins, max_del, 1)
    d = abs(lr - lq)
    return max(min((max_gap + d + 1) >> 1, w2), d + 3)


def retry_loop(opt, q, t, truesc, ar_w, cigar=False):
    """The loop at bwamem.cpp:2558-2567 over the sequences as bwa_gen_cigar2 aligns them.  Returns (tries, exit, cigar):
    tries = [(band or -1 for the gap-free shortcut, score)], exit in 'same' (the score of the try before), 'cap' (w2 reached
    4 opt.w), 'score' (the score came within a of truesc), 'three' (three tries made)."""
    so = sw_opt(opt)
    lq, lr = len(q), len(t)
    w2 = inferred_w2(opt, lq, lr, truesc, ar_w)
    tries, last, i, cig = [], -(1 << 30), 0, None
    while True:
        w2 = min(w2, opt.w << 2)
        if lq == lr and w2 == 0:                           # bwa.cpp:400-409
            w, score = -1, int(sum(opt.mat[int(tb) * 5 + int(qb)] for qb, tb in zip(q, t)))
            cig = np.array([lq << 4], np.uint32)
        else:
            w = band(opt, lq, lr, w2)
            if cigar:
                score, cig = loader.ksw_global2_cigar(q, t, w, so)
            else:
                score = loader.ksw_global2_score(q, t, w, so)
        tries.append((w, score))
        if score == last:
            return tries, "same", cig
        if w2 == opt.w << 2:
            return tries, "cap", cig
        last = score
        w2 <<= 1
        i += 1
        if i >= 3:
            return tries, "three", cig
        if not score < truesc - opt.a:
            return tries, "score", cig


def aligned_seqs(ar, read, ref, l_pac):
    q, t = read[int(ar["qb"]):int(ar["qe"])], ref[int(ar["rb"]):int(ar["re"])]
    return (q[::-1], t[::-1]) if ar["rb"] >= l_pac else (q, t)      # bwa.cpp:394-399


def rejected(ar, l_pac):
    """What mem_reg2aln answers with the unmapped record (bwamem.cpp:2541), what bwa_gen_cigar2 rejects (bwa.cpp:391-393) and
    the library's own limit on the reference span."""
    rb, re, lq = int(ar["rb"]), int(ar["re"]), int(ar["qe"]) - int(ar["qb"])
    return rb < 0 or re < 0 or lq <= 0 or re - rb <= 0 or (rb < l_pac and re > l_pac) or re > 2 * l_pac or re - rb > 1 << 20


TIES = {1: "M|E", 2: "H|F", 4: "D extended|opened", 8: "I extended|opened"}     # loader.ksw_global2_cigar's flip bits


def ties_of(opt, q, t, w):
    """The comparisons of the direction byte on whose tie rule the CIGAR of this alignment hangs: turned, the CIGAR changes."""
    so = sw_opt(opt)
    base = loader.ksw_global2_cigar(q, t, w, so)[1]
    return {bit for bit in TIES if not np.array_equal(loader.ksw_global2_cigar(q, t, w, so, flip=bit)[1], base)}


def model(opt, regs, reg_off, enc, cum, ref, l_pac, cigar=False, ties=False):
    """Per region a dict: route ('bad', 'simple', 'ring', 'wave1', 'wave2'), requeue (ring -> wave launch 2), hbm (the wave kernel
    passes it on to the launch with the row in global memory), tries, exit, lq, lr (and, on request, cigar, and ties: ties_of the
    last try).  counts: what bwams_debug_aln_lists must return."""
    out = []
    for r in range(len(reg_off) - 1):
        read = enc[cum[r]:cum[r + 1]]
        for k in range(int(reg_off[r]), int(reg_off[r + 1])):
            ar = regs[k]
            if rejected(ar, l_pac):
                out.append(dict(route="bad", requeue=False, hbm=False, tries=[], exit=None, lq=0, lr=0, cigar=None, ties=set()))
                continue
            q, t = aligned_seqs(ar, read, ref, l_pac)
            tries, ex, cig = retry_loop(opt, q, t, int(ar["truesc"]), int(ar["w"]), cigar)
            w1 = tries[0][0]
            route = "simple" if w1 < 0 else "ring" if 2 * w1 + 2 <= RING_COLS else "wave1" if 2 * w1 + 2 <= 128 else "wave2"
            requeue = route == "ring" and any(2 * w + 2 > RING_COLS for w, _ in tries)
            hbm = (route in ("wave1", "wave2") or requeue) and len(q) + 1 > WAVE_COLS
            out.append(dict(route=route, requeue=requeue, hbm=hbm, tries=tries, exit=ex, lq=len(q), lr=len(t), cigar=cig,
                            ties=ties_of(opt, q, t, tries[-1][0]) if ties and w1 >= 0 else set()))
    return out


def counts(m):
    return np.array([sum(x["route"] == "ring" for x in m), sum(x["route"] == "wave1" for x in m),
                     sum(x["route"] == "wave2" or x["requeue"] for x in m), sum(x["hbm"] for x in m)], np.int64)


def kernel_of(x):
    """The kernel that finishes the region."""
    if x["route"] in ("bad", "simple"):
        return x["route"]
    return "hbm" if x["hbm"] else "wave" if x["requeue"] or x["route"] != "ring" else "ring"


def truesc_for(opt, lq, lr, w2, ar_w=1 << 20):
    """The largest truesc from which mem_reg2aln infers the band w2 for these lengths."""
    for truesc in range(min(lq, lr) * opt.a + 1, -(1 << 16), -1):
        if inferred_w2(opt, lq, lr, truesc, ar_w) == w2:
            return truesc
    raise ValueError((lq, lr, w2))


# ---- reads and regions -------------------------------------------------------------------------------------------------
class Cases:
    """Reads as edited windows of the genome g, and their regions.  An edit is ('S', at) a substitution, ('N', at) an N in the
    read, ('D', at, n) n window bases missing from the read, ('I', at, n or bases) bases inserted before window base at."""

    def __init__(self, g, seed=1):
        self.g, self.l_pac = np.asarray(g, np.uint8), len(g)
        self.rng = np.random.default_rng(seed)
        self.reads, self.regs, self.tags = [], [], []          # regs[r] = the regions of read r

    def segment(self, p, n, edits):
        r = [int(x) for x in self.g[p:p + n]]
        for e in sorted(edits, key=lambda e: -e[1]):
            at = e[1]
            if e[0] == "S":
                r[at] = (r[at] + 1 + int(self.rng.integers(0, 3))) & 3
            elif e[0] == "N":
                r[at] = 4
            elif e[0] == "D":
                del r[at:at + e[2]]
            elif e[0] == "I":
                ins = [int(x) for x in (self.rng.integers(0, 4, size=e[2]) if np.isscalar(e[2]) else e[2])]
                r[at:at] = ins
            else:
                raise ValueError(e)
        return np.array(r, np.uint8)

    def add(self, p, n, edits=(), rev=False, clip=(0, 0), truesc=None, w2=None, tag="", opt=None, **fields):
        """A read over g[p, p + n) with one region; returns the read's index.  truesc: given, or the one that infers the band w2,
        or (default) the score of the unbanded global alignment.  opt (oracle options) is needed for the last two."""
        seg = self.segment(p, n, edits)
        c5, c3 = (self.rng.integers(0, 4, size=c).astype(np.uint8) for c in clip)
        ar = np.zeros(1, loader.ALNREG_DTYPE)[0]
        if rev:                                              # the read is the reverse complement; its region lies on the second strand
            read = comp(np.concatenate([c5, seg, c3]))[::-1]
            ar["rb"], ar["re"], ar["qb"] = 2 * self.l_pac - (p + n), 2 * self.l_pac - p, len(c3)
        else:
            read = np.concatenate([c5, seg, c3])
            ar["rb"], ar["re"], ar["qb"] = p, p + n, len(c5)
        ar["qe"] = ar["qb"] + len(seg)
        opt = opt or loader.default_mem_opt()
        if truesc is None and w2 is not None:
            truesc = truesc_for(opt, len(seg), n, w2)
        elif truesc is None:
            truesc = loader.ksw_global2_score(seg, self.g[p:p + n], max(len(seg), n) + 1, sw_opt(opt)) if len(seg) and n > 0 else 0
        ar["truesc"] = truesc
        ar["score"], ar["w"], ar["secondary"], ar["seedcov"], ar["seedlen0"] = max(int(truesc), 1), 100, -1, max(len(seg) // 2, 2), 19
        ar["sub"], ar["frac_rep"] = int(self.rng.integers(0, 20)), 0.0
        for k, v in fields.items():
            ar[k] = v
        self.reads.append(read); self.regs.append([ar]); self.tags.append(tag)
        return len(self.reads) - 1

    def more(self, r, **fields):
        """Another region of read r: a copy of its first one with other fields."""
        ar = self.regs[r][0].copy()
        for k, v in fields.items():
            ar[k] = v
        self.regs[r].append(ar)

    def bare(self, n):
        """A read without a region."""
        self.reads.append(self.rng.integers(0, 4, size=n).astype(np.uint8)); self.regs.append([]); self.tags.append("bare")
        return len(self.reads) - 1

    def extend(self, other):
        self.reads += other.reads; self.regs += other.regs; self.tags += other.tags
        return self

    def ids(self, order=None):
        """(read, region of the read) per region, for the reads in the given order."""
        order = range(len(self.reads)) if order is None else order
        return [(r, j) for r in order for j in range(len(self.regs[r]))]

    def flat(self, order=None):
        """(enc, cum, regs, reg_off, tag per region) with the reads in the given order."""
        order = range(len(self.reads)) if order is None else order
        reads = [self.reads[r] for r in order]
        cum = np.zeros(len(reads) + 1, np.int64)
        cum[1:] = np.cumsum([len(x) for x in reads])
        enc = np.concatenate(reads + [np.zeros(0, np.uint8)]).astype(np.uint8) if reads else np.zeros(0, np.uint8)
        regs = [ar for r in order for ar in self.regs[r]]
        off = np.zeros(len(reads) + 1, np.int64)
        off[1:] = np.cumsum([len(self.regs[r]) for r in order])
        tags = [self.tags[r] for r in order for _ in self.regs[r]]
        return enc, cum, (np.array(regs, loader.ALNREG_DTYPE) if regs else np.zeros(0, loader.ALNREG_DTYPE)), off, tags


def tandem_runs(g, period, min_len, limit):
    """Starts and lengths of the longest runs of g with the given period (and no shorter one), at most `limit` of them."""
    g = np.asarray(g)
    same = g[period:] == g[:-period]
    runs, i = [], 0
    while i < len(same):
        if same[i]:
            j = i
            while j < len(same) and same[j]:
                j += 1
            ln = j - i + period
            unit = g[i:i + period]
            if ln >= min_len and not any(period % d == 0 and np.array_equal(unit, np.resize(unit[:d], period)) for d in range(1, period)):
                runs.append((ln, i))
            i = j
        else:
            i += 1
    runs.sort(reverse=True)
    return [(s, ln) for ln, s in runs[:limit]]


# ---- the catalogue ---------------------------------------------------------------------------------------------------------
SPOTS = tuple(300 + 1500 * i for i in range(8))          # eight windows of up to 1 700 bases; odd ones go to the second strand
KERNEL_LQ = {"ring": 120, "wave": 300, "hbm": 600}


def _each(c, opt, n, edits_of, tag, w2=None, truesc=None, **kw):
    """The same case at the eight spots, on both strands.  edits_of(i, n) -> edits; truesc may be a function of (lq, lr)."""
    for i, p in enumerate(SPOTS):
        e = edits_of(i, n) if callable(edits_of) else edits_of
        ts = truesc
        if callable(truesc):
            lq = n + sum(x[2] if np.isscalar(x[2]) else len(x[2]) for x in e if x[0] == "I") - sum(x[2] for x in e if x[0] == "D")
            ts = truesc(lq, n)
        c.add(p + i, n, e, rev=bool(i & 1), w2=w2, truesc=ts, tag=tag, opt=opt, **kw)


def routing_cases(g, opt):
    """First-try bands 15 | 16 and 63 | 64, queries of 511 | 512 bases under a DP band, the gap-free shortcut's edge."""
    c = Cases(g, 11)
    subs = lambda i, n: [("S", 10 + 7 * i), ("S", n - 20)]                                    # noqa: E731
    for w in (15, 16):
        _each(c, opt, 100, subs, f"band{w}", w2=w)
    for w in (63, 64):
        _each(c, opt, 300, subs, f"band{w}", w2=w)
    for lq in (511, 512):
        _each(c, opt, lq + 3, lambda i, n: [("S", 30), ("D", 200 + i, 3)], f"lq{lq}", w2=20)
    edge = 2 * (opt.o_del + opt.e_del - opt.a)
    edge = min(edge, 2 * (opt.o_ins + opt.e_ins - opt.a))
    for deficit in (edge - 1, edge):                      # infer_bw returns 0 below the edge for both gap kinds: no DP
        _each(c, opt, 100, subs, f"deficit{'-' if deficit < edge else '='}edge", truesc=100 * opt.a - deficit)
    return c


def retry_cases(g, opt5, kernel):
    """Every exit of the retry loop in the kernel that finishes the region ('ring', 'wave', 'hbm').  opt5: the options with
    w = 5 (the cap 4 w = 20 is then within reach); the cases that need the default w = 100 are in retry_cases_w100."""
    c = Cases(g, 12)
    n = KERNEL_LQ[kernel]
    if kernel == "ring":
        # inferred 50, held to the region's w = 20 = 4 opt.w: one try; a query of 50 bases keeps the band at 10
        _each(c, opt5, 50, [("S", 9)], "cap@1", w2=50, w=20)
        # the issue's case: bands 5, 10, 20 from w = 5; the third outgrows the ring (requeue), and only it spans the 12-base gaps
        _each(c, opt5, 150, lambda i, n: [("I", 40 + i, 12), ("D", 90 + i, 12)], "requeue@3", w=5)
        _each(c, opt5, 150, lambda i, n: [("D", 40 + i, 12), ("I", 90 + i, 12)], "requeue@3", w=5)
        # bands 10, 20: requeue at the second try
        _each(c, opt5, 150, lambda i, n: [("I", 40 + i, 12), ("D", 90 + i, 12)], "requeue@2", w=10)
    else:
        _each(c, opt5, n, [("S", 9)], "cap@1", w2=50, w=20)
        # bands 5, 10, 20 from the ring: requeued, then finished by the wave kernel or (512 columns and more) passed on
        _each(c, opt5, n, lambda i, n: [("I", 40 + i, 12), ("D", 90 + i, 12)], "requeue@3", w=5)
        _each(c, opt5, n, lambda i, n: [("I", 40 + i, 18), ("D", 120 + i, 18)], "cap@1 gaps", w=20)
    return c


def retry_cases_w100(g, opt, kernel):
    """first try / same score / three tries with rising scores, under w = 100."""
    c = Cases(g, 13)
    n = KERNEL_LQ[kernel]
    full = lambda lq, lr: min(lq, lr) * opt.a                                                # noqa: E731
    if kernel == "ring":
        _each(c, opt, n, [("S", 30), ("D", 60, 2)], "first")                                     # truesc is the real score
        _each(c, opt, n, [("S", 30), ("D", 60, 3)], "same", truesc=full)                         # truesc out of reach: the retry changes nothing
        # bands 4, 6, 12: (5 in, 6 out) needs 5, (10 in, 10 out) then needs 9
        ed = lambda i, n: [("I", 20 + i, 5), ("D", 45 + i, 6), ("I", 70 + i, 10), ("D", 95 + i, 10)]   # noqa: E731
        _each(c, opt, n, ed, "three", truesc=lambda lq, lr: min(lq, lr) * opt.a - opt.o_ins - opt.e_ins)
        # bands 10, 20: the first misses the two gaps of 12 and falls short of truesc, the second outgrows the ring
        _each(c, opt, 150, lambda i, n: [("I", 40 + i, 12), ("D", 90 + i, 12)], "requeue", w2=10)
    else:
        _each(c, opt, n, [("S", 30), ("D", 60, 14)], "first")
        _each(c, opt, n, [("S", 30), ("D", 60, 20)], "same", truesc=full)
        ed = lambda i, n: [("I", 30 + i, 20), ("D", 90 + i, 20), ("I", 150 + i, 40), ("D", 225 + i, 40)]   # noqa: E731
        _each(c, opt, n, ed, "three", w2=16)
    return c


def geometry_cases(g, opt):
    """The wave kernel's chunks of 64 band columns, its LDS row of 512 query columns, its staged target of 1 024 bases."""
    c = Cases(g, 14)
    subs = lambda i, n: [("S", 10 + 7 * i), ("S", n - 20)]                                    # noqa: E731
    for w in (31, 32):
        _each(c, opt, 200, subs, f"cols{2 * w + 1}", w2=w)
    for w in (63, 64):
        _each(c, opt, 300, subs, f"cols{2 * w + 1}", w2=w)
    _each(c, opt, 697, lambda i, n: [("D", 100 + 40 * i, 197)], "cols401", w=1000)            # band 200: 401 columns
    # the same bands with gaps that carry the path over a chunk's last and first column (band offsets 63 | 64, 127 | 128):
    # the CIGAR of a gap-free read does not show a wrong cell there
    away = lambda k: lambda i, n: [("I", 40 + i, k), ("D", 100 + i, k), ("D", 150 + i, k), ("I", 215 + i, k)]   # noqa: E731
    _each(c, opt, 300, away(32), "cols65 gaps", w2=32)                                        # offsets 0 and 64
    _each(c, opt, 300, away(1), "cols127 gaps", w2=63)                                        # offsets 64 and 62
    _each(c, opt, 300, away(2), "cols129 gaps", w2=64)                                        # offsets 66 and 62
    _each(c, opt, 500, away(8), "cols247 gaps", w2=200, w=1000)                               # band 123 of 247 columns: offsets 131 and 115
    for lq in (1, 2):
        _each(c, opt, 24, lambda i, n: [("D", i % (lq + 1), n - lq)], f"lq{lq}")               # band |lr - lq| + 3 >= 25
    for lq in (63, 64, 65):
        _each(c, opt, lq + 15, lambda i, n: [("D", 5 + 6 * i, 15)], f"lq{lq}")
    _each(c, opt, 511, subs, "lq511", w2=20)
    for lr in (1024, 1025):                               # a deletion of more than 512 bases: the band covers every column
        _each(c, opt, lr, lambda i, n: [("D", 100 + 50 * i, n - 511 + 40), ("I", 50, 40), ("N", 20)], f"lr{lr}")
    _each(c, opt, 1100, lambda i, n: [("D", 150 + 20 * i, 700)], "lr1100")
    return c


def traceback_cases(g, opt, kernel):
    """Gap runs across the traceback window's edges, gaps at the alignment's ends, ties that the direction bits decide."""
    c = Cases(g, 15)
    n = KERNEL_LQ[kernel]
    w2 = None if kernel == "ring" else 20
    runs = (1, 5, 11, 12) if kernel == "ring" else (31, 32, 33, 64)    # the ring's band of 15 holds |lr - lq| + 3 <= 15
    for ln in runs:
        _each(c, opt, n, lambda i, n: [("D", 30 + 9 * i, ln)], f"D{ln}")      # truesc is the real score: the band is the run's + 3
        _each(c, opt, n, lambda i, n: [("I", 30 + 9 * i, ln)], f"I{ln}")
    for x in range(28, 37):                                # the walk starts at the last cell: a gap x cells before it
        g_ = 5 if kernel == "ring" else 33
        c.add(SPOTS[x % 8], n, [("D", n - x, g_)], rev=bool(x & 1), tag="Dwin", opt=opt)
        c.add(SPOTS[x % 8] + 50, n, [("I", n - x, g_)], rev=bool(x & 1), tag="Iwin", opt=opt)
        c.add(SPOTS[x % 8] + 90, n, [("D", n - 32 - x, g_)], rev=bool(x & 1), tag="Dwin2", opt=opt)
    _each(c, opt, n, [("D", 0, 3)], "D first", w2=w2)
    _each(c, opt, n, lambda i, n: [("D", n - 3, 3)], "D last", w2=w2)
    _each(c, opt, n, [("I", 0, 4)], "I first", w2=w2)
    _each(c, opt, n, lambda i, n: [("I", n, 4)], "I last", w2=w2)
    flank = (n - 20) // 2
    for period in (1, 2, 3):
        for k, (s, ln) in enumerate(tandem_runs(g[flank:len(g) - flank - 40], period, {1: 5, 2: 6, 3: 6}[period], 10)):
            s += flank
            unit = [int(v) for v in g[s:s + period]]
            # one unit out / one unit in, in the middle of the run: every placement along the run scores the same
            at = flank + period * ((ln // period) // 2)
            c.add(s - flank, 2 * flank + ln, [("D", at, period)], rev=bool(k & 1), w2=w2, tag=f"tandem{period}D", opt=opt)
            c.add(s - flank, 2 * flank + ln, [("I", at, unit)], rev=bool(k & 1), w2=w2, tag=f"tandem{period}I", opt=opt)
            c.add(s - flank, 2 * flank + ln, [("I", at, unit * 3)], rev=bool(k & 1), w2=w2, tag=f"tandem{period}I3", opt=opt)
    return c


def record_cases(g, opt):
    """Strands, clips, flags, rejected regions among good neighbours, Ns."""
    c = Cases(g, 16)
    L = len(g)
    ed = lambda i, n: [("S", 20 + i), ("D", 60 + i, 2), ("N", 90)]                                # noqa: E731
    for clip in ((7, 0), (0, 9), (5, 6)):
        _each(c, opt, 130, ed, f"clip{clip}", clip=clip)
    _each(c, opt, 130, ed, "secondary", secondary=3)
    _each(c, opt, 130, ed, "alt", n_comp_is_alt=(1 << 30) | 5)
    _each(c, opt, 130, lambda i, n: [("N", 3 + i), ("N", 4 + i), ("N", 64), ("I", 80, 3), ("N", 120)], "Ns")
    # the same records from the gap-free shortcut (aln_simple_kernel's own NM / MD, clips and position): no indel, and a truesc
    # whose deficit lies one below the edge 2 (o + e - a)
    flat = lambda i, n: [("S", 20 + i), ("N", 90), ("S", 91)]                                     # noqa: E731
    short = lambda lq, lr: lq * opt.a - 2 * (min(opt.o_del + opt.e_del, opt.o_ins + opt.e_ins) - opt.a) + 1   # noqa: E731
    for clip in ((7, 0), (0, 9), (5, 6)):
        _each(c, opt, 130, flat, f"gap-free clip{clip}", clip=clip, truesc=short)
    _each(c, opt, 130, flat, "gap-free secondary", secondary=3, truesc=short)
    _each(c, opt, 130, flat, "gap-free alt", n_comp_is_alt=(1 << 30) | 5, truesc=short)
    for i, edge in enumerate((0, 9000, 15000, L)):          # next to every boundary of the three-contig table (and the text's ends)
        for rev in (False, True):
            if edge < L:
                c.add(edge, 140, [("D", 50, 2), ("S", 9)], rev=rev, tag="contig start", opt=opt)
                c.add(edge, 140, [("D", 0, 3)], rev=rev, tag="contig start D", opt=opt)
            if edge > 0:
                c.add(edge - 140, 140, [("I", 50, 2), ("S", 9)], rev=rev, tag="contig end", opt=opt)
                c.add(edge - 140, 140, [("S", 9), ("N", 139)], rev=rev, truesc=short(140, 140), tag="gap-free contig end", opt=opt)
            if edge < L:
                c.add(edge, 140, [("S", 9), ("N", 0)], rev=rev, truesc=short(140, 140), tag="gap-free contig start", opt=opt)
    bad = (dict(rb=L - 50, re=L + 80), dict(rb=-5, re=125), dict(qe=0, qb=0), dict(rb=2 * L - 100, re=2 * L + 30),
           dict(rb=L + 10, re=L + 10 + (1 << 20) + 1), dict(rb=5000, re=5000), dict(rb=-1, re=-1), dict(rb=700, re=-3))
    for i, b in enumerate(bad):                            # each between two good regions of the same read, and alone in a read
        r = c.add(SPOTS[i], 130, [("D", 60, 2)], rev=bool(i & 1), clip=(3, 4), tag="good", opt=opt)
        c.more(r, **b)
        c.more(r, secondary=0)
        c.tags[r] = "bad among good"
        r = c.add(SPOTS[i] + 200, 90, [("S", 11)], tag="bad alone", opt=opt, **b)
    return c



# Windows with short stretches replaced by other bases of another length, found by a search on the CPU (random such edits, kept
# where turning the tie rule of the deletion's or the insertion's "extended | opened" comparison changes the oracle's CIGAR under
# the default scoring; ties_of says which).  Such a tie needs two ways across a stretch that score the same and differ in where
# a gap of two or more bases opens, which edits made for another purpose hardly ever produce.  (window start, second strand, edits)
TIE_TABLE = {
    "ring": (
        (14887, 0, (('D', 9, 5), ('I', 9, 'C'), ('D', 21, 6), ('I', 21, 'CCTCA'))),
        (11664, 0, (('D', 15, 8), ('I', 15, 'CTG'), ('D', 27, 1), ('I', 27, 'CCG'))),
        (5135, 0, (('D', 11, 7), ('I', 11, 'GTCGAG'))),
        (13130, 1, (('D', 12, 8), ('I', 12, 'CTTCGTGA'), ('D', 25, 1), ('I', 25, 'CG'))),
        (11221, 1, (('D', 9, 5), ('I', 9, 'GAG'), ('D', 19, 8), ('I', 19, 'CAATC'))),
        (11205, 1, (('D', 6, 5), ('I', 6, 'ATCT'), ('D', 15, 5), ('I', 15, 'TT'), ('D', 24, 3), ('I', 24, 'CTAATGGG'))),
        (16787, 0, (('D', 11, 7), ('D', 22, 2), ('I', 22, 'CTG'))),
        (4577, 0, (('D', 19, 3), ('I', 19, 'A'), ('D', 26, 8), ('I', 26, 'CACAAGCG'))),
        (13527, 1, (('D', 13, 3), ('I', 13, 'G'), ('D', 23, 4), ('I', 23, 'GATGGA'))),
        (10067, 0, (('D', 9, 5), ('I', 9, 'AAAT'), ('D', 22, 2), ('I', 22, 'TTAG'))),
        (12904, 0, (('I', 13, 'TTA'), ('D', 26, 5), ('I', 26, 'TGCGGCCT'))),
        (569, 0, (('D', 9, 4), ('I', 9, 'GTGGC'), ('D', 24, 7), ('I', 24, 'TAT'))),
        (9359, 0, (('D', 17, 3), ('I', 17, 'GGC'), ('D', 26, 4), ('I', 26, 'TCGCTCTG'))),
        (1052, 0, (('D', 6, 6), ('I', 6, 'AGTTA'), ('D', 25, 8), ('I', 25, 'GGATTCTC'))),
        (3288, 1, (('D', 12, 8), ('I', 12, 'A'), ('D', 25, 6), ('I', 25, 'ACGAAACT'))),
        (19016, 0, (('D', 16, 4), ('I', 16, 'CGGAACG'), ('D', 25, 8), ('I', 25, 'TG'))),
        (15985, 1, (('D', 19, 8), ('I', 19, 'ACGCAGAA'))),
        (4296, 1, (('D', 6, 2), ('I', 6, 'T'), ('D', 17, 5), ('I', 17, 'CTACT'), ('D', 27, 2), ('I', 27, 'GATCCTCA'))),
        (374, 1, (('D', 7, 1), ('I', 7, 'ACCCCA'), ('D', 13, 1), ('I', 13, 'TGTTAT'), ('D', 20, 7), ('I', 20, 'C'))),
        (2091, 0, (('D', 17, 4), ('I', 17, 'CCGATATT'), ('D', 26, 2), ('I', 26, 'GAGA'))),
    ),
    "wave": (
        (1747, 0, (('D', 19, 4), ('I', 19, 'GTCT'), ('I', 36, 'CACCGATA'), ('D', 45, 7), ('D', 64, 7), ('I', 64, 'AGTCTC'))),
        (3717, 1, (('D', 9, 8), ('I', 9, 'GGCAGCC'), ('D', 23, 3), ('I', 23, 'AGCCGTA'), ('D', 37, 4), ('I', 37, 'A'))),
        (4571, 0, (('D', 5, 8), ('I', 5, 'AAG'), ('D', 25, 3), ('I', 25, 'GGAA'), ('D', 35, 2), ('I', 35, 'CATT'))),
        (892, 1, (('I', 17, 'CATCTTA'), ('D', 21, 6), ('I', 32, 'CTCAGGGT'), ('D', 41, 7), ('I', 58, 'CTATGA'), ('D', 64, 8), ('I', 64, 'GCCAG'))),
        (6181, 1, (('D', 9, 1), ('I', 9, 'CTAAGC'), ('D', 25, 7), ('I', 25, 'GGGTAT'), ('D', 37, 8), ('I', 37, 'CGTAAA'))),
        (671, 0, (('I', 14, 'AGATG'), ('D', 24, 4), ('I', 24, 'TA'), ('D', 32, 5), ('D', 46, 2), ('I', 46, 'G'))),
        (18154, 1, (('D', 17, 7), ('I', 17, 'CTGCAATA'), ('D', 34, 8), ('I', 34, 'GAC'), ('D', 49, 3), ('I', 49, 'ATAAGG'))),
        (8324, 0, (('I', 12, 'ATAGG'), ('D', 25, 4), ('I', 25, 'GCCCAA'), ('D', 39, 6), ('I', 39, 'TTTGGAAC'), ('D', 52, 7), ('I', 52, 'ACT'))),
        (5974, 0, (('D', 16, 6), ('I', 16, 'CCT'), ('D', 35, 6), ('I', 35, 'AT'), ('D', 53, 1), ('I', 53, 'TCCCGGG'))),
        (10546, 1, (('D', 9, 8), ('I', 9, 'TTAACTTC'), ('D', 21, 7), ('I', 21, 'ATCGGA'), ('D', 32, 4), ('I', 32, 'AAGGAA'))),
        (16571, 1, (('D', 19, 6), ('I', 35, 'ATCG'), ('D', 39, 2), ('I', 39, 'GGGG'), ('D', 47, 4), ('I', 47, 'AAA'))),
        (4955, 1, (('D', 6, 2), ('I', 6, 'TCAGCCAG'), ('D', 14, 3), ('I', 14, 'A'), ('D', 23, 7), ('D', 40, 3), ('I', 40, 'A'))),
        (705, 0, (('D', 14, 1), ('I', 14, 'CCG'), ('D', 24, 3), ('I', 24, 'GGATCTG'), ('D', 47, 8), ('I', 47, 'C'))),
        (16657, 1, (('D', 9, 8), ('I', 9, 'ACGAGC'), ('D', 26, 2), ('I', 26, 'TACCCTT'), ('D', 32, 7), ('I', 32, 'T'))),
        (16268, 1, (('I', 8, 'CGT'), ('D', 12, 7), ('D', 27, 7), ('I', 27, 'GCGCCACT'), ('I', 38, 'GGACTC'), ('D', 44, 2), ('I', 44, 'AGTC'))),
        (10608, 1, (('D', 9, 2), ('I', 9, 'ATC'), ('D', 15, 3), ('I', 15, 'GCTCGG'), ('D', 28, 3), ('D', 44, 7), ('I', 44, 'GCCCGAT'))),
        (15365, 0, (('I', 11, 'AGTC'), ('D', 21, 6), ('I', 21, 'CGATGAG'), ('D', 35, 5), ('I', 35, 'G'), ('D', 49, 6))),
        (9946, 1, (('D', 18, 5), ('I', 18, 'GATTTAGT'), ('D', 32, 4), ('I', 32, 'CGAATC'), ('D', 46, 7), ('I', 46, 'CAACATCC'))),
        (11477, 0, (('D', 11, 6), ('I', 11, 'GACGCCG'), ('D', 30, 8), ('I', 30, 'AGACGCT'), ('D', 47, 5), ('I', 47, 'TTCAAC'))),
        (1643, 0, (('I', 16, 'TGCCGT'), ('D', 21, 8), ('I', 21, 'CCAAA'), ('D', 39, 6), ('D', 51, 2), ('D', 63, 2), ('I', 63, 'GCGTG'))),
    ),
    "hbm": (
        (3328, 1, (('D', 6, 4), ('I', 6, 'CTCAA'), ('D', 21, 7), ('I', 21, 'TGATA'), ('D', 36, 8), ('I', 36, 'ATTGT'))),
        (8639, 1, (('D', 16, 5), ('I', 16, 'TGG'), ('D', 26, 8), ('I', 26, 'GCCAGTAG'), ('D', 44, 5), ('I', 44, 'CTAGGA'))),
        (1934, 1, (('I', 8, 'GTTAGCCG'), ('D', 13, 8), ('I', 13, 'GAAA'), ('D', 27, 6), ('I', 27, 'C'), ('D', 38, 5))),
        (9810, 1, (('D', 7, 5), ('I', 7, 'GG'), ('D', 18, 6), ('I', 18, 'CTT'), ('D', 28, 7), ('I', 28, 'GACGTCGC'))),
        (10087, 1, (('D', 19, 6), ('D', 38, 7), ('I', 38, 'TGGACTAC'), ('D', 55, 2), ('I', 55, 'GAC'), ('D', 61, 4), ('I', 61, 'TAAG'))),
        (17181, 1, (('D', 19, 8), ('I', 19, 'GAA'), ('D', 35, 6), ('I', 35, 'TAAGATGA'), ('D', 45, 8), ('I', 45, 'GGACGCTT'))),
        (15847, 1, (('D', 11, 6), ('I', 11, 'GCAT'), ('D', 29, 3), ('I', 29, 'CTTTACCC'), ('D', 44, 8), ('I', 44, 'GCATA'))),
        (1384, 1, (('D', 7, 2), ('I', 7, 'GTAC'), ('D', 22, 4), ('I', 22, 'ATGCAGC'), ('D', 37, 6), ('I', 37, 'GTAC'))),
        (4193, 1, (('D', 18, 6), ('I', 18, 'TGA'), ('D', 31, 7), ('I', 31, 'GTCAGGCC'), ('D', 42, 1), ('I', 42, 'AAG'))),
        (13108, 1, (('D', 11, 7), ('I', 11, 'C'), ('D', 23, 2), ('I', 23, 'TGGCATCG'), ('D', 32, 8), ('I', 32, 'GACACA'))),
        (2726, 1, (('D', 19, 8), ('I', 19, 'GTC'), ('D', 33, 7), ('I', 33, 'TGGGAA'), ('D', 47, 5), ('I', 47, 'GCTGCCC'))),
        (15256, 0, (('D', 18, 5), ('I', 18, 'TTT'), ('D', 29, 5), ('I', 29, 'GATTACT'), ('D', 38, 6), ('I', 38, 'G'))),
        (9870, 0, (('D', 13, 7), ('I', 25, 'TTT'), ('D', 30, 1), ('I', 30, 'AGGGCCAA'), ('D', 37, 4), ('I', 37, 'CACGATA'))),
        (3751, 1, (('D', 16, 6), ('I', 16, 'T'), ('D', 35, 5), ('I', 35, 'GTCGCCGT'), ('I', 45, 'CCTT'), ('D', 50, 3), ('I', 50, 'AACA'))),
        (17607, 1, (('D', 13, 7), ('I', 13, 'GCAC'), ('I', 28, 'CTTCATGT'), ('D', 40, 7), ('I', 40, 'AGTAA'), ('D', 51, 5), ('I', 51, 'GG'))),
        (11000, 1, (('D', 9, 4), ('I', 9, 'GGGCAA'), ('D', 24, 4), ('I', 24, 'GGCTACCG'), ('D', 36, 7), ('I', 36, 'AGGCC'))),
        (14160, 1, (('D', 8, 7), ('D', 23, 4), ('I', 23, 'CCTAG'), ('D', 36, 4), ('I', 36, 'TATGG'), ('D', 53, 3), ('I', 53, 'CGGTTAG'))),
        (6936, 0, (('D', 5, 4), ('I', 5, 'ATCGTTAC'), ('D', 15, 6), ('I', 15, 'ATC'), ('D', 28, 8), ('I', 28, 'ACC'))),
        (15876, 1, (('D', 5, 7), ('I', 5, 'GTCA'), ('I', 25, 'AGTGAA'), ('D', 30, 5), ('I', 30, 'CTA'), ('D', 46, 3), ('I', 46, 'TAACAT'))),
        (3614, 0, (('D', 5, 4), ('I', 5, 'TTATTA'), ('D', 14, 2), ('I', 14, 'A'), ('D', 29, 5), ('I', 29, 'GGCGC'))),
    ),
}


def tie_cases(g, opt, kernel):
    """The regions of TIE_TABLE for the kernel that finishes them: 50, 300 and 600 bases (bwa_gen_cigar2 holds the band of a
    50-base query to the ring's 15; the others are steered to a band of 20)."""
    c = Cases(g, 17)
    n = {"ring": 50, "wave": 300, "hbm": 600}[kernel]
    for p, rev, edits in TIE_TABLE[kernel]:
        ed = [(e[0], e[1], e[2] if e[0] == "D" else ["ACGT".index(x) for x in e[2]]) for e in edits]
        c.add(p, n, ed, rev=bool(rev), w2=None if kernel == "ring" else 20, tag="ties", opt=opt)
    return c
