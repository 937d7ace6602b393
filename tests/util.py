"""Shared fixtures: small seeded genomes/indexes/reads, cached per process."""
from __future__ import annotations

import functools

import numpy as np

from bwams import fmindex, simulate


@functools.lru_cache(maxsize=None)
def toy(n_bases: int = 20000, seed: int = 7, repeat_frac: float = 0.15):
    g = simulate.make_genome(n_bases, seed=seed, repeat_frac=repeat_frac, repeat_len=200, n_families=3)
    idx = fmindex.build_fmindex(g)
    return g, idx


@functools.lru_cache(maxsize=None)
def toy_reads(n_bases: int = 20000, n_reads: int = 300, seed: int = 11):
    g, idx = toy(n_bases)
    reads, pos, rev = simulate.make_reads(g, n_reads, seed=seed)
    return reads, pos, rev


def naive_sa(text: np.ndarray) -> np.ndarray:
    """Suffix array of text+'$' by direct comparison (small inputs only)."""
    n = len(text)
    b = bytes((text + 1).astype(np.uint8)) + b"\x00"
    return np.array(sorted(range(n + 1), key=lambda i: b[i:]), dtype=np.int64)


def make_pairs(n: int, seed: int = 5, max_q: int = 140, max_extra_t: int = 120, n_frac: float = 0.02,
               h0_max: int = 150):
    """Random extension tasks in the reference's SeqPair layout.

    Targets are mutated copies of the query (substitutions, indels, or unrelated
    tails) so that every exit path of the DP is exercised: z-drop, band shrink,
    row maximum reaching zero, reaching the query end (gscore)."""
    from oracle.loader import SEQPAIR_DTYPE
    rng = np.random.default_rng(seed)
    pairs = np.zeros(n, dtype=SEQPAIR_DTYPE)
    refs, qers = [], []
    ro = qo = 0
    for i in range(n):
        ql = int(rng.integers(1, max_q + 1))
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        mode = rng.integers(0, 5)
        t = list(q)
        if mode >= 1:
            rate = [0.0, 0.02, 0.08, 0.2, 0.5][mode]
            out = []
            for b in t:
                u = rng.random()
                if u < rate * 0.6:
                    out.append((b + rng.integers(1, 4)) & 3)
                elif u < rate * 0.8:
                    continue
                elif u < rate:
                    out.extend([b, rng.integers(0, 4)])
                else:
                    out.append(b)
            t = out
        if rng.random() < 0.3:                     # a long gap somewhere
            cut = int(rng.integers(0, len(t) + 1))
            gap = int(rng.integers(1, 40))
            if rng.random() < 0.5:
                t = t[:cut] + list(rng.integers(0, 4, size=gap)) + t[cut:]
            else:
                t = t[:cut] + t[cut + gap:]
        t = t + list(rng.integers(0, 4, size=int(rng.integers(0, max_extra_t))))
        if len(t) == 0:
            t = [0]
        t = np.array(t, dtype=np.uint8)
        nmask = rng.random(len(t)) < n_frac
        t[nmask] = 4
        q = q.copy()
        q[rng.random(ql) < n_frac] = 4
        pairs[i]["idr"], pairs[i]["idq"], pairs[i]["id"] = ro, qo, i
        pairs[i]["len1"], pairs[i]["len2"] = len(t), ql
        pairs[i]["h0"] = int(rng.integers(1, h0_max + 1))
        pairs[i]["seqid"], pairs[i]["regid"] = i // 3, i % 3
        refs.append(t); qers.append(q)
        ro += len(t); qo += ql
    return pairs, np.concatenate(refs), np.concatenate(qers)


OUT_FIELDS = ("score", "tle", "gtle", "qle", "gscore", "max_off")


def assert_pairs_equal(a, b, what=""):
    for f in OUT_FIELDS:
        bad = np.flatnonzero(a[f] != b[f])
        assert bad.size == 0, f"{what}: field {f} differs at {bad[:5]}: {a[f][bad[:5]]} vs {b[f][bad[:5]]}; pair={a[bad[0]]}"


def make_local_cases(n: int, seed: int = 9, qmax: int = 151, tmax: int = 900):
    """(query, target) pairs shaped like mate rescue: a (mutated, possibly truncated) copy of the
    query somewhere in a longer random window, sometimes twice (second-best hit), sometimes not at all."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ql = int(rng.integers(20, qmax + 1))
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        tl = int(rng.integers(ql, tmax))
        t = rng.integers(0, 4, size=tl, dtype=np.uint8)

        def mutated():
            rate = float(rng.choice([0.0, 0.02, 0.06, 0.15]))
            o = []
            for b in q:
                u = rng.random()
                if u < rate * 0.6:
                    o.append((b + rng.integers(1, 4)) & 3)
                elif u < rate * 0.8:
                    continue
                elif u < rate:
                    o.extend([b, rng.integers(0, 4)])
                else:
                    o.append(b)
            a = int(rng.integers(0, max(1, len(o) // 3)))
            z = int(rng.integers(0, max(1, len(o) // 3)))
            return np.array(o[a: len(o) - z], dtype=np.uint8)
        k = int(rng.choice([0, 1, 1, 1, 2, 3]))
        for _c in range(k):
            c = mutated()
            if len(c) and len(c) < tl:
                st = int(rng.integers(0, tl - len(c) + 1))
                t[st: st + len(c)] = c
        if rng.random() < 0.1:
            t[rng.integers(0, tl, size=3)] = 4
        if rng.random() < 0.1:
            q[rng.integers(0, ql, size=2)] = 4
        out.append((q, t))
    return out


def oracle_pe_pipeline(g, idx, reads, contigs=None, opt=None):
    """Run the CPU oracle from reads to final regions (+ insert-size statistics) for a chunk of read pairs.
    Returns a dict with enc, cum, ref, regs, reg_off, pes."""
    from bwams import simulate
    from oracle import loader
    enc, cum = simulate.flatten_reads(reads)
    opt = opt or loader.default_mem_opt()
    o = loader.OracleFMI(idx)
    sm = o.collect_smem(enc, cum)
    coord, off = o.sa_lookup(sm)
    l_pac = len(g)
    ref = np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])
    ch, sd, choff = loader.chain_seeds(sm, coord, off, cum, l_pac, contigs=contigs, opt=opt, ref_string=ref, enc=enc)
    regs, reg_off, _ = loader.chain2aln(ch, sd, choff, enc, cum, ref, l_pac, contigs=contigs, opt=opt)
    fin, fin_off = loader.regs_finish(regs, reg_off, enc, cum, ref, l_pac, contigs=contigs, opt=opt)
    pes = loader.pestat(fin, fin_off, l_pac, opt=opt)
    return dict(enc=enc, cum=cum, ref=ref, l_pac=l_pac, regs=fin, reg_off=fin_off, pes=pes, opt=opt, sm=sm, coord=coord, off=off)



def ert_mems_from_smems(sm, all_coord, all_off, nseq, l_pac, seed=0, shuffle=True, backward_frac=0.4, dup_frac=0.05):
    """Dress FM-index SMEMs up as the output of the reference's ERT walk (mem_t records + per-read hit arrays).

    all_coord / all_off hold EVERY occurrence of each SMEM (SA lookup with max_occ = infinity), in BWT-row order, so
    that mem_chain_new's strided pick (hits[hitbeg + k], k = 0, step, ..) sees the rows get_sa_entries would.  A
    backward_frac of the MEMs are marked "found by backward search": their hits are stored as the walk stores them
    (position of the reverse-complemented match, off by end_correction) and mem_chain_new maps them back.  MEMs are
    shuffled within a read (the reference sorts them) and a few are duplicated (ties for the unstable sort)."""
    from oracle import loader
    rng = np.random.default_rng(seed)
    mems, hits, mem_off, hit_off = [], [], [0], [0]
    order = np.argsort(sm["rid"], kind="stable")
    by_read = [[] for _ in range(nseq)]
    for i in order:
        by_read[int(sm["rid"][i])].append(int(i))
    for r in range(nseq):
        idxs = list(by_read[r])
        idxs += [i for i in idxs if rng.random() < dup_frac]
        if shuffle:
            rng.shuffle(idxs)
        hb = 0
        for i in idxs:
            pos = all_coord[all_off[i]:all_off[i + 1]].astype(np.int64)
            m = np.zeros(1, loader.ERT_MEM_DTYPE)[0]
            m["start"], m["end"] = int(sm["m"][i]), int(sm["n"][i]) + 1
            slen = int(m["end"]) - int(m["start"])
            m["hitbeg"], m["hitcount"] = hb, len(pos)
            kind = rng.random()
            if kind < backward_frac:
                m["forward"], m["fetch_leaves"] = 0, 0
                m["end_correction"] = int(rng.integers(0, 4))
                stored = 2 * l_pac - pos - slen + int(m["end_correction"])
            elif kind < backward_frac + 0.2:
                m["forward"], m["fetch_leaves"] = 0, 1
                stored = pos
            else:
                m["forward"] = 1
                stored = pos
            hits.append(stored.astype(np.uint64))
            hb += len(pos)
            mems.append(m)
        mem_off.append(len(mems))
        hit_off.append(hit_off[-1] + hb)
    mems = np.array(mems, dtype=loader.ERT_MEM_DTYPE) if mems else np.zeros(0, loader.ERT_MEM_DTYPE)
    hits = np.concatenate(hits) if hits else np.zeros(0, np.uint64)
    return mems, np.array(mem_off, np.int64), hits, np.array(hit_off, np.int64)


def seeds_equal_but_junction(got, gcoord, goff, want, wcoord, woff, cum, l_pac):
    """Seeding results (SMEM records in (rid, m, n) order + sampled coordinates) of two statements of ERT-mode seeding
    must be identical read by read, EXCEPT for reads with a hit whose placement crosses the junction between the two
    strands of the text: there the reference's get_seq (ertseeding.cpp:455-472) hands leaf expansion nothing and its walk
    emits non-maximal matches, which FM-index seeding and the HIP path do not reproduce
    (tests/test_oracle_ert_walk.py::test_strand_junction_is_the_only_difference).  Returns the differing reads."""
    import collections

    def per_read(sm, co, of):
        d = collections.defaultdict(list)
        rid, m, n, s = sm["rid"], sm["m"], sm["n"], sm["s"]
        for t in range(len(sm)):
            d[int(rid[t])].append((int(m[t]), int(n[t]), int(s[t]), tuple(int(x) for x in co[of[t]:of[t + 1]])))
        return d

    if (len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("rid", "m", "n", "s"))
            and np.array_equal(goff, woff) and np.array_equal(gcoord, wcoord)):
        return []
    A, B = per_read(got, gcoord, goff), per_read(want, wcoord, woff)
    bad = sorted(r for r in set(A) | set(B) if A.get(r) != B.get(r))
    for r in bad:
        ln = int(cum[r + 1] - cum[r])
        placements = [p - m for (m, n, s, ps) in A.get(r, []) + B.get(r, []) for p in ps]
        assert any(p < l_pac < p + ln for p in placements), f"read {r}: {A.get(r)} != {B.get(r)}"
    return bad


# ---- banded-SW task sets at scale (tests/test_gpu_bsw.py): numpy per sequence, no loop over bases -------------------------
def pack_pairs(queries, targets, h0):
    """A SeqPair array and the flat (ref, qer) buffers of lists of query / target code arrays and their initial scores."""
    from oracle.loader import SEQPAIR_DTYPE
    n = len(queries)
    ql = np.array([len(q) for q in queries], np.int64)
    tl = np.array([len(t) for t in targets], np.int64)
    pairs = np.zeros(n, dtype=SEQPAIR_DTYPE)
    pairs["idq"] = np.concatenate([[0], np.cumsum(ql)[:-1]]) if n else []
    pairs["idr"] = np.concatenate([[0], np.cumsum(tl)[:-1]]) if n else []
    pairs["id"] = np.arange(n)
    pairs["len1"], pairs["len2"], pairs["h0"] = tl, ql, h0
    pairs["seqid"], pairs["regid"] = np.arange(n) // 3, np.arange(n) % 3
    cat = lambda xs: np.concatenate([np.asarray(x, np.uint8) for x in xs] + [np.zeros(1, np.uint8)])   # never empty
    return pairs, cat(targets), cat(queries)


def mutate(rng, q, rate: float):
    """q with substitutions (0.6 rate), deletions (0.2 rate) and duplicated bases (0.2 rate), as make_pairs draws them."""
    u = rng.random(len(q))
    sub = u < rate * 0.6
    t = q.copy()
    t[sub] = (t[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
    keep = ~((u >= rate * 0.6) & (u < rate * 0.8))
    dup = (u >= rate * 0.8) & (u < rate)
    return np.repeat(t, keep.astype(np.int64) + dup)


def make_task_pool(n: int, qlen_lo: int, qlen_hi: int, seed: int, tlen_max: int = 2000, h0_max: int = 150,
                   n_frac: float = 0.02):
    """n extension tasks with query lengths spread over [qlen_lo, qlen_hi] (both ends included) and targets from 0 to
    tlen_max bases: mutated copies of the query at make_pairs' rates, sometimes with a long gap, or unrelated bases, followed
    by a random tail.  Lifetimes then range from one row (an unrelated target, a row maximum of 0) to several hundred rows of
    a band that spans several 32-column windows (an exact copy with a long tail); z-drop exits and full runs both occur.
    Returns (queries, targets, h0)."""
    rng = np.random.default_rng(seed)
    qls = np.concatenate([[qlen_lo, qlen_hi], rng.integers(qlen_lo, qlen_hi + 1, size=max(n - 2, 0))])[:n]
    queries, targets = [], []
    for ql in qls:
        q = rng.integers(0, 4, size=int(ql), dtype=np.uint8)
        kind = rng.integers(0, 7)
        if kind == 6:
            t = rng.integers(0, 4, size=int(rng.integers(0, tlen_max + 1)), dtype=np.uint8)
        else:
            t = mutate(rng, q, [0.0, 0.0, 0.02, 0.08, 0.2, 0.5][kind])
            if rng.random() < 0.3 and len(t):                     # a long gap somewhere
                cut, gap = int(rng.integers(0, len(t) + 1)), int(rng.integers(1, 40))
                t = (np.concatenate([t[:cut], rng.integers(0, 4, size=gap, dtype=np.uint8), t[cut:]]) if rng.random() < 0.5
                     else np.concatenate([t[:cut], t[cut + gap:]]))
            tail = int(rng.choice([0, rng.integers(0, 120), rng.integers(0, tlen_max + 1)]))
            t = np.concatenate([t, rng.integers(0, 4, size=tail, dtype=np.uint8)])[:tlen_max]
        if rng.random() < 0.03:
            t = t[:0]
        t = t.copy()
        t[rng.random(len(t)) < n_frac] = 4
        q[rng.random(len(q)) < n_frac] = 4
        queries.append(q)
        targets.append(t)
    return queries, targets, rng.integers(1, h0_max + 1, size=n)


def bsw_class(qlen, h0, max_sc: int):
    """bsw_class_of (csrc/bsw_extend.hip) restated: classes 0-4 by query length for the packed kernels, 5 for the rest
    (queries of more than 191 bases, a score bound h0 + qlen * max_sc of 2^14 or more, h0 < 0)."""
    qlen, h0 = np.asarray(qlen, np.int64), np.asarray(h0, np.int64)
    cls = np.searchsorted(np.array([31, 63, 95, 143, 191]), qlen, side="left")
    cls[(qlen > 191) | (h0 + qlen * max_sc >= 1 << 14) | (h0 < 0)] = 5
    return cls


# ---- the edge families of the banded-SW tests: the oracle is pinned to the reference on exactly these inputs
# (tests/test_oracle_bsw.py), the GPU kernels to the oracle (tests/test_gpu_bsw.py)
BSW_LIMIT = 1 << 14                   # scores of the packed classes stay below it
BSW_CLASS_EDGES = (1, 31, 32, 63, 64, 95, 96, 143, 144, 191, 192)
BSW_WIDE_W = (0, 1, 2, 31, 32, 33, 64, 100, 200, 700)
# (a, (o_del, e_del, o_ins, e_ins), score against N) at the edge of what bsw_pk_kernel takes (bsw_pk_eligible)
BSW_SCORING_EDGES = (
    (1, (6, 64, 6, 64), -1), (5, (6, 64, 6, 64), -1),            # e = 64: packed
    (1, (6, 65, 6, 65), -1), (5, (6, 64, 6, 65), -1),            # e = 65: the eight-task kernel
    (1, (7935, 64, 7935, 64), -1), (1, (7998, 1, 7998, 1), -1),  # o + e = 7999: packed
    (1, (7936, 64, 6, 1), -1), (1, (7999, 1, 7999, 1), -1),      # o + e = 8000: the eight-task kernel
    (1, (6, 1, 6, 1), 0), (2, (6, 1, 6, 1), -2),                 # N scored 0 / -2: the eight-task kernel
)


def bsw_sw_opt(mod, end_bonus=5, a=1, b=4, zdrop=100, gaps=None, n_score=-1):
    """mod.default_sw_opt (mod: oracle.loader or bwams.capi) with other gap costs and another score against N."""
    o = mod.default_sw_opt(end_bonus, a, b)
    o.zdrop = zdrop
    if gaps:
        o.o_del, o.e_del, o.o_ins, o.e_ins = gaps
    for k in range(5):
        o.mat[k * 5 + 4] = o.mat[4 * 5 + k] = n_score
    return o


def bsw_class_edge_tasks(seed: int):
    """qlen at every class edge (and 0), tlen 0, 1, qlen and 3000: the query itself, a mutated copy or unrelated bases."""
    rng = np.random.default_rng(seed)
    qs, ts, hs = [], [], []
    for ql in (0,) + BSW_CLASS_EDGES:
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        for tl in sorted({0, 1, ql, 3000}):
            tail = rng.integers(0, 4, size=tl, dtype=np.uint8)
            for t in (np.concatenate([q, tail]), np.concatenate([mutate(rng, q, 0.08), tail]), tail):
                for h0 in (1, 20, 100):
                    qs.append(q); ts.append(t[:tl]); hs.append(h0)
    return pack_pairs(qs, ts, hs)


def bsw_score_limit_tasks(a: int):
    """Identical query and target, so that the score climbs to h0 + qlen * a, with h0 putting that bound at 2^14 - 1 (the
    largest score the packed kernels hold), 2^14, 2^14 + 1 and 2^15 - 1 (beyond what 16-bit lanes hold) at every class edge;
    the same pair with a mismatch or an N as the last base; h0 far beyond the bound (2^15, 2^16 + 7, 10^6), 0 and negative."""
    rng = np.random.default_rng(a)
    qs, ts, hs = [], [], []
    for ql in BSW_CLASS_EDGES:
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        mis, tn, qn = q.copy(), q.copy(), q.copy()
        mis[-1] = (mis[-1] + 1) & 3
        tn[-1] = qn[-1] = 4
        h0s = [BSW_LIMIT - 1 - ql * a + d for d in (0, 1, 2)] + [(1 << 15) - 1 - ql * a, 0, 1 << 15, (1 << 16) + 7, 10 ** 6, -1, -37]
        for qq, t in ((q, q), (q, mis), (q, tn), (qn, q)):
            for extra in (0, 60):
                tt = np.concatenate([t, rng.integers(0, 4, size=extra, dtype=np.uint8)])
                for h0 in h0s:
                    qs.append(qq); ts.append(tt); hs.append(h0)
    return pack_pairs(qs, ts, hs)


def bsw_wide_band_tasks():
    """Homopolymers and (AC)^n against themselves: every cell of a wide band is positive, a row spans several 32-column windows."""
    qs, ts, hs = [], [], []
    for ql in (20, 64, 150, 191, 250, 600):
        for unit in (np.zeros(ql, np.uint8), np.resize(np.array([0, 1], np.uint8), ql)):
            for tl in (ql, ql + 40, 2 * ql):
                for h0 in (40, 400):
                    qs.append(unit); ts.append(np.resize(unit, tl)); hs.append(h0)
    return pack_pairs(qs, ts, hs)


def bsw_n_run_tasks():
    """Runs of N in the query, in the target or in both; all-N queries against bases and against N."""
    rng = np.random.default_rng(11)
    q0, t0, h = make_task_pool(600, 1, 300, seed=12, tlen_max=500)
    qs, ts = [], []
    for k, (q, t) in enumerate(zip(q0, t0)):
        q, t = q.copy(), t.copy()
        for s, where in ((q, k % 3 != 1), (t, k % 3 != 0)):
            if where and len(s):
                for _ in range(int(rng.integers(1, 4))):
                    st = int(rng.integers(0, len(s)))
                    s[st:st + int(rng.integers(1, 25))] = 4
        qs.append(q); ts.append(t)
    for ql in (1, 31, 40, 191, 250):
        qs += [np.full(ql, 4, np.uint8)] * 2
        ts += [rng.integers(0, 4, size=ql + 10, dtype=np.uint8), np.full(ql, 4, np.uint8)]
        h = np.concatenate([h, [50, 50]])
    return pack_pairs(qs, ts, h)


def bsw_scoring_edge_tasks(a: int, seed: int):
    """make_pairs tasks (queries up to 191 bases, 5 % N), and exact or gapped copies whose score ends at the packed bound."""
    pairs, ref, qer = make_pairs(600, seed=seed, max_q=191, max_extra_t=200, n_frac=0.05)
    tasks = [(qer[p["idq"]:p["idq"] + p["len2"]], ref[p["idr"]:p["idr"] + p["len1"]], int(p["h0"])) for p in pairs]
    rng = np.random.default_rng(a)
    for ql in (31, 95, 143, 191):
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        for t in (q, np.concatenate([q[:ql // 2], q[ql // 2 + 3:], q[:20]]), np.concatenate([q[:50], [0, 1, 2], q[50:]])):
            tasks.append((q, t, BSW_LIMIT - 1 - ql * a))
    return pack_pairs([x[0] for x in tasks], [x[1] for x in tasks], [x[2] for x in tasks])
