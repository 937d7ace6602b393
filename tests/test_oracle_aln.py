"""The SAM-side alignment step of the oracle (oracle/aln_oracle.c).  ksw_global2 with its traceback is PINNED to the
reference's ksw.cpp object; bwa_gen_cigar2 / mem_reg2aln (bwa.cpp / bwamem.cpp, not buildable here) are checked through
properties: the CIGAR consumes exactly the query and reference spans, NM and MD are recomputed independently; their band
inference, retry loop, squeeze and clips against a second restatement over the pinned ksw_global2 (tests/aln_cases.py)."""
import numpy as np

import aln_cases as ac
from bwams import simulate
from oracle import loader
from ref_answers import Answers
from util import toy

REF = loader.ref_lib()


def _pairs(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        ql = int(rng.integers(1, 160))
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        t = list(q)
        rate = float(rng.choice([0.0, 0.02, 0.1, 0.3]))
        o = []
        for b in t:
            u = rng.random()
            if u < rate * 0.5:
                o.append((b + rng.integers(1, 4)) & 3)
            elif u < rate * 0.75:
                continue
            elif u < rate:
                o.extend([b, rng.integers(0, 4)])
            else:
                o.append(b)
        if not o:
            o = [0]
        t = np.array(o, np.uint8)
        if rng.random() < 0.1:
            q[rng.integers(0, ql)] = 4
        w = int(rng.choice([0, 1, 3, 8, 20, 100, 400]))
        yield q, t, max(w, abs(len(t) - ql))            # the band must reach the last cell, as bwa_gen_cigar2's min_w ensures


def test_global_alignment_with_traceback_equals_reference():
    ans = Answers(REF is not None)
    for opt in (loader.default_sw_opt(), loader.default_sw_opt(5, 2, 3)):
        if opt.mat[0] == 2:
            opt.o_del, opt.e_del, opt.o_ins, opt.e_ins = 5, 2, 4, 1
        for q, t, w in _pairs(600, 3):
            a = loader.ksw_global2_cigar(q, t, w, opt)
            b = (int(ans(lambda: loader.ksw_global2_cigar(q, t, w, opt, L=REF)[0])[0]), ans(lambda: loader.ksw_global2_cigar(q, t, w, opt, L=REF)[1]))
            assert a[0] == b[0] and np.array_equal(a[1], b[1]), (len(q), len(t), w)
            assert a[0] == loader.ksw_global2_score(q, t, w, opt)


def _limit_pairs():
    """(query, target, band) at the shapes tests/test_gpu_aln_limits.py drives the kernels to: queries of 511, 512 and 1 500 bases,
    gap runs of 31 to 64, bands up to 703, compensating gaps that only a wider band spans, tandem repeats with a unit missing."""
    rng = np.random.default_rng(17)
    base = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)                                # noqa: E731
    for ql in (511, 512, 1500):
        q = base(ql)
        for run in (31, 32, 33, 48, 64):
            at = int(rng.integers(40, ql - 100))
            for t in (np.concatenate([q[:at], q[at + run:]]), np.concatenate([q[:at], base(run), q[at:]])):
                for w in (run + 3, run + 40, 200):
                    yield q, t, w
                    yield t, q, w
        t = np.concatenate([q[:40], base(20), q[40:100], q[120:160], base(40), q[160:240], q[280:]])
        for w in (16, 32, 64, 703):
            yield q, t, w
    q = base(400)
    t = np.concatenate([q[:150], base(700), q[150:]])
    yield q, t, 703
    yield q[:1], t[:24], 26
    yield q[:2], t[:24], 25
    for unit in ([0], [1, 3], [2, 0, 1]):
        for k in (2, 3, 7, 20):
            for fl in (40, 250):
                a, b = base(fl), base(fl)
                q = np.concatenate([a, np.tile(unit, k), b]).astype(np.uint8)
                for t in (np.concatenate([a, np.tile(unit, k + 1), b]), np.concatenate([a, np.tile(unit, k - 1), b])):
                    for w in (4, 20):
                        yield q, t.astype(np.uint8), w
                        yield q[::-1].copy(), t[::-1].astype(np.uint8), w


def test_global_alignment_at_the_kernels_limits_equals_reference():
    """Score and CIGAR of the restated ksw_global2 against the reference's object where the device kernels are driven to their
    limits; only a digest of each answer is kept."""
    ans = Answers(REF is not None)
    alt = loader.default_sw_opt(5, 2, 3)
    alt.o_del, alt.e_del, alt.o_ins, alt.e_ins = 4, 2, 5, 1
    n = 0
    for opt in (loader.default_sw_opt(), alt):
        for q, t, w in _limit_pairs():
            sc, cig = loader.ksw_global2_cigar(q, t, w, opt)
            assert ans.same(np.concatenate([[sc], cig]), lambda: np.concatenate([[x] if np.isscalar(x) else x for x in
                                                                                 loader.ksw_global2_cigar(q, t, w, opt, L=REF)])), (len(q), len(t), w)
            assert sc == loader.ksw_global2_score(q, t, w, opt)
            n += 1
    assert n > 500


def test_reg2aln_retry_loop_against_pinned_alignment():
    """mem_reg2aln's band inference and retry loop and bwa_gen_cigar2's band, restated in tests/aln_cases.py from the reference's
    bwamem.cpp:2553-2597 and bwa.cpp:400-420 over the pinned ksw_global2: the number of tries, the last try's score and its CIGAR
    after the squeeze of an edge deletion and the clips, and the position, equal the oracle's on hand-made regions of every exit."""
    g, idx = toy()
    L, ref = len(g), idx.ref_0123
    seen = set()
    for okw in ({}, dict(w=5), dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1), dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1, w=5)):
        opt = ac.opts(**okw)[0]
        c = ac.routing_cases(g, opt).extend(ac.record_cases(g, opt)).extend(ac.traceback_cases(g, opt, "wave"))
        for kernel in ("ring", "wave", "hbm"):
            c.extend(ac.retry_cases(g, opt, kernel)).extend(ac.retry_cases_w100(g, opt, kernel))
        enc, cum, regs, off, _ = c.flat()
        tries = np.zeros((len(regs), 2), np.int32)
        aln, cig, _ = loader.reg2aln(regs, off, enc, cum, ref, L, opt=opt, tries=tries)
        m = ac.model(opt, regs, off, enc, cum, ref, L, cigar=True)
        read_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
        for k, x in enumerate(m):
            a, ar = aln[k], regs[k]
            if x["route"] == "bad":
                assert a["flag"] == 4 and a["rid"] == -1 and a["pos"] == -1 and a["n_cigar"] == 0
                continue
            assert (len(x["tries"]), x["tries"][-1][1]) == (tries[k][1], tries[k][0]), (k, x["tries"], tries[k])
            cg = [int(v) for v in x["cigar"]]
            is_rev = ar["rb"] >= L
            pos = int(2 * L - ar["re"] if is_rev else ar["rb"])
            if cg[0] & 0xf == 2:                           # bwamem.cpp:2573-2583
                pos += cg[0] >> 4
                cg = cg[1:]
            elif cg[-1] & 0xf == 2:
                cg = cg[:-1]
            lq = int(cum[read_of[k] + 1] - cum[read_of[k]])
            clip5, clip3 = (lq - ar["qe"], ar["qb"]) if is_rev else (ar["qb"], lq - ar["qe"])       # bwamem.cpp:2584-2598
            cg = ([int(clip5) << 4 | 3] if clip5 else []) + cg + ([int(clip3) << 4 | 3] if clip3 else [])
            assert cg == [int(v) for v in cig[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]] and pos == a["pos"], k
            seen.add((x["exit"], len(x["tries"]), len({s for _, s in x["tries"]})))
    # every exit: the first try, the same score twice, the cap at each try, three tries with three scores, the gap-free shortcut
    assert {("score", 1, 1), ("same", 2, 1), ("cap", 1, 1), ("cap", 2, 2), ("cap", 3, 3), ("three", 3, 3), ("same", 3, 2)} <= seen, seen


def _walk(cig, q, r):
    """(query consumed, reference consumed, mismatches + gap bases, MD) from a CIGAR without clips."""
    x = y = nm = u = 0
    md = ""
    for k, c in enumerate(cig):
        op, ln = int(c) & 0xf, int(c) >> 4
        if op == 0:
            for i in range(ln):
                if q[x + i] != r[y + i]:
                    md += str(u) + "ACGTN"[r[y + i]]; nm += 1; u = 0
                else:
                    u += 1
            x += ln; y += ln
        elif op == 2:
            if 0 < k < len(cig) - 1:
                md += str(u) + "^" + "".join("ACGTN"[b] for b in r[y:y + ln]); u = 0; nm += ln
            y += ln
        elif op == 1:
            x += ln; nm += ln
    return x, y, nm, md + str(u)


def test_reg2aln_properties_on_toy_regions():
    g, idx = toy()
    l_pac = len(g)
    ref = idx.ref_0123
    reads, _, _ = simulate.make_reads(g, 400, seed=5)
    enc, cum = simulate.flatten_reads(reads)
    o = loader.OracleFMI(idx)
    sm = o.collect_smem(enc, cum)
    coord, off = o.sa_lookup(sm)
    ch, sd, choff = loader.chain_seeds(sm, coord, off, cum, l_pac)
    regs, reg_off, _ = loader.chain2aln(ch, sd, choff, enc, cum, ref, l_pac)
    fin, fin_off = loader.regs_finish(regs, reg_off, enc, cum, ref, l_pac)
    assert len(fin) > 300
    aln, cig, md = loader.reg2aln(fin, fin_off, enc, cum, ref, l_pac)
    n_gapped = 0
    for r in range(len(fin_off) - 1):
        q = enc[cum[r]:cum[r + 1]]
        for k in range(fin_off[r], fin_off[r + 1]):
            a, ar = aln[k], fin[k]
            c = cig[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]
            m = bytes(md[a["md_off"]:a["md_off"] + a["md_len"]])
            assert m.endswith(b"\0") and a["rid"] == 0 and a["flag"] in (0, 0x100)
            is_rev = ar["rb"] >= l_pac
            assert a["is_rev"] == int(is_rev)
            core = [x for x in c if (int(x) & 0xf) != 3]
            clip5 = int(c[0]) >> 4 if (int(c[0]) & 0xf) == 3 else 0
            clip3 = int(c[-1]) >> 4 if len(c) > 1 and (int(c[-1]) & 0xf) == 3 else 0
            assert clip5 == (len(q) - ar["qe"] if is_rev else ar["qb"]) and clip3 == (ar["qb"] if is_rev else len(q) - ar["qe"])
            # the alignment in forward-strand terms: query segment (reverse-complemented on the reverse strand) vs forward text
            qs = q[ar["qb"]:ar["qe"]]
            rs = ref[ar["rb"]:ar["re"]]
            if is_rev:                                  # bwa_gen_cigar2 reverses both; the CIGAR then reads along the forward strand
                qs, rs = qs[::-1], rs[::-1]
                rs_f = np.where(rs < 4, 3 - rs, rs); qs_f = np.where(qs < 4, 3 - qs, qs)
            else:
                rs_f, qs_f = rs, qs
            # leading / trailing deletions were squeezed out of the CIGAR: put the reference bases they skip back
            lead = int(a["pos"]) - int(l_pac * 2 - 1 - (ar["re"] - 1) if is_rev else ar["rb"])
            x, y, nm, want_md = _walk(core, qs_f, rs_f[lead:])
            assert x == len(qs) and lead + y <= len(rs) and lead >= 0
            assert nm == a["NM"] or lead + y < len(rs) or lead > 0
            if lead == 0 and y == len(rs):
                assert want_md.encode() + b"\0" == m, (r, k)
            n_gapped += any((int(v) & 0xf) in (1, 2) for v in core)
            assert 0 <= a["mapq"] <= 60 and a["score"] == ar["score"]
    assert n_gapped > 10
