"""The planted chaining cases (tests/chain_cases.py) under the oracle alone: every case sits on the side of its limit that it was
built for, the settling cases are decided by the rule they are named after, and the route model's constants are the chaining sources'.
Where the reference's kbtree.h / ksort.h are built (oracle/_ref/libref_chain.so), the reads in which tree shape and sort
stability decide go through them as well."""
import bisect
import os
import re

import numpy as np
import pytest

import chain_cases as cc
from oracle import loader

REF = loader.ref_chain_lib()
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bwa-mem-scale_amd", "csrc")
CHAIN_SOURCES = ("chain_dev.h", "chain_wave.h", "chain.hip", "chain_lane.hip")


def _reads(case):
    m = cc.model(case)
    return m, dict(zip(case.notes, m["reads"]))


def _chains_of(case, r, **kw):
    ch, sd, off = case.oracle(**kw)
    return ch[off[r]:off[r + 1]], sd


def test_model_constants_are_chain_hip_s():
    texts = []
    for name in CHAIN_SOURCES:
        with open(os.path.join(CSRC, name)) as f:
            texts.append(f.read())
    assert cc.missing_constants("\n".join(texts)) == []
    for c in cc.SOURCE_CONSTANTS:                                                # a constant defined in two files would be a bug
        assert len([name for name, t in zip(CHAIN_SOURCES, texts) if re.search(c, t)]) == 1, c
    assert cc.missing_constants("constexpr int kLaneSeeds = 33;") != []
    assert [cc.cap_f("xl", cc.CLASS_XL), cc.cap_f("xl", cc.CLASS_XL2)] == [1197, 3803]
    assert all(cc.cap_f("lds", k) > k for k in cc.LDS_CLASSES)               # in the other classes the filter always fits
    assert [cc.tier_of(n) for n in (32, 33, 128, 129, 1700, 1701, 4096, 4097, 13000, 13001)] == [
        ("lane", 0), ("lds", 128), ("lds", 128), ("lds", 256), ("lds", 1700), ("xl", 4096), ("xl", 4096), ("xl", 13000), ("xl", 13000), ("hbm", 0)]


def test_class_limits_sides():
    c = cc.class_limits()
    m, rd = _reads(c)
    ns = cc.seeds_per_read(c)
    for t in cc.CLASS_ORDER:
        assert rd["seeds%d" % t][0] == t and rd["seeds%d" % (t + 1)][0] == t + 1
        assert cc.tier_of(t) != cc.tier_of(t + 1)                              # the two reads go to different launches
    assert 45000 < ns.sum() < 50000
    assert [m[k] for k in cc.COUNT_KEYS[:10]] == [int((ns > t).sum()) for t in cc.CLASS_ORDER]
    assert m["gt_XL2"] == 1 and m["gt_lane"] == 21 and m["gt_XL"] == 3
    # one chain per base position: the ladders merged as built (no read was handed to the B-tree, every chain position distinct)
    assert m["redo"] == 0 and all(r[1] == min(r[0], 499) for n, r in rd.items() if n.startswith("seeds"))
    assert rd["over_by_skipped"][:4] == (35, 30, 30, "lds") and rd["all_skipped"][:4] == (40, 0, 0, "lds") and rd["all_skipped"][5] is None
    assert rd["seeds32"][3:] == ("lane", False, "heavy") and rd["seeds13001"][3:] == ("hbm", False, "heavy")
    # both storage forms and the three orders occur
    assert {mm[3] for r in c.reads for mm in r} == {"f", "b"}
    ch, sd, off = c.oracle()
    assert off[c.read("all_skipped") + 1] == off[c.read("all_skipped")]


def test_ordered_array_sides():
    c = cc.ordered_array()
    m, rd = _reads(c)
    assert [rd[n][1] for n in ("chains64", "chains65", "chains4096", "chains4097")] == [64, 65, 4096, 4097]
    assert rd["chains4096"][3:] == ("xl", False, "heavy") and rd["chains4097"][3:] == ("xl", False, "in_wave")
    assert cc.tier_of(4096)[1] == cc.CLASS_XL and cc.tier_of(4097)[1] == cc.CLASS_XL2
    assert rd["chains64"][2] == 1 and rd["front"][1] == rd["end"][1] == 300 and rd["interleave"][1] == 328
    pos = lambda n: np.concatenate([mm[2] for mm in c.reads[c.read(n)]])        # noqa: E731
    assert np.all(np.diff(pos("front")) < 0) and np.all(np.diff(pos("end")) > 0)
    p = pos("interleave")
    assert np.all(np.diff(np.sort(p[:128])[::2]) == 16) and set(np.sort(p[:128])[::2]) == set(p[:64])      # pass two falls between pass one's
    assert m["redo"] == 0
    # default options too, and insertions AT the 64-entry chunk edges in both
    d = cc.ordered_default()
    md, rdd = _reads(d)
    assert d.opts == {} and [rdd[n][1:3] for n in d.notes] == [(64, 64), (65, 65), (300, 300), (300, 300), (328, 328), (196, 196)] and md["redo"] == 0
    for case in (c, d):
        p, held, at = np.concatenate([mm[2] for mm in case.reads[case.read("chunk_edges")]]), [], []
        for x in p.tolist():                                                    # every seed starts a chain: where its key goes
            at.append(bisect.bisect_left(held, x))
            bisect.insort(held, x)
        assert at[:192] == list(range(192)) and at[192:] == [128, 127, 64, 63]


def test_settling_rules_decide():
    c = cc.settling()
    m, rd = _reads(c)
    ch, sd, off = c.oracle(do_flt=False)
    of = lambda n: ch[off[c.read(n)]:off[c.read(n) + 1]]                        # noqa: E731
    assert rd["independent"][:2] == (300, 300)
    assert of("tandem")["n"].max() == 200 and rd["tandem"][1] == 101
    assert np.all(of("touched")["n"] == 4) and rd["touched"][1] == 20
    assert np.all(of("two_smems")["n"] == 2) and rd["two_smems"][1] == 40
    assert rd["mems64"][1] == 128 and rd["mems65"][1] == 130
    assert len(c.reads[c.read("mems64")]) == 64 and len(c.reads[c.read("mems65")]) == 65
    # equal positions: a second chain at a held position hands the read to the B-tree, a contained or merged seed does not
    assert [rd[n][4] for n in ("equal_in_pass", "equal_on_key", "equal_contained")] == [True, True, False]
    for n in ("equal_in_pass", "equal_on_key"):
        assert len(np.unique(of(n)["pos"])) == len(of(n)) - 1
    assert rd["equal_contained"][:2] == (103, 100) and of("equal_contained")["n"].sum() == 101       # two seeds contained, one merged
    assert sum(len(mm[2]) for mm in c.reads[c.read("equal_in_pass")]) <= 64                          # one pass holds the read
    # the displaced seed j (the read's last MEM): what the chain born between its looked-up chain C and itself makes of it,
    # and what C alone would have made of it (the read without seed i, its MEM before the last)
    # (across l_pac: C before it, j beyond it.  With i beyond it too, j extends i's chain where C alone leaves it on its own; with i
    # before it, j is on its own either way — test_and_merge lets no chain cross l_pac, whichever chain j is tested against)
    for note, with_i, without_i in (("displaced_new", "own", "C"), ("displaced_unsettled", "i", "C"), ("displaced_noop", "gone", "own"),
                                    ("displaced_across_lpac", "i", "own"), ("displaced_lpac_between", "own", "own")):
        r = c.read(note)
        mems = c.reads[r]
        (qi, li, pi, _), (qj, lj, pj, _) = mems[-2], mems[-1]
        P = int(mems[0][2][0])

        def fate(case):
            h, s, o = case.oracle(do_flt=False)
            for k in range(int(o[r]), int(o[r + 1])):
                ss = s[int(h[k]["seed_off"]):int(h[k]["seed_off"]) + int(h[k]["n"])]
                if ((ss["rbeg"] == int(pj[0])) & (ss["qbeg"] == qj)).any():
                    return {P: "C", int(pi[0]): "i", int(pj[0]): "own"}[int(h[k]["pos"])]
            return "gone"
        assert fate(c) == with_i, note
        assert fate(c.with_read(r, mems[:-2] + mems[-1:])) == without_i, note
        assert sum(len(mm[2]) for mm in mems[:1]) == 64                                              # C is settled a pass earlier


def test_settling_perturbations():
    """The seed (or MEM) each remaining settling read is about, moved: the oracle's chains change as the rule says."""
    c = cc.settling()

    def chains(note, mems=None):
        r = c.read(note)
        h, s, o = (c if mems is None else c.with_read(r, mems)).oracle(do_flt=False)
        return h[o[r]:o[r + 1]]
    shift = lambda m, d: (m[0], m[1], m[2] + d, m[3])                              # noqa: E731
    t = c.reads[c.read("touched")]
    assert np.all(chains("touched")["n"] == 4)
    moved = chains("touched", [t[0], shift(t[1], 200)] + t[2:])                    # the second MEM out of the band: its seeds start chains,
    assert len(moved) == 40 and sorted(set(moved["n"])) == [1, 3]                  # and the third and fourth MEMs extend those
    t = c.reads[c.read("tandem")]
    assert chains("tandem")["n"].max() == 200
    wide = chains("tandem", [(0, 20, t[0][2][0] + 105 * np.arange(200), "f"), t[1]])     # period beyond w: nothing extends anything
    assert len(wide) == 300 and wide["n"].max() == 1
    t = c.reads[c.read("two_smems")]
    assert np.all(chains("two_smems")["n"] == 2)
    assert len(chains("two_smems", [t[0], shift(t[1], 150)])) == 80                # the second span out of the band
    for note in ("equal_in_pass", "equal_on_key"):
        r = c.read(note)
        assert cc.model(c)["reads"][r][4]
        without = c.with_read(r, c.reads[r][:-1])                                   # the repeated position taken away
        assert not cc.model(without)["reads"][r][4] and len(chains(note, c.reads[r][:-1])) == len(chains(note)) - 1


def test_another_sequence_between():
    """displaced_other_seq: seed j lies inside the band of seed i's chain, born in the same pass between j and its looked-up chain
    C, but on the next sequence: a chain of its own; on one sequence it extends i's chain.  What cannot be built is a read in
    which C alone would have taken j (merged or contained) and i's sequence undoes that: a sequence is an interval of each strand
    (the sequence index is monotone in the position, checked here on the tables the cases use), so a chain between C and j on
    another sequence puts C on another sequence than j too, and across the strands test_and_merge refuses by l_pac (above).
    Random triples around the boundaries confirm it: whenever i and j lie on different sequences, j's fate is the same without i."""
    for which in ("none", "mid", "first"):
        c = cc.alt_tables(which)
        r = c.read("displaced_other_seq")
        mems = c.reads[r]
        pj, pi = int(mems[-1][2][0]), int(mems[-2][2][0])

        def fate(h, s, o):
            for k in range(int(o[r]), int(o[r + 1])):
                ss = s[int(h[k]["seed_off"]):int(h[k]["seed_off"]) + int(h[k]["n"])]
                if (ss["rbeg"] == pj).any():
                    return {pi: "i", pj: "own"}.get(int(h[k]["pos"]), "C")
            return "gone"
        assert fate(*c.oracle(do_flt=False)) == "own"
        one = cc.Case("one", c.reads, c.notes, c.opts, None, c.lens)
        assert fate(*one.oracle(do_flt=False)) == "i"
    for table in (cc.alt_tables("mid").contigs, cc.sequences(65).contigs, cc.sequences(4097).contigs):
        o = table["offset"].astype(np.int64)
        p = np.arange(0, 2 * cc.L_PAC, 7, dtype=np.int64)
        rid = np.searchsorted(o, np.where(p < cc.L_PAC, p, 2 * cc.L_PAC - 1 - p), "right") - 1
        assert np.all(np.diff(rid[p < cc.L_PAC]) >= 0) and np.all(np.diff(rid[p >= cc.L_PAC]) <= 0)
    rng = np.random.default_rng(12)
    tab = cc.alt_tables("none").contigs
    n_diff_seq = 0
    for _ in range(300):
        edge = int(rng.choice([cc.THREE[0], cc.THREE[1], 2 * cc.L_PAC - cc.THREE[0], 2 * cc.L_PAC - cc.THREE[1], cc.L_PAC]))
        pc, pi, pj = np.sort(edge + rng.integers(-120, 120, size=3))
        if pc == pi or pi == pj:
            continue
        qs = np.sort(rng.integers(0, 150, size=3))
        mems = [(int(qs[0]), 20, np.array([pc]), "f"), (int(qs[1]), 20, np.array([pi]), "f"), (int(qs[2]) + 1, 20, np.array([pj]), "f")]
        out = []
        for rd in (mems, [mems[0], mems[2]]):
            h, s, o = cc.Case("t", [rd], ["t"], contigs=tab).oracle(do_flt=False)
            hit = [int(h[k]["pos"]) for k in range(len(h)) if (s[int(h[k]["seed_off"]):int(h[k]["seed_off"]) + int(h[k]["n"])]["rbeg"] == pj).any()]
            out.append(hit[0] if hit else None)
        lay = lambda x: int(np.searchsorted(tab["offset"], x if x < cc.L_PAC else 2 * cc.L_PAC - 1 - x, "right")) * (1 if x < cc.L_PAC else -1)   # noqa: E731
        if lay(int(pi)) != lay(int(pj)) and lay(int(pi + 19)) == lay(int(pi)) and lay(int(pj + 19)) == lay(int(pj)):
            n_diff_seq += 1
            assert out[0] == out[1], (pc, pi, pj, qs)
    assert n_diff_seq > 50


def test_alt_meets_primary_both_ways():
    """(e) A heavier chain over the query span of two lighter ones, on a lane-tier read (filter_seq) and a wave-tier read
    (heavy_read).  The heavier one ALT: it shadows no primary chain, so the 19 it drops on an all-primary table is kept and
    neither is marked as overlapped by it.  The lighter ones ALT: shadowed exactly as primary chains are — by mem_chain_flt's
    rule (an overlap counts unless the selected chain is ALT and the candidate is not) these kept codes cannot differ from the
    all-primary table's, only the ALT bits do."""
    got = {}
    for which in ("none", "mid", "first"):
        c = cc.alt_tables(which)
        ch, sd, off = c.oracle()
        for note in ("alt_lane", "alt_wave"):
            r = c.read(note)
            x = ch[off[r]:off[r + 1]]
            x = x[np.isin(x["pos"], (50000, 20000, 10000))]
            got[which, note] = [(int(p), int(k >> 29) & 3, int(k >> 31)) for p, k in zip(x["pos"], x["w_kept_alt"])]
    for note in ("alt_lane", "alt_wave"):
        assert got["none", note] == [(50000, 3, 0), (20000, 1, 0)]
        assert got["mid", note] == [(50000, 3, 1), (20000, 3, 0), (10000, 1, 0)]
        assert got["first", note] == [(50000, 3, 0), (20000, 1, 1)]
    _, rd = _reads(cc.alt_tables("mid"))
    assert rd["alt_lane"][5] == "lane_seq" and rd["alt_wave"][5] == "in_wave"


def test_sequences_sides():
    for n in (1, 64, 65, 4096, 4097):
        c = cc.sequences(n)
        assert len(c.contigs) == n and int(c.contigs["len"].sum()) == cc.L_PAC
        m, rd = _reads(c)
        assert rd["wave"][0] > 64 and rd["wave"][3] == "lds" and rd["wave33"][0] == 33 and rd["lane"][3] == "lane"
        ch, sd, off = c.oracle(do_flt=False)
        in_chains = np.diff(off)
        assert all(in_chains > 0)
        # seeds across two sequences or across l_pac never reach a chain; the ones at a sequence's edges do
        sd_r = sd["rbeg"].astype(np.int64)
        fwd = np.where(sd_r < cc.L_PAC, sd_r, 2 * cc.L_PAC - (sd_r + sd["len"]))
        o = c.contigs["offset"].astype(np.int64)
        rb, re_ = np.searchsorted(o, fwd, "right") - 1, np.searchsorted(o, fwd + sd["len"] - 1, "right") - 1
        assert np.array_equal(rb, re_)
        assert (fwd == 0).any() and (fwd + sd["len"] == cc.L_PAC).any() and (sd_r >= cc.L_PAC).any()
        if n > 1:
            assert np.isin(fwd, o[1:]).any() and np.isin(fwd + sd["len"], o[1:]).any()
            assert (c.contigs["len"] == 20).any() and c.contigs["is_alt"].any()
            assert (ch["w_kept_alt"] >> 31).any()


def test_filter_sides():
    c = cc.filter_limits()
    m, rd = _reads(c)
    assert rd["lane16"][1:] == (16, 16, "lane", False, "lane_seq") and rd["lane17"][1:] == (17, 17, "lane", False, "heavy")
    assert rd["redo16"][1:] == (16, 16, "lds", True, "lane_seq") and rd["redo17"][1:] == (17, 17, "lds", True, "heavy")
    for n in (64, 65, 66, 128, 129, 256, 257, 512, 513, 960, 961):
        assert rd["redo%d" % n] == (n, n, n, "lds", True, "heavy")
    assert rd["xl1197"][1:] == (1197, 1197, "xl", False, "in_wave") and rd["xl1198"][1:] == (1198, 1198, "xl", False, "heavy")
    assert rd["depth_limit"][1:] == (200, 200, "lds", False, "in_wave")
    ch, sd, off = c.oracle()
    kept = (ch["w_kept_alt"] >> 29) & 3
    r = c.read("tie_blocks")
    k_tb, n_pre = kept[off[r]:off[r + 1]], rd["tie_blocks"][2]
    assert set(k_tb) == {1, 2, 3} and len(k_tb) < n_pre                         # dropped, first-shadowed, overlapping and free chains
    w = cc.chain_weights(*_chains_of(c, r, do_flt=False))
    runs = np.diff(np.flatnonzero(np.concatenate([[1], np.diff(np.sort(w)) != 0, [1]])))
    assert {16, 17}.issubset(set(runs)) and runs.max() >= 40
    r = c.read("depth_limit")
    w = cc.chain_weights(*_chains_of(c, r, do_flt=False))
    order = []
    assert cc.ks_introsort_trace(len(w), lambda i, j: (order.append(0), w[i] > w[j])[1])             # this very input reaches the depth limit
    b = cc.filter_big()
    mb, rb = _reads(b)
    assert rb["redo3840"][2:] == (3840, "xl", True, "heavy") and rb["redo3841"][2:] == (3841, "xl", True, "seq")
    assert rb["xl2_3803"][2:] == (3803, "xl", False, "in_wave") and rb["xl2_3804"][2:] == (3804, "xl", False, "heavy")
    assert all(cc.tier_of(x[0])[1] == cc.CLASS_XL2 for n, x in rb.items() if n.startswith("xl2"))
    assert mb["flt_more"] == 3 and mb["flt_seq"] == 1 and mb["n_heavy"] == 3 and cc.model(cc.filter_limits())["flt_seq"] == 0


def test_filter_options_bite():
    base = cc.filter_limits()
    ext, none = cc.filter_options("extend"), cc.filter_options("floor_all")
    ch, sd, off = ext.oracle()
    ch0, sd0, off0 = ext.oracle(max_chain_extend=1 << 30)
    assert np.diff(off).sum() < np.diff(off0).sum() and (np.diff(off) > 5).any()               # truncated, and fewer than the chains
    ch, sd, off = none.oracle()
    assert np.all(np.diff(off) == 1)                                                           # a_[0] alone
    _, rd = _reads(none)
    assert rd["lane16"][5] == "lane_seq" and rd["xl1197"][5] == "in_wave" and all(x[2] == 1 for x in rd.values())
    _, rs = _reads(cc.filter_options("floor_some"))
    assert all(1 < x[2] < x[1] for n, x in rs.items() if n != "xl1197")
    assert base.read("lane16") == 0


def test_stride_pick_and_coordinates_sides():
    c = cc.stride_pick()
    m, rd = _reads(c)
    assert [rd["hits%d" % h][0] for h in (50, 51, 99, 100, 151)] == [50] * 5                   # max_occ = 50 seeds whatever the hit count
    ch, sd, off = c.oracle(do_flt=False)
    for h, step in ((50, 1), (51, 1), (99, 1), (100, 2), (151, 3)):
        r = c.read("hits%d" % h)
        want = np.sort(c.reads[r][0][2][::step][:50])
        assert np.array_equal(np.sort(ch["pos"][off[r]:off[r + 1]]), want), h
    assert rd["empty_mems"][0] == 40 and rd["only_empty"][:2] == (0, 0) and rd["duplicates"][:2] == (100, 70)
    g = cc.coordinates()
    ch, sd, off = g.oracle()
    assert g.lens == [32767] and (sd["qbeg"] + sd["len"]).max() == 32767 and len(ch) >= 3


def test_tree_shape_and_sort_stability_against_the_reference():
    if REF is None:
        pytest.skip("oracle/_ref/libref_chain.so is not built here")
    c = cc.settling()
    ch, sd, off = c.oracle(do_flt=False)
    for note in ("equal_in_pass", "equal_on_key"):                  # every seed starts a chain: the script is the seeds in MEM order
        r = c.read(note)
        pos = np.concatenate([mm[2] for mm in sorted(c.reads[r], key=lambda mm: (mm[0], mm[0] + mm[1]))]).astype(np.int64)
        put = np.ones(len(pos), np.uint8)
        lo, order = loader.kbt_script(pos, put)
        lo_r, order_r = loader.kbt_script(pos, put, REF)
        assert np.array_equal(lo, lo_r) and np.array_equal(order, order_r)
        assert np.array_equal(pos[order_r], ch["pos"][off[r]:off[r + 1]])                      # the oracle's chains come in the reference tree's order
    f = cc.filter_limits()
    for note in ("tie_blocks", "depth_limit", "redo513"):
        w = cc.chain_weights(*_chains_of(f, f.read(note), do_flt=False)).astype(np.uint32)
        assert np.array_equal(loader.flt_sort(w), loader.flt_sort(w, REF)), note
