"""The generators of tests/pair_cases.py keep their promises, under the oracle alone (no GPU): every read sits on the intended
side of every limit (the pool capacity from the inputs, the final region count from loader.pair_pe / loader.mark_primary_se),
every route gets its eight reads, the events a case aims at happen (windows aligned, regions added, regions dropped, equal ends
in a read that consumes an alignment), the pairs of tied fillers decide the result by their order, and no candidate of mem_pair
has an insert-size score within 1e-6 of the integer step it is truncated at.  These are conditions on the inputs, not
measurements of the library: tests/test_gpu_pair_limits.py compares the device's counts with the numbers checked here."""
import collections

import numpy as np
import pytest

import aln_cases as ac
import pair_cases as pc
from oracle import loader


@pytest.fixture(scope="module")
def env():
    g, idx = pc.setting()
    return g, idx.ref_0123, ac.opts()[0]


def _run(env, c, pes, **kw):
    g, ref, opt = env
    assert c.acceptable()
    enc, cum, regs, off = c.flat()
    want, woff, pairs = loader.pair_pe(regs, off, enc, cum, ref, pc.L_PAC, pes, contigs=c.contigs, opt=opt, **kw)
    return (enc, cum, regs, off), (want, woff, pairs)


def _q_margin(pes, want, woff, pairs, opt):
    q = pc.insert_q(pes, want, woff, pairs, opt)
    frac = q - np.floor(q)
    assert q.size == 0 or min(frac.min(), (1 - frac).min()) >= 1e-6, "an insert-size score within 1e-6 of its integer step"
    return q.size


def _by_tag(c, *cols):
    by = collections.defaultdict(list)
    for p, t in enumerate(c.tags):
        by[t].append(tuple(col[p] for col in cols))
    return by


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
@pytest.mark.parametrize("name", sorted(pc.RESCUE_FILES))
def test_rescue_file(env, name, alt):
    opt = env[2]
    c = pc.RESCUE_FILES[name](alt)
    pes = pc.RESCUE_PES.get(name, pc.PES_FR)
    (enc, cum, regs, off), (want, woff, pairs) = _run(env, c, pes)
    cap, added = pc.caps(opt, regs, off), np.diff(woff) - np.diff(off)
    plan = pc.planned(opt, c.contigs, pes, regs, off, cum)
    n_in = np.diff(off)
    P = range(len(c.tags))
    by = _by_tag(c, [cap[2 * p + 1] for p in P], [int(added[2 * p + 1]) for p in P], [int(pairs["n_matesw"][p]) for p in P],
                 [len(plan[2 * p]) for p in P], [len(plan[2 * p + 1]) for p in P], [int(n_in[2 * p + 1]) for p in P], list(P))
    route = pc.routes(opt, regs, off, woff)
    assert all(len(v) >= 8 for t, v in by.items() if not t.startswith(("clip", "edge")))
    _q_margin(pes, want, woff, pairs, opt)
    if name == "capacity":
        for k in (4, 5, 16, 17, 1024, 1025):
            assert all(x[0] == k and x[1] == 1 and x[2] >= 1 for x in by["cap%d" % k]), k
        assert route["post_lane"] >= 24 and route["post_wave"] >= 16 and route["post_one_lane"] == 8
        assert all(x[0] == 230 and x[1] >= 3 for x in by["anchors50"])                      # several of the fifty succeed
        assert all(len(pc.anchors_of(opt, regs, off, 2 * x[6])) == 50 for x in by["anchors50"])
        for t, k in (("idle_lane", 12), ("idle_wave", 38)):                                 # both planned, the second no longer wanted
            assert all(x[0] == k and x[1] == 1 and x[4] == 2 and x[2] == x[3] + 1 for x in by[t]), t
    elif name == "sort":
        for t, v in by.items():
            k = int(t[4:])
            na = 2 if k < 1000 else 1
            assert all(x[5] + 1 == k and x[0] == k - 1 + 4 * na <= pc.POST_LDS and x[1] == na for x in v), t
        assert {int(t[4:]) for t in by} >= {pc.RANK_MAX, pc.RANK_MAX + 1, 127, 128, 129, 512, 513, 1020}
    elif name == "insertion":
        for t, v in by.items():
            for x in v:
                p = x[6]
                fl, out = regs[off[2 * p + 1]:off[2 * p + 2]], want[woff[2 * p + 1]:woff[2 * p + 2]]
                new = [a for a in out if a["re"] - a["rb"] > 100]
                assert x[1] == 1 and len(new) == 1
                at = int((fl["score"] >= new[0]["score"]).sum())
                n = len(fl)
                assert at == (0 if t.startswith("at0") else n if t.startswith("atn") else 8 if t == "eq" else 64 if t == "eq_wave" else int(t[2:])), (t, at)
                if t.startswith("eq"):
                    assert (fl["score"] == new[0]["score"]).sum() == 3
                if t.startswith("at0"):
                    assert (n - at) % 64 == 0
    elif name == "tie":
        (_, _, regs2, off2), (want2, woff2, _) = _run(env, pc.tie_cases(alt, swap=True), pes)
        assert np.array_equal(np.sort(regs2, order=["rb", "re", "w"]), np.sort(regs, order=["rb", "re", "w"]))      # the same regions, tied pairs in the other order
        for t, v in by.items():
            for x in v:
                r = 2 * x[6] + 1
                fl = regs[off[r]:off[r + 1]]
                assert len(fl) - len(np.unique(fl["re"])) == 3 and x[1] == -2 and x[2] >= 1   # equal ends, an alignment consumed, one of each pair dropped
                a, b = want[woff[r]:woff[r + 1]], want2[woff2[r]:woff2[r + 1]]
                assert len(a) == len(b) and sorted(a["rb"].tolist()) != sorted(b["rb"].tolist())     # the introsort's order decided the survivors
        assert all(x[5] + 1 <= pc.RANK_MAX for x in by["tie_rank"]) and all(x[5] + 1 > pc.RANK_MAX for x in by["tie_net"])
    elif name == "dedup":
        for t, v in by.items():
            for x in v:
                r = 2 * x[6] + 1
                out = want[woff[r]:woff[r + 1]]
                long_ = [int(a["re"] - a["rb"]) for a in out if a["re"] - a["rb"] > 100]
                assert x[1] == 0
                if t == "consistent":
                    assert x[4] == 0 and long_ == [pc.SEG]                                   # no window: the filler stays alone
                else:
                    assert x[4] == 1 and long_ == [{"filler_wins": pc.SEG + 60}.get(t, pc.SEG)], (t, long_)
    elif name == "window":
        assert all(x[2] == x[3] + x[4] for v in by.values() for x in v)                     # empty mate lists: every planned window is aligned
        w = lambda t, k: [pc.window(opt, c.contigs, pes, int(regs["rb"][off[2 * x[6]]]), int(regs["rid"][off[2 * x[6]]]), k, pc.SEG) for x in by[t]]  # noqa: E731
        assert w("clip19_lo", 3) == [(0, 19)] and w("clip18_lo", 3) == [None]
        assert w("clip19_hi", 0) == [(2 * pc.L_PAC - 19, 2 * pc.L_PAC)] and w("clip18_hi", 0) == [None]
        ws = [pc.window(opt, c.contigs, pes, int(regs["rb"][off[2 * x[6]]]), int(regs["rid"][off[2 * x[6]]]), k, pc.SEG) for x in by["edge"] for k in range(4)]
        full = pes["high"][0] - pes["low"][0] + pc.SEG
        assert sum(x is None for x in ws) >= 8 and sum(x is not None and x[1] - x[0] == full for x in ws) >= 8
        assert sum(x is not None and x[1] - x[0] < full for x in ws) >= (16 if alt else 8)  # clipped at a sequence's end
    elif name == "matelen":
        for L in (249, 250, 512):
            for x in by["len%d" % L]:
                r = 2 * x[6] + 1
                out = want[woff[r]:woff[r + 1]]
                assert x[1] == 1 and x[0] == 24 and cum[r + 1] - cum[r] == L and max(out["qe"] - out["qb"]) >= L - 30


@pytest.mark.parametrize("alt", (False, True), ids=("one_seq", "alt"))
def test_ert_variant_events(env, alt):
    """Under useErt: a filler that shares the rescued region's end in a read that consumes an alignment (the resort by score),
    reads whose last anchor consumes an alignment and reads whose last anchor does not."""
    opt = env[2]
    c = pc.dedup_cases(alt)
    (enc, cum, regs, off), (want, woff, pairs) = _run(env, c, pc.PES_NARROW, use_ert=True)
    n = 0
    for p, t in enumerate(c.tags):
        if t == "same_re":
            r = 2 * p + 1
            ends = regs["re"][off[r]:off[r + 1]]
            b_re = {0: 2 * pc.L_PAC - pc.COPIES[(n // 2) % 4][0], 1: pc.COPIES[(n // 2) % 4][0] + pc.SEG}[n % 2]
            assert b_re in ends.tolist() and pairs["n_matesw"][p] >= 2
            n += 1
    assert n == 8
    c = pc.capacity_cases(alt)
    (enc, cum, regs, off), (want, woff, pairs) = _run(env, c, pc.PES_FR, use_ert=True)
    plan = pc.planned(opt, c.contigs, pc.PES_FR, regs, off, cum)
    idle = [pairs["n_matesw"][p] == len(plan[2 * p]) + 1 and len(plan[2 * p + 1]) == 2 for p, t in enumerate(c.tags) if t.startswith("idle")]
    busy = [pairs["n_matesw"][p] == len(plan[2 * p]) + 1 and len(plan[2 * p + 1]) == 1 for p, t in enumerate(c.tags) if t == "cap1025"]
    assert len(idle) == 16 and all(idle) and len(busy) == 8 and all(busy)
    cap = pc.caps(opt, regs, off)
    assert sum(x <= 16 for x in cap) >= 8 and sum(100 <= x <= 1024 for x in cap) >= 8 and sum(x > 1024 for x in cap) >= 8


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_reaches_every_route(env, seed):
    opt = env[2]
    c = pc.fuzz_cases(bool(seed & 1), seed)
    (enc, cum, regs, off), (want, woff, pairs) = _run(env, c, pc.PES_ALL)
    route = pc.routes(opt, regs, off, woff)
    assert all(route[k] >= 8 for k in ("post_lane", "post_wave", "post_one_lane", "mark_lane", "mark_wave256", "mark_wave2048")), route
    assert (np.diff(woff) > np.diff(off)).sum() >= 60 and (np.diff(woff) < np.diff(off)).sum() >= 4
    _q_margin(pc.PES_ALL, want, woff, pairs, opt)


def test_second_pass_reads(env):
    """Under BWAMS_PAIR_DROP_PLAN the second pass visits every read for which the first one would have planned a window: at
    least eight on every route."""
    opt = env[2]
    for f in (pc.capacity_cases, pc.sort_cases):
        c = f(True)
        enc, cum, regs, off = c.flat()
        plan = pc.planned(opt, c.contigs, pc.PES_FR, regs, off, cum)
        cap = pc.caps(opt, regs, off)
        redo = collections.Counter(pc.post_route(cap[r], False) for r in range(len(cap)) if plan[r])
        assert all(redo[k] >= 8 for k in (("post_lane", "post_wave", "post_one_lane") if f is pc.capacity_cases else ("post_wave",))), redo


def test_mark_cases(env):
    opt = env[2]
    c = pc.mark_cases()
    enc, cum, regs, off = c.flat()
    assert (len(cum) - 1) % 2 == 1 and c.acceptable() and pc.mark_cases(True).acceptable()
    id_base = 1001
    n_z, routes, moved = [], collections.Counter(), 0
    seen = dict(sub=0, sub_n=0, alt_sc=0, sec_differs=0, equal_runs=0)
    for r in range(len(cum) - 1):
        a = regs[off[r]:off[r + 1]]
        out, n_pri = loader.mark_primary_se(a, id_base + r, opt)
        n, form = len(a), pc.MARK_FORMS[r % 4] if r < 52 else "pri" if r < 54 else "mixed"
        assert n == (pc.MARK_SIZES[r // 4] if r < 52 else 2049 if r < 54 else 300)
        assert n_pri == {"pri": n, "alt": 0, "one_pri": min(n, 1)}.get(form, n_pri) and (form != "mixed" or n < 3 or 0 < n_pri < n)
        routes[pc.mark_route(n)] += 1
        routes["rank" if pc.MARK_LIGHT < n <= pc.RANK_MAX else "net" if pc.RANK_MAX < n <= pc.MARK_LDS else "-"] += 1
        if n:
            n_z.append(int((out["secondary"] < 0).sum()))
            seen["sub"] += int((out["sub"] > 0).sum()); seen["sub_n"] += int((out["sub_n"] > 0).sum()); seen["alt_sc"] += int((out["alt_sc"] > 0).sum())
            seen["sec_differs"] += int((out["secondary"] != out["secondary_all"]).sum())
            seen["equal_runs"] += int(((np.diff(a["score"]) == 0) & (np.diff(a["n_comp_is_alt"]) == 0)).sum())
        if n > pc.MARK_SMALL:
            out5, _ = loader.mark_primary_se(a, id_base + r, opt, primary5_T=30)
            moved += int(out5["rb"][0] != out["rb"][0])
    assert all(routes[k] >= 8 for k in ("mark_lane", "mark_wave256", "mark_wave2048", "mark_one_lane", "rank", "net")), routes
    assert min(n_z) == 1 and max(n_z) >= 24 and all(v >= 100 for v in seen.values()), (min(n_z), max(n_z), seen)
    assert moved >= 4                                          # long lists whose leftmost primary is not region 0


@pytest.mark.parametrize("pes", (pc.PES_ALL, pc.PES_RF_FAILED), ids=("all", "rf_failed"))
def test_mark_cases_as_pairs(env, pes):
    """The marking reads as ends of pairs (no rescue): mem_pair over up to 2600 primaries per end."""
    opt = env[2]
    c = pc.mark_cases()
    c.reads, c.regs, c.tags = c.reads[:54], c.regs[:54], c.tags[:27]
    (enc, cum, regs, off), (want, woff, pairs) = _run(env, c, pes, no_rescue=True, id_base=77)
    assert np.array_equal(woff, off)
    assert (pairs["n_pri"].min(axis=1) >= 2049).sum() >= 1 and (pairs["n_pri"].min(axis=1) == 0).sum() >= 8
    assert ((pairs["n_pri"].min(axis=1) == 0) <= (pairs["score"] == 0)).all() and (pairs["score"] > 0).sum() >= 8
    assert (pairs["n_sub"] > 0).sum() >= 4 and (pairs["sub"] > 0).sum() >= 8
    assert _q_margin(pes, want, woff, pairs, opt) >= 1000
