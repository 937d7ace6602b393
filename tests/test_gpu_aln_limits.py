"""bwams_reg2aln_run on hand-made regions (bwams_debug_regs_upload), at the limits of each of its kernels: the gap-free shortcut,
the lane-per-region DP on the 32-column ring, the wave-per-region DP, the lane-per-region DP with its row in global memory, the
retry loop of mem_reg2aln around them and the requeue from the ring to the wave kernel.  Every record field, every CIGAR word
and every MD byte equal the oracle's on the same regions (integers and bytes: no tolerance), and the lengths of the device's
four region lists (bwams_debug_aln_lists) equal what tests/aln_cases.py computes from aln_plan_kernel's rule.  A test that aims
at a route asserts that the device's own list holds at least 8 regions of it.

The tie rules of the direction byte are tested by test_direction_ties on regions found for the purpose (aln_cases.TIE_TABLE); the
cases of the other tests hang on the M | E and H | F rules by the hundred but hardly ever on the two "gap extended | opened" ones.

Not reachable, even with the hook: a single gap run of more than 12 bases in the ring kernel (the band is at least
|lr - lq| + 3, and the ring holds bands up to 15), and the limit of 2^20 reference bases on its own (the toy text has 40 000
positions, so such a region also ends beyond the text)."""
import collections

import numpy as np
import pytest

import aln_cases as ac
from bwams import capi
from oracle import loader
from test_gpu_aln import FIELDS, _check
from util import toy

pytestmark = pytest.mark.gpu

ALT = dict(a=2, b=3, o_del=4, e_del=2, o_ins=5, e_ins=1)
KERNELS = ("ring", "wave", "hbm")


@pytest.fixture(scope="module")
def dev():
    g, idx = toy()
    ix = capi.Index.from_host(idx, 0)
    yield g, idx, ix
    ix.close()


def _upload(b, flat):
    enc, cum, regs, off, _ = flat
    b.seed_upload(enc if len(enc) else np.zeros(1, np.uint8), cum)
    b.debug_regs_upload(regs, off)


def _run(dev, c, okw, order=None, batch=None, contigs=None, ix=None, ties=False):
    """Upload the reads and regions of c, run reg2aln(opt, 0), compare with the oracle and with the model's list counts.
    Returns (model per region, tag per region, device list counts, device result)."""
    g, idx, ix0 = dev
    oopt, gopt = ac.opts(**okw)
    flat = c.flat(order)
    enc, cum, regs, off, tags = flat
    b = batch or capi.Batch(ix or ix0, max(len(cum) - 1, 1), max(int(cum[-1]), 1))
    _upload(b, flat)
    got = b.reg2aln(gopt, 0)
    cnt = b.debug_aln_lists()
    if batch is None:
        b.close()
    m = ac.model(oopt, regs, off, enc, cum, idx.ref_0123, len(g), ties=ties)
    print("regions", len(regs), "device lists", cnt.tolist(), "model", ac.counts(m).tolist(),
          "finished by", dict(collections.Counter(ac.kernel_of(x) for x in m)))
    _check(got, loader.reg2aln(regs, off, enc, cum, idx.ref_0123, len(g), contigs=contigs, opt=oopt))
    assert np.array_equal(cnt, ac.counts(m)), (cnt, ac.counts(m))
    return m, tags, cnt, got


def _tagged(m, tags, tag, n=8):
    xs = [x for x, t in zip(m, tags) if t == tag]
    assert len(xs) >= n, (tag, len(xs))
    return xs


def _bands(x):
    return [w for w, _ in x["tries"]]


def _n_scores(x):
    return len({s for _, s in x["tries"]})


def test_routing_edges(dev):
    """First-try band 15 | 16 (ring | wave launch 1) and 63 | 64 (wave launch 1 | 2), 511 | 512 query bases under a DP band
    (wave | row in global memory), a score deficit one below and at 2 (o + e - a) with equal lengths (shortcut | DP)."""
    for okw in ({}, ALT):
        m, tags, cnt, _ = _run(dev, ac.routing_cases(dev[0], ac.opts(**okw)[0]), okw)
        want = {"band15": ("ring", 15), "band16": ("wave1", 16), "band63": ("wave1", 63), "band64": ("wave2", 64)}
        for tag, (route, w) in want.items():
            assert all(x["route"] == route and _bands(x) == [w] for x in _tagged(m, tags, tag)), tag
        assert all(x["lq"] == 511 and ac.kernel_of(x) == "wave" for x in _tagged(m, tags, "lq511"))
        assert all(x["lq"] == 512 and ac.kernel_of(x) == "hbm" for x in _tagged(m, tags, "lq512"))
        assert all(x["route"] == "simple" for x in _tagged(m, tags, "deficit-edge"))
        assert all(x["route"] == "ring" for x in _tagged(m, tags, "deficit=edge"))
        assert cnt[0] >= 16 and cnt[1] >= 32 and cnt[2] >= 8 and cnt[3] >= 8


@pytest.mark.parametrize("kernel", KERNELS)
def test_retry_loop(dev, kernel):
    """Every exit of mem_reg2aln's loop in the kernel that finishes the region: the first try, the score of the try before,
    w2 = 4 opt.w, three tries; scores that rise from try to try (so that the CIGAR must be the last band's); the requeue."""
    g = dev[0]
    m, tags, cnt, _ = _run(dev, ac.retry_cases_w100(g, ac.opts()[0], kernel), {})
    assert all(ac.kernel_of(x) == kernel for x, t in zip(m, tags) if t != "requeue")
    if kernel == "ring":                                       # bands 10, 20, 35: the second try outgrows the ring and spans the gaps
        assert all(x["requeue"] and _bands(x) == [10, 20, 35] and _n_scores(x) == 2 for x in _tagged(m, tags, "requeue"))
        assert cnt[2] >= 8
    assert all(len(x["tries"]) == 1 and x["exit"] == "score" for x in _tagged(m, tags, "first"))
    assert all(len(x["tries"]) == 2 and x["exit"] == "same" for x in _tagged(m, tags, "same"))
    assert all(x["exit"] == "three" and _n_scores(x) == 3 and len(set(_bands(x))) == 3 for x in _tagged(m, tags, "three"))
    assert cnt[{"ring": 0, "wave": 1, "hbm": 3}[kernel]] >= 24

    m, tags, cnt, _ = _run(dev, ac.retry_cases(g, ac.opts(w=5)[0], kernel), dict(w=5))
    assert all(x["exit"] == "cap" and len(x["tries"]) == 1 and ac.kernel_of(x) == kernel for x in _tagged(m, tags, "cap@1"))
    # bands 5, 10, 20 from the ring's list: the third try outgrows the ring, and only it spans the two gaps of 12
    rq = [x for x in _tagged(m, tags, "requeue@3") if x["requeue"]]
    assert len(rq) >= 8 and all(_bands(x) == [5, 10, 20] and x["exit"] == "cap" and _n_scores(x) >= 2 for x in rq)
    assert all(ac.kernel_of(x) == ("wave" if kernel == "ring" else kernel) for x in rq)
    if kernel == "ring":
        # 16 such regions: in two of them the band of 10 already finds what the band of 5 found, and the loop ends there
        rq += [x for x in _tagged(m, tags, "requeue@2") if x["requeue"]]
        assert len(rq) >= 16 and cnt[0] >= 24 and cnt[2] >= 16     # launch 2 holds nothing but requeued regions
    else:
        assert all(x["exit"] == "cap" and _bands(x) == [20] for x in _tagged(m, tags, "cap@1 gaps"))
        assert cnt[1] >= 16 and cnt[2] >= 8 and (kernel == "wave" or cnt[3] >= 24)
    assert cnt[2] == len(rq)


def test_wave_kernel_geometry(dev):
    """Band columns 63, 65, 127, 129 and 401 (chunks of 64 columns with carries), queries of 1, 2, 63, 64, 65 and 511 bases,
    targets of 1 024 (staged in LDS) and 1 025 (read from global memory) bases on both strands, a band of 703."""
    m, tags, cnt, _ = _run(dev, ac.geometry_cases(dev[0], ac.opts()[0]), {})
    assert all(ac.kernel_of(x) == "wave" for x in m)
    for cols in (63, 65, 127, 129, 401):
        assert all(2 * _bands(x)[0] + 1 == cols for x in _tagged(m, tags, f"cols{cols}")), cols
    for lq in (1, 2, 63, 64, 65, 511):
        assert all(x["lq"] == lq for x in _tagged(m, tags, f"lq{lq}")), lq
    for lr in (1024, 1025, 1100):
        assert all(x["lr"] == lr and x["lq"] <= 511 for x in _tagged(m, tags, f"lr{lr}")), lr
    assert all(_bands(x) == [703] for x in _tagged(m, tags, "lr1100"))
    # row i holds columns [max(i - w, 0), min(i + w + 1, qlen)): regions with rows of the full 2 w + 1 columns between the two
    # clipped ends, regions whose rows past w are clipped by the query's end only, regions with no row past w at all
    w = np.array([_bands(x)[0] for x in m]); lq = np.array([x["lq"] for x in m]); lr = np.array([x["lr"] for x in m])
    assert ((lr > w + 1) & (lq > 2 * w + 2)).sum() >= 8 and ((lr > w + 1) & (lq <= 2 * w + 1)).sum() >= 8
    assert (lr <= w + 1).sum() >= 8
    assert cnt[1] >= 8 and cnt[2] >= 8 and cnt[3] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_traceback(dev, kernel):
    """Gap runs of 31, 32, 33 and 64 (ring: up to 12), gaps a sweep of distances before the cell the walk starts from (the
    edges of the wave kernel's 32 x 32 window), alignments that begin or end with a gap, tandem repeats with one unit missing
    or added, where only the precedence of the direction bits places the gap."""
    c = ac.traceback_cases(dev[0], ac.opts()[0], kernel)
    m, tags, cnt, got = _run(dev, c, {})
    assert all(ac.kernel_of(x) == kernel for x in m)
    for ln in ((1, 5, 11, 12) if kernel == "ring" else (31, 32, 33, 64)):
        for op in "DI":
            _tagged(m, tags, f"{op}{ln}")
    for tag in ("Dwin", "Iwin", "Dwin2", "D first", "D last", "I first", "I last"):
        _tagged(m, tags, tag)
    for period in (1, 2, 3):
        _tagged(m, tags, f"tandem{period}D"); _tagged(m, tags, f"tandem{period}I")
    # alignments that begin with a deletion: the squeeze shifts the position off the region's first base
    regs, aln, L = c.flat()[2], got[0], len(dev[0])
    start = np.where(regs["rb"] < L, regs["rb"], 2 * L - regs["re"])
    edge = np.array([t in ("D first", "D last") for t in tags])
    assert (aln["pos"][edge] != start[edge]).sum() >= 8
    assert cnt[{"ring": 0, "wave": 1, "hbm": 3}[kernel]] >= 100


@pytest.mark.parametrize("kernel", KERNELS)
def test_direction_ties(dev, kernel):
    """The four comparisons behind a direction byte (M against E, H against F, a gap extended against opened, for deletions and
    for insertions): regions whose CIGAR changes when the oracle turns one of them on a tie, at least 8 per comparison and
    kernel, so that a kernel with a wrong tie rule cannot equal the oracle.  Then, under opt.w = 5, the cases whose band the cap
    of 4 opt.w holds below their gaps: the alignment runs along the band's edge, where the extension ties are frequent."""
    g = dev[0]
    m, _, cnt, _ = _run(dev, ac.tie_cases(g, ac.opts()[0], kernel), {}, ties=True)
    assert all(ac.kernel_of(x) == kernel for x in m)
    for bit, name in ac.TIES.items():
        assert sum(bit in x["ties"] for x in m) >= 8, name
    assert cnt[{"ring": 0, "wave": 1, "hbm": 3}[kernel]] >= 16
    o5 = ac.opts(w=5)[0]
    c = ac.retry_cases_w100(g, o5, kernel)
    if kernel == "wave":
        c.extend(ac.geometry_cases(g, o5))
    m, _, _, _ = _run(dev, c, dict(w=5), ties=True)
    if kernel != "ring":                                       # the ring's bands stay below the cap of 20
        for bit in (4, 8):
            assert sum(bit in x["ties"] and ac.kernel_of(x) == kernel for x in m) >= 2, ac.TIES[bit]


def test_strands_records_contigs(dev):
    """Clips on either end and both, on both strands; 0x100; the ALT bit; Ns; regions next to every boundary of a three-contig
    table; the regions the plan rule rejects become the unmapped record and leave their neighbours right."""
    g, idx, _ = dev
    c = ac.record_cases(g, ac.opts()[0])
    m, tags, cnt, got = _run(dev, c, {})
    aln = got[0]
    bad = np.array([x["route"] == "bad" for x in m])
    assert bad.sum() >= 16
    assert np.all(aln["rid"][bad] == -1) and np.all(aln["pos"][bad] == -1) and np.all(aln["flag"][bad] == 4)
    assert np.all(aln["n_cigar"][bad] == 0) and np.all(aln["md_len"][bad] == 0)
    assert np.all(aln["rid"][~bad] == 0) and np.all(aln["n_cigar"][~bad] > 0)
    sec = c.flat()[2]["secondary"] >= 0
    assert sec.sum() >= 16
    assert np.all(aln["flag"][sec] == 0x100) and np.all(aln["flag"][~sec & ~bad] == 0)
    alt = (c.flat()[2]["n_comp_is_alt"] >> 30 & 1) == 1
    assert alt.sum() >= 16 and np.all(aln["is_alt"][alt & ~bad] == 1) and not aln["is_alt"][~alt].any()
    assert 0.3 < aln["is_rev"][~bad].mean() < 0.7
    assert cnt[0] >= 8
    simple = np.array([x["route"] == "simple" for x in m])      # the gap-free twins: clipped, secondary, ALT, at the contigs' ends
    assert simple.sum() >= 40 and all(t.startswith("gap-free") for t, s_ in zip(tags, simple) if s_)
    assert (aln["n_cigar"][simple] > 1).sum() >= 24 and (aln["flag"][simple] == 0x100).sum() >= 8 and aln["is_alt"][simple].sum() >= 8
    assert np.all(aln["NM"][simple] >= 2) and 0.3 < aln["is_rev"][simple].mean() < 0.7

    contigs = np.zeros(3, capi.CONTIG_DTYPE)
    contigs["offset"], contigs["len"], contigs["is_alt"] = [0, 9000, 15000], [9000, 6000, len(g) - 15000], [0, 1, 0]
    ix = capi.Index.from_host(idx, 0)
    ix.set_contigs(contigs)
    _, tags, _, got = _run(dev, c, {}, contigs=contigs, ix=ix)
    ix.close()
    rid = got[0]["rid"]
    for tag in ("contig start", "contig start D", "contig end", "gap-free contig start", "gap-free contig end"):
        assert {0, 1, 2} <= set(rid[[t == tag for t in tags]].tolist()), tag


def test_other_scoring_and_band_option(dev):
    """a, b = 2, 3 with o_del, e_del, o_ins, e_ins = 4, 2, 5, 1 (with a = 2 and e = 1 or 2 every quotient of bwa_gen_cigar2's
    max_gap is an integer, where the truncation after '+ 1.' must not lose one), under opt.w = 100 and 5."""
    g = dev[0]
    o100, o5 = ac.opts(**ALT)[0], ac.opts(w=5, **ALT)[0]
    c = ac.geometry_cases(g, o100)
    for kernel in KERNELS:
        c.extend(ac.retry_cases_w100(g, o100, kernel)).extend(ac.traceback_cases(g, o100, kernel))
    m, _, cnt, _ = _run(dev, c, ALT)
    by = collections.Counter(ac.kernel_of(x) for x in m)
    assert min(by[k] for k in KERNELS) >= 100 and cnt.min() >= 8
    assert sum(x["exit"] == "three" and _n_scores(x) == 3 for x in m) >= 24
    c = ac.Cases(g)
    for kernel in KERNELS:
        c.extend(ac.retry_cases(g, o5, kernel))
    m, _, cnt, _ = _run(dev, c, dict(w=5, **ALT))
    assert sum(x["requeue"] for x in m) >= 8 and cnt.min() >= 8


def _everything(g):
    o = ac.opts()[0]
    c = ac.routing_cases(g, o).extend(ac.geometry_cases(g, o)).extend(ac.record_cases(g, o))
    for kernel in KERNELS:
        c.extend(ac.retry_cases_w100(g, o, kernel)).extend(ac.traceback_cases(g, o, kernel)).extend(ac.tie_cases(g, o, kernel))
    for n in (0, 1, 30, 150, 700):
        for _ in range(8):
            c.bare(n)
    return c


def _per_region(c, order, got):
    aln, cig, md = got
    out = {}
    for k, key in enumerate(c.ids(order)):
        a = aln[k]
        out[key] = (tuple(int(a[f]) for f in FIELDS if f not in ("cigar_off", "md_off")),
                    cig[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]].tobytes(), md[a["md_off"]:a["md_off"] + a["md_len"]].tobytes())
    return out


def test_all_regions_shuffled_and_batch_reuse(dev):
    """Every region of the tests above in one call, shuffled among reads without a region; a second order gives the same
    per-region results; then, on the same batch, no region at all, a small call, and the large one again: class lists,
    counters and scratch offsets of an earlier call must not show."""
    g, _, ix = dev
    c = _everything(g)
    rng = np.random.default_rng(5)
    o1, o2 = rng.permutation(len(c.reads)), rng.permutation(len(c.reads))
    b = capi.Batch(ix, len(c.reads), sum(len(r) for r in c.reads))
    m, _, cnt, got1 = _run(dev, c, {}, order=o1, batch=b)
    assert len(m) >= 800 and cnt.min() >= 16
    first = _per_region(c, o1, got1)

    empty = ac.Cases(g)
    for r in c.reads[:50]:
        empty.reads.append(r); empty.regs.append([]); empty.tags.append("bare")
    m, _, cnt0, got = _run(dev, empty, {}, batch=b)
    assert len(m) == 0 and len(got[0]) == 0 and not cnt0.any()

    small = ac.retry_cases(g, ac.opts()[0], "wave")          # under w = 100 here: other routes than under w = 5
    _run(dev, small, {}, batch=b)
    _, _, cnt2, got2 = _run(dev, c, {}, order=o2, batch=b)
    assert _per_region(c, o2, got2) == first and np.array_equal(cnt2, cnt)
    _run(dev, small, {}, batch=b)
    b.close()


def test_hook_refusals(dev):
    """bwams_debug_regs_upload refuses what would make a kernel read outside the reads, with BWAMS_ERR_ARG, and leaves the batch
    as it was: the regions uploaded before still give their result."""
    g, idx, ix = dev
    c = ac.routing_cases(g, ac.opts()[0])
    flat = c.flat()
    enc, cum, regs, off, _ = flat
    oopt, gopt = ac.opts()
    b = capi.Batch(ix, len(cum) - 1, int(cum[-1]))
    b.seed_upload(enc, cum)
    with pytest.raises(capi.BwamsError) as e:                  # nothing uploaded yet: no run either
        b.debug_aln_lists()
    assert e.value.code == -3
    b.debug_regs_upload(regs, off)
    want = loader.reg2aln(regs, off, enc, cum, idx.ref_0123, len(g), opt=oopt)
    _check(b.reg2aln(gopt, 0), want)
    cnt = b.debug_aln_lists()

    def refused(r, o):
        with pytest.raises(capi.BwamsError) as e:
            b.debug_regs_upload(r, o)
        assert e.value.code == -3
        _check(b.reg2aln(gopt, 0), want)
        assert np.array_equal(b.debug_aln_lists(), cnt)

    refused(regs[:int(off[-2])], off[:-1])                     # one read fewer than uploaded
    refused(regs, np.concatenate([off, off[-1:]]))             # one read more
    o = off.copy(); o[0] = 1
    refused(regs, o)                                           # does not start at 0
    o = off.copy(); o[-1] -= 1
    refused(regs, o)                                           # does not end at n_regs
    o = off.copy(); o[3], o[4] = off[4], off[3]
    assert o[4] < o[3]
    refused(regs, o)                                           # decreases
    k = int(off[5])
    for f, v in (("qb", -1), ("qe", int(cum[6] - cum[5]) + 1), ("qb", int(regs["qe"][k]) + 1)):
        r = regs.copy(); r[f][k] = v
        refused(r, off)
    r = regs.copy(); r["qb"][k] = r["qe"][k]                   # an empty query span is the plan rule's to reject, not the hook's
    b.debug_regs_upload(r, off)
    got = b.reg2aln(gopt, 0)
    assert got[0]["flag"][k] == 4 and got[0]["rid"][k] == -1
    _check(got, loader.reg2aln(r, off, enc, cum, idx.ref_0123, len(g), opt=oopt))
    b.close()
