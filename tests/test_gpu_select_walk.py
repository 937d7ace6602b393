"""The selection walk of the wave tier (ext_select_wave_kernel: 64 slots per batch, every lane its own seed against the regions
kept before the batch, then the slots in order with each newly kept region broadcast to the lanes behind it) against the CPU oracle
(loader.chain2aln) on an input chosen for the two places where such a walk can go wrong: a slot explained by a region kept in an
earlier batch beside one kept in the same batch, and an overlap rescue that reads a purge made earlier in the same batch.  Tandem
arrays of short periods give reads with hundreds of seeds on neighbouring diagonals: a region explains seeds hundreds of slots
behind it, and many explained seeds are kept by the rescue.  Integer work: every comparison is bit-exact."""
import numpy as np
import pytest

from bwams import capi, fmindex, simulate
from test_gpu_chain import _indel_reads
from test_gpu_ext_rounds import TIER_EDGES, _batch, _extend, _oracle, _tier_genome, knobs  # noqa: F401  (knobs: a fixture)

pytestmark = pytest.mark.gpu

BATCH = 64                                   # slots the wave tier decides together (ext_aln.hip)
MAX_OCC = 3000
MODES = {"natural": dict(BWAMS_EXT_ALL_ROUNDS="1"), "long": dict(BWAMS_EXT_ALL_ROUNDS="1", BWAMS_EXT_MAX_ROUNDS="64"), "default": {}}


def _walk_input():
    """5 kb random, then for each period p in (23, 37, 61) 1200 copies of a random p-mer with 1 % substitutions and 5 kb random
    behind them; 12 reads of 150 bases per array, 1 % substitutions."""
    rng = np.random.default_rng(11)

    def rnd(n):
        return rng.integers(0, 4, size=n, dtype=np.uint8)

    def mutate(x, rate):
        x = x.copy()
        m = rng.random(len(x)) < rate
        x[m] = (x[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
        return x

    parts, arrays, at = [rnd(5000)], [], 5000
    for p in (23, 37, 61):
        parts.append(mutate(np.tile(rnd(p), 1200), 0.01))
        arrays.append((at, at + 1200 * p))
        parts.append(rnd(5000))
        at += 1200 * p + 5000
    g = np.concatenate(parts).astype(np.uint8)
    reads = []
    for b, e in arrays:
        for st in rng.integers(b, e - 150, size=12):
            reads.append(mutate(g[int(st):int(st) + 150], 0.01))
    return g, reads


def _max_gap(opt, qlen):
    """cal_max_gap (bwamem.cpp:94-104) on an array; the casts to int truncate"""
    l_del = np.trunc((qlen * opt.a - opt.o_del) / float(opt.e_del) + 1.).astype(np.int64)
    l_ins = np.trunc((qlen * opt.a - opt.o_ins) / float(opt.e_ins) + 1.).astype(np.int64)
    return np.minimum(np.maximum(np.maximum(l_del, l_ins), 1), opt.w << 1)


def _explains(opt, s, l_query, K):
    """[slot, kept region] -> does the region explain the slot's seed: the purge test of mem_chain2aln_across_reads_V2
    (bwamem.cpp:3648-3755) restated — containment, the seedlen0 rule, then the two cal_max_gap tests"""
    rbeg, qbeg, ln = s["rbeg"][:, None], s["qbeg"].astype(np.int64)[:, None], s["len"].astype(np.int64)[:, None]
    rb, re, qb, qe = K["rb"][None, :], K["re"][None, :], K["qb"].astype(np.int64)[None, :], K["qe"].astype(np.int64)[None, :]
    ok = ~((qb == -1) & (qe == -1)) & ~((rbeg < rb) | (rbeg + ln > re) | (qbeg < qb) | (qbeg + ln > qe))
    ok &= ~((ln - K["seedlen0"][None, :]).astype(np.float64) > .1 * l_query)
    pw = K["w"].astype(np.int64)[None, :]
    qd, rd = qbeg - qb, rbeg - rb
    w = np.minimum(_max_gap(opt, np.minimum(qd, rd)), pw)
    yes = (qd - rd < w) & (rd - qd < w)
    qd, rd = qe - (qbeg + ln), re - (rbeg + ln)
    w = np.minimum(_max_gap(opt, np.minimum(qd, rd)), pw)
    yes |= (qd - rd < w) & (rd - qd < w)
    return ok & yes


def _replay(w, opt):
    """the decisions of every read's walk from the oracle's output: per slot (purged, explained from >= BATCH slots back, explained
    from nearer).  A read's slots are its chains in order; inside a chain the seeds go by descending (score << 32 | index)."""
    chains, seeds, regs, reg_off, cum = w["chains"], w["wseeds"], w["wregs"], w["wreg_off"], w["cum"]
    n = len(regs)
    slot_seed = np.zeros(n, np.int64)
    for c in chains:
        o, k = int(c["seed_off"]), int(c["n"])
        key = (seeds["score"][o:o + k].astype(np.int64) << 32) | np.arange(k)
        slot_seed[o:o + k] = o + np.argsort(-key)
    # the oracle's own record of where each seed's region lies agrees with that order
    seqid = np.repeat(chains["seqid"], chains["n"])
    assert np.array_equal(reg_off[seqid[slot_seed]] + seeds["aln"][slot_seed], np.arange(n))
    purged = (regs["qb"] == -1) & (regs["qe"] == -1)
    far, near = np.zeros(n, bool), np.zeros(n, bool)
    for r in range(len(reg_off) - 1):
        a, b = int(reg_off[r]), int(reg_off[r + 1])
        kept = np.flatnonzero(~purged[a:b])                  # slots of the read, by their place in it
        if b == a or len(kept) == 0:
            continue
        e = _explains(opt, seeds[slot_seed[a:b]], int(cum[r + 1] - cum[r]), regs[a + kept])
        back = np.arange(b - a)[:, None] - kept[None, :]     # how many slots before the seed's the region was kept
        far[a:b] = (e & (back >= BATCH)).any(axis=1)
        near[a:b] = (e & (back > 0) & (back < BATCH)).any(axis=1)
    return purged, far, near


def _conditions(w, opt):
    """conditions on the input, from the oracle alone"""
    n_regs = np.diff(w["wreg_off"])
    tiers = np.bincount(np.searchsorted(TIER_EDGES, n_regs, side="left"), minlength=5)
    purged, far, near = _replay(w, opt)
    only_far, both = int((purged & far & ~near).sum()), int((purged & far & near).sum())
    rescued = int((~purged & (far | near)).sum())
    print("reads", len(n_regs), "slots", len(purged), "heaviest", int(n_regs.max()), "per tier (<=32, <=256, <=640, <=1280, beyond)",
          tiers.tolist(), "purged", int(purged.sum()), "only from >=64 back", only_far, "from both sides", both, "kept", int((~purged).sum()),
          "kept although explained", rescued)
    assert (tiers > 0).all(), tiers
    assert (far | near)[purged].all()                        # every purged slot has an earlier kept region that explains it
    assert only_far >= 100 and both >= 50 and rescued >= 100


@pytest.fixture(scope="module")
def alone():
    """the 36 reads on their genome"""
    capi.lib()
    g, reads = _walk_input()
    idx = fmindex.build_fmindex(g)
    ix = capi.Index.from_host(idx, 0)
    c = np.zeros(1, capi.CONTIG_DTYPE)
    c["len"] = len(g)
    ix.set_contigs(c)
    w = _oracle(idx, g, reads, max_occ=MAX_OCC)
    _conditions(w, w["gopt"])
    yield ix, w
    ix.close()


@pytest.fixture(scope="module")
def mixed():
    """the reads of test_gpu_ext_rounds' `tiered` chunk with the 36 behind them, on the two genomes one after the other: lane tier,
    every class and the HBM fallback in one chunk and one ticket list"""
    capi.lib()
    g1 = _tier_genome()
    g2, reads2 = _walk_input()
    reads = list(simulate.make_reads(g1, 1500, seed=3)[0]) + _indel_reads(g1)
    n1 = len(reads)
    g = np.concatenate([g1, g2]).astype(np.uint8)
    idx = fmindex.build_fmindex(g)
    ix = capi.Index.from_host(idx, 0)
    c = np.zeros(1, capi.CONTIG_DTYPE)
    c["len"] = len(g)
    ix.set_contigs(c)
    w = _oracle(idx, g, reads + reads2, max_occ=MAX_OCC)
    tail = dict(w)                                            # the conditions hold for the 36 reads inside the larger chunk too
    o = int(w["wreg_off"][n1])
    first = int(np.searchsorted(w["chains"]["seqid"], n1))
    assert o == (int(w["chains"]["seed_off"][first]) if first < len(w["chains"]) else len(w["wregs"]))
    ch = w["chains"][first:].copy()
    ch["seed_off"] -= o
    ch["seqid"] -= n1
    tail.update(chains=ch, wseeds=w["wseeds"][o:], wregs=w["wregs"][o:], wreg_off=w["wreg_off"][n1:] - o,
                cum=w["cum"][n1:] - w["cum"][n1])
    _conditions(tail, w["gopt"])
    yield ix, w
    ix.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("chunk", ["alone", "mixed"])
def test_walk_matches_oracle(request, knobs, chunk, mode):
    """regions, offsets and aln equal the oracle's (asserted by _extend); with the rounds not cut short the walks stop at a request
    and resume inside their batches"""
    ix, w = request.getfixturevalue(chunk)
    knobs(**MODES[mode])
    b = _batch(ix, w)
    st = _extend(b, w)[3]
    print(chunk, mode, "rounds", st.n_ext_rounds, "tasks", st.n_left, st.n_right)
    if mode != "default":
        assert st.n_ext_rounds >= 3
    b.close()


def test_two_runs_give_the_same(mixed, knobs):
    ix, w = mixed
    knobs()
    b = _batch(ix, w)
    r1 = _extend(b, w)
    r2 = _extend(b, w)
    for x, y in zip(r1[:3], r2[:3]):
        assert x.tobytes() == y.tobytes()
    assert r1[3].n_ext_rounds == r2[3].n_ext_rounds
    b.close()


def test_flat_task_buffers(mixed, knobs):
    """BWAMS_EXT_INPLACE=0: the flat task buffers built over the request list"""
    ix, w = mixed
    knobs(BWAMS_EXT_INPLACE="0")
    b = _batch(ix, w)
    _extend(b, w)
    b.close()
