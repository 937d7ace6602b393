"""Extension rounds driven from the request list: regions against the CPU oracle (loader.chain2aln) on chunks chosen for what a
round holds — reads in every tier of the selection walk, rounds with nothing on one side, empty request lists, a batch reused for
chunks of very different sizes.  Integer work: every comparison is bit-exact."""
import numpy as np
import pytest

from bwams import capi, fmindex, simulate
from oracle import loader
from test_gpu_chain import _assert_regs, _indel_reads, _mem_opts

pytestmark = pytest.mark.gpu

TIER_EDGES = (32, 256, 640, 1280)            # the selection's lane tier and the three LDS classes of its wave tier (ext_aln.hip)


def _tier_genome():
    """20 kb random, 1500 copies of a 171-bp monomer (2 % substitutions), 20 kb random, 300 copies of a second monomer (the first with
    30 % of its bases changed; 3 %), 20 kb random, 60 copies of a third (3 %), 20 kb random: reads from the arrays carry from a handful
    to far more than a thousand seeds, and the three arrays differ in how many of them a region of the read explains."""
    rng = np.random.default_rng(5)

    def rnd(n):
        return rng.integers(0, 4, size=n, dtype=np.uint8)

    def mutate(x, rate):
        x = x.copy()
        m = rng.random(len(x)) < rate
        x[m] = (x[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
        return x

    m1 = rnd(171)
    m2 = mutate(m1, 0.30)
    m3 = rnd(171)
    parts = [rnd(20000), mutate(np.tile(m1, 1500), 0.02), rnd(20000), mutate(np.tile(m2, 300), 0.03), rnd(20000),
             mutate(np.tile(m3, 60), 0.03), rnd(20000)]
    return np.concatenate(parts).astype(np.uint8)


@pytest.fixture(scope="module")
def tiered():
    capi.lib()
    g = _tier_genome()
    idx = fmindex.build_fmindex(g)
    ix = capi.Index.from_host(idx, 0)
    c = np.zeros(1, capi.CONTIG_DTYPE)
    c["len"] = len(g)
    ix.set_contigs(c)
    reads = list(simulate.make_reads(g, 1500, seed=3)[0]) + _indel_reads(g)
    yield g, idx, ix, reads
    ix.close()


@pytest.fixture(scope="module")
def plain():
    """a genome without repeats: one chain per read, seeds on one diagonal"""
    capi.lib()
    g = simulate.make_genome(60000, seed=17, repeat_frac=0.0)
    idx = fmindex.build_fmindex(g)
    ix = capi.Index.from_host(idx, 0)
    c = np.zeros(1, capi.CONTIG_DTYPE)
    c["len"] = len(g)
    ix.set_contigs(c)
    yield g, idx, ix
    ix.close()


@pytest.fixture
def knobs(monkeypatch):
    def set_(**kw):
        for k in ("BWAMS_EXT_ALL_ROUNDS", "BWAMS_EXT_MAX_ROUNDS", "BWAMS_EXT_INPLACE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv(k, v)
        capi.debug_reload()                                   # the switches are read once: say that they changed
    yield set_
    monkeypatch.undo()
    capi.debug_reload()


def _oracle(idx, g, reads, **mem_kw):
    enc, cum = simulate.flatten_reads(reads)
    oopt, gopt = _mem_opts(**mem_kw)
    so, sg = loader.default_seed_opt(), capi.default_seed_opt()
    so.max_occ = sg.max_occ = oopt.max_occ
    o = loader.OracleFMI(idx)
    sm = o.collect_smem(enc, cum, so)
    coord, off = o.sa_lookup(sm, so.max_occ)
    l_pac = len(g)
    ref = np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])
    chains, seeds, chain_off = loader.chain_seeds(sm, coord, off, cum, l_pac, opt=oopt, ref_string=ref, enc=enc)
    wregs, wreg_off, wseeds = loader.chain2aln(chains, seeds, chain_off, enc, cum, ref, l_pac, opt=oopt)
    return dict(enc=enc, cum=cum, sg=sg, gopt=gopt, n_smem=len(sm), n_sa=len(coord), chains=chains, seeds=seeds, wregs=wregs,
                wreg_off=wreg_off, wseeds=wseeds)


def _batch(ix, w):
    return capi.Batch(ix, max(len(w["cum"]) - 1, 1), max(int(w["cum"][-1]), 1), max_smem=w["n_smem"] + 4096, max_sa=w["n_sa"] + 4096)


def _extend(b, w):
    """the chunk through seeding, chaining and the extension rounds on batch b; regions compared with the oracle's"""
    b.seed_upload(w["enc"], w["cum"])
    b.seed_run(w["sg"], with_sa=True)
    b.chain_run(w["gopt"])
    n = b.extend_run(w["gopt"])
    regs, reg_off, aln = b.extend_fetch()
    assert n == len(w["wregs"]) and np.array_equal(reg_off, w["wreg_off"]) and np.array_equal(aln, w["wseeds"]["aln"])
    _assert_regs(regs, w["wregs"], False)
    return regs, reg_off, aln, b.stats()


@pytest.fixture(scope="module")
def tiered_want(tiered):
    g, idx, ix, reads = tiered
    w = _oracle(idx, g, reads, max_occ=2000)
    # conditions on the input, from the oracle alone: every tier of the selection holds at least one read
    n_regs = np.diff(w["wreg_off"])
    tiers = np.bincount(np.searchsorted(TIER_EDGES, n_regs, side="left"), minlength=5)
    print("reads per tier (<=32, <=256, <=640, <=1280, beyond):", tiers.tolist(), "most regions of a read:", int(n_regs.max()))
    assert (tiers > 0).all(), tiers
    return w


@pytest.mark.parametrize("mode", ["natural", "long", "default", "flat"])
def test_every_tier_of_the_selection(tiered, tiered_want, knobs, mode):
    """natural: BWAMS_EXT_ALL_ROUNDS=1, the rounds are not cut short while something is requested (the cap of six rounds holds); long:
    the cap raised to 64 as well; default: the rest is extended at once when little is left; flat: BWAMS_EXT_INPLACE=0, the flat task
    buffers built over the request list."""
    ix = tiered[2]
    knobs(**{"natural": dict(BWAMS_EXT_ALL_ROUNDS="1"), "long": dict(BWAMS_EXT_ALL_ROUNDS="1", BWAMS_EXT_MAX_ROUNDS="64"), "default": {}, "flat": dict(BWAMS_EXT_INPLACE="0")}[mode])
    b = _batch(ix, tiered_want)
    st = _extend(b, tiered_want)[3]
    print(mode, "rounds", st.n_ext_rounds, "tasks", st.n_left, st.n_right)
    if mode in ("natural", "long"):
        assert st.n_ext_rounds >= 3
    b.close()


def test_two_runs_give_the_same(tiered, tiered_want, knobs):
    """the order of the tasks inside a round is unspecified; nothing that leaves the library is"""
    knobs()
    b = _batch(tiered[2], tiered_want)
    r1 = _extend(b, tiered_want)
    r2 = _extend(b, tiered_want)
    for x, y in zip(r1[:3], r2[:3]):
        assert x.tobytes() == y.tobytes()
    assert r1[3].n_left + r1[3].n_right == r2[3].n_left + r2[3].n_right and r1[3].bsw_cells == r2[3].bsw_cells
    assert r1[3].n_ext_rounds == r2[3].n_ext_rounds
    b.close()


def _one_sided_reads(g, left_free: bool):
    """a stretch of the genome with random bases behind it (left_free: every seed starts at query position 0) or in front of it"""
    rng = np.random.default_rng(7)
    out = []
    for _ in range(300):
        st = int(rng.integers(0, len(g) - 200))
        n = int(rng.integers(21, 29))                         # below the length at which a seed is split again: one seed per read
        junk = rng.integers(0, 4, size=150 - n, dtype=np.uint8)
        r = np.concatenate([g[st:st + n], junk]) if left_free else np.concatenate([junk, g[st:st + n]])
        out.append(r)
    return out


@pytest.mark.parametrize("left_free", [True, False])
def test_rounds_with_one_side_empty(plain, knobs, left_free):
    g, idx, ix = plain
    knobs()
    w = _oracle(idx, g, _one_sided_reads(g, left_free))
    sd, ch = w["seeds"], w["chains"]
    assert len(sd) > 100
    qlen = np.diff(w["cum"])[np.repeat(ch["seqid"], ch["n"])]
    if left_free:                                             # a condition on the input: no seed has anything to its left ...
        assert (sd["qbeg"] == 0).all() and (sd["qbeg"] + sd["len"] < qlen).any()
    else:                                                     # ... or to its right
        assert (sd["qbeg"] + sd["len"] == qlen).all() and (sd["qbeg"] > 0).any()
    b = _batch(ix, w)
    st = _extend(b, w)[3]
    assert (st.n_left == 0 and st.n_right > 0) if left_free else (st.n_right == 0 and st.n_left > 0)
    b.close()


def test_empty_request_lists(plain, knobs):
    """one read; reads without any chain; a chunk that round 0 settles (exact reads have no task at all, reads with one mismatch
    one chain whose first region explains the other seed): one build..select pass, nothing requested by its selection"""
    g, idx, ix = plain
    knobs()
    rng = np.random.default_rng(11)
    w = _oracle(idx, g, [g[1000:1150]])
    b = _batch(ix, w)
    assert _extend(b, w)[3].n_ext_rounds == 1
    b.close()
    w = _oracle(idx, g, [rng.integers(0, 4, size=150, dtype=np.uint8) for _ in range(64)])
    assert len(w["chains"]) == 0 and len(w["wregs"]) == 0
    b = _batch(ix, w)
    st = _extend(b, w)[3]
    assert st.n_ext_rounds == 1 and st.n_left + st.n_right == 0
    b.close()
    reads = []
    for k in range(400):
        s0 = int(rng.integers(0, len(g) - 150))
        r = g[s0:s0 + 150].copy()
        if k % 2:
            r[75] = (r[75] + 1) & 3
        reads.append(r)
    w = _oracle(idx, g, reads)
    b = _batch(ix, w)
    st = _extend(b, w)[3]
    assert st.n_ext_rounds == 1 and st.n_left + st.n_right > 0
    b.close()


def test_batch_reused_for_smaller_and_larger_chunks(tiered, tiered_want, knobs):
    """entries that a larger chunk left in the lists, and its counters, are not read by the chunks that follow"""
    g, idx, ix, reads = tiered
    knobs()
    small = _oracle(idx, g, reads[:7], max_occ=2000)
    tiny = _oracle(idx, g, reads[40:41], max_occ=2000)
    b = _batch(ix, tiered_want)
    big1 = _extend(b, tiered_want)
    _extend(b, small)
    _extend(b, tiny)
    big2 = _extend(b, tiered_want)
    _extend(b, small)
    for x, y in zip(big1[:3], big2[:3]):
        assert x.tobytes() == y.tobytes()
    assert big1[3].n_left + big1[3].n_right == big2[3].n_left + big2[3].n_right
    b.close()
