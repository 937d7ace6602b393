"""The dense suffix-array table (csrc/fmi_sal.hip, api_index.hip) on the toy indexes of tests/sa_dense_cases.py: its entries, the
lookups through it at every stride, the re-run behind a grown coordinate buffer, refusal, giving way, and giving way under two
seeding threads.  The table is built once per index, so every setting gets an index handle of its own."""
import threading

import numpy as np
import pytest

from bwams import capi

import sa_dense_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = ("rid", "m", "n", "k", "l", "s")


def _setting(monkeypatch, stride, **env):
    monkeypatch.setenv("BWAMS_SA_DENSE", str(stride))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capi.debug_reload()


def _gopt(opt):
    g = capi.default_seed_opt()
    g.min_seed_len, g.split_factor, g.split_width, g.max_mem_intv, g.max_occ = (opt.min_seed_len, opt.split_factor, opt.split_width,
                                                                               opt.max_mem_intv, opt.max_occ)
    return g


def _seed(ix, L, max_occ, max_sa=None):
    """one seeding pass of the case's reads on a batch of its own: (smems, coord, off, n_sa_lookups, n_lf_steps)"""
    enc, cum = cases.reads(L)
    sm, coord, off, ctr, opt = cases.oracle_seeds(L, max_occ)
    b = capi.Batch(ix, len(cum) - 1, int(cum[-1]), max_smem=len(sm) + 64, max_sa=max_sa if max_sa is not None else len(coord) + 64)
    got = b.seed(enc, cum, _gopt(opt))
    st = b.stats()
    b.close()
    return got + (st.n_sa_lookups, st.n_lf_steps)


def _assert_oracle(got, L, max_occ, what):
    sm, coord, off, ctr, _ = cases.oracle_seeds(L, max_occ)
    gsm, gcoord, goff, n_sa, n_lf = got
    assert len(gsm) == len(sm), what
    for f in FIELDS:
        assert np.array_equal(gsm[f], sm[f]), (what, f)
    assert np.array_equal(goff, off), what
    assert np.array_equal(gcoord, coord), what
    assert n_sa == ctr.n_sa_lookups and n_lf == ctr.n_lf_steps, (what, n_sa, ctr.n_sa_lookups, n_lf, ctr.n_lf_steps)


@pytest.mark.parametrize("L", cases.SIZES)
@pytest.mark.parametrize("stride", (1, 2, 4))
def test_whole_table(monkeypatch, L, stride):
    """every entry — coordinate, step count, sentinel flag, row 0 and the last row included — is the oracle's walk from its row"""
    _setting(monkeypatch, stride)
    _, idx = cases.case(L)
    ix = capi.Index.from_host(idx, 0)
    try:
        assert ix.sa_dense_state()[0] == "absent"
        before = ix.nbytes
        _seed(ix, L, 500)
        state, s, nbytes, _ = ix.sa_dense_state()
        want = cases.expected_table(L, stride)
        assert (state, s, nbytes) == ("built", stride, 8 * len(want))
        assert ix.nbytes == before                                   # the index's own arrays: a used handle reports what a fresh one does
        got = ix.sa_dense_fetch()
        assert len(got) == len(want)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"entries {bad[:8]} (rows {bad[:8] * stride}): {got[bad[:8]]} vs {want[bad[:8]]}"
    finally:
        ix.close()


@pytest.mark.parametrize("L", cases.SIZES)
@pytest.mark.parametrize("max_occ", (500, 3))
def test_lookup_parity(monkeypatch, L, max_occ):
    """sa_off, every coordinate, n_sa_lookups and n_lf_steps under BWAMS_SA_DENSE = 0, 1, 2, 4 equal the oracle's, hence one another"""
    _, idx = cases.case(L)
    for stride in (0, 1, 2, 4):
        _setting(monkeypatch, stride)
        ix = capi.Index.from_host(idx, 0)
        try:
            got = _seed(ix, L, max_occ)
            assert ix.sa_dense_state()[0] == ("built" if stride else "absent")
            _assert_oracle(got, L, max_occ, f"stride {stride}")
            _assert_oracle(_seed(ix, L, max_occ), L, max_occ, f"stride {stride}, second pass")     # the table is there already
        finally:
            ix.close()


@pytest.mark.parametrize("stride", (1, 4))
def test_small_coordinate_buffer(monkeypatch, stride):
    """a batch whose max_sa is too small: bwams_seed_counts grows the buffer and runs the lookup again, through the table"""
    L = 1000
    _setting(monkeypatch, stride)
    _, idx = cases.case(L)
    ix = capi.Index.from_host(idx, 0)
    try:
        assert len(cases.oracle_seeds(L, 500)[1]) > 16
        _assert_oracle(_seed(ix, L, 500, max_sa=16), L, 500, "max_sa = 16")
        assert ix.sa_dense_state()[0] == "built"
    finally:
        ix.close()


def test_refusal(monkeypatch):
    """a cap below the table's size: the state is "refused", nothing is resident for it, and the walk gives the same results"""
    L = 2051
    _setting(monkeypatch, 2, BWAMS_SA_DENSE_MAX_BYTES="1")
    _, idx = cases.case(L)
    ix = capi.Index.from_host(idx, 0)
    try:
        before = ix.nbytes
        _assert_oracle(_seed(ix, L, 500), L, 500, "refused")
        assert ix.sa_dense_state()[0] == "refused" and ix.sa_dense_state()[2] == 0 and ix.nbytes == before
        with pytest.raises(capi.BwamsError):
            ix.sa_dense_fetch()
        _assert_oracle(_seed(ix, L, 3), L, 3, "refused, second pass")
        assert ix.sa_dense_state()[0] == "refused"
    finally:
        ix.close()


def test_giving_way(monkeypatch):
    """the routine the allocator calls on out-of-memory: the table goes, the results stay, it is not built again, and a second index
    on the device — with a table, which goes too, and one made afterwards, which builds its own — keeps working"""
    _setting(monkeypatch, 2)
    ix = capi.Index.from_host(cases.case(2051)[1], 0)
    ix2 = capi.Index.from_host(cases.case(1000)[1], 0)
    ix3 = None
    try:
        _assert_oracle(_seed(ix, 2051, 500), 2051, 500, "before")
        _assert_oracle(_seed(ix2, 1000, 3), 1000, 3, "second index before")
        assert ix.sa_dense_state()[0] == ix2.sa_dense_state()[0] == "built"
        assert ix.sa_dense_state()[2] == 8 * len(cases.expected_table(2051, 2))
        assert capi.sa_dense_release(0) >= 2
        assert ix.sa_dense_state()[0] == ix2.sa_dense_state()[0] == "yielded"
        assert ix.sa_dense_state()[2] == 0 and ix2.sa_dense_state()[2] == 0
        _assert_oracle(_seed(ix, 2051, 500), 2051, 500, "after")
        _assert_oracle(_seed(ix2, 1000, 3), 1000, 3, "second index after")
        assert ix.sa_dense_state()[0] == ix2.sa_dense_state()[0] == "yielded"      # no rebuild
        assert capi.sa_dense_release(0) == 0
        ix3 = capi.Index.from_host(cases.case(100)[1], 0)
        _assert_oracle(_seed(ix3, 100, 500), 100, 500, "an index opened afterwards")
        assert ix3.sa_dense_state()[0] == "built"
    finally:
        ix.close(); ix2.close()
        if ix3 is not None:
            ix3.close()


def test_release_under_two_seeding_threads(monkeypatch):
    """two batches on two host threads seed one index, pass after pass, while the main thread releases its table: every pass of both
    gives the oracle's result, whichever side of the release it fell on"""
    L = 2051
    _setting(monkeypatch, 1)
    _, idx = cases.case(L)
    ix = capi.Index.from_host(idx, 0)
    try:
        _assert_oracle(_seed(ix, L, 500), L, 500, "first pass")
        assert ix.sa_dense_state()[0] == "built"
        cases.oracle_seeds(L, 3)                                     # the shared reference is computed here, not in the threads
        started, errors = threading.Barrier(3), []

        def work(max_occ):
            try:
                started.wait()
                for i in range(6):
                    _assert_oracle(_seed(ix, L, max_occ), L, max_occ, f"thread max_occ {max_occ}, pass {i}")
            except BaseException as e:      # noqa: BLE001 — reported by the main thread
                errors.append(e)

        ts = [threading.Thread(target=work, args=(m,)) for m in (500, 3)]
        for t in ts:
            t.start()
        started.wait()
        n = capi.sa_dense_release(0)
        for t in ts:
            t.join()
        assert not errors, errors
        assert n >= 1 and ix.sa_dense_state()[0] == "yielded"
    finally:
        ix.close()


@pytest.mark.parametrize("rl", (255, 256))
def test_sort_key_fields_at_the_boundary(monkeypatch, rl):
    """reads of 255 bases sort by 8-bit position fields, reads of 256 by 16-bit ones: the (rid, m, n) order of the SMEMs — a chunk of
    several waves, whose pool has holes — is the oracle's, and the one BWAMS_SORT_NARROW=0 gives"""
    from util import toy
    from oracle import loader
    g, idx = toy(20000)
    rng = np.random.default_rng(rl)
    reads = []
    for _ in range(700):
        at = int(rng.integers(0, len(g) - rl))
        r = g[at:at + rl].copy()
        for _ in range(int(rng.integers(0, 6))):
            r[int(rng.integers(0, rl))] = rng.integers(0, 4)
        reads.append(r)
    reads.append(g[100:160].copy())                                  # a short read among them: the longest read decides
    enc = np.concatenate(reads)
    cum = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    want = loader.OracleFMI(idx).collect_smem(enc, cum)
    assert want["n"].max() >= rl - 1 and len(want) > 256
    ix = capi.Index.from_host(idx, 0)
    try:
        got = {}
        for narrow in ("1", "0"):
            monkeypatch.setenv("BWAMS_SORT_NARROW", narrow)
            capi.debug_reload()
            b = capi.Batch(ix, len(reads), int(cum[-1]), max_smem=len(want) + 64, max_sa=64)
            got[narrow] = b.seed(enc, cum, with_sa=False)[0]
            b.close()
            for f in FIELDS:
                assert np.array_equal(got[narrow][f], want[f]), (narrow, f)
    finally:
        ix.close()
