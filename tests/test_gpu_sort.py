"""The device sorts (csrc/ksort.h) as the wave tiers run them (bwams_debug_sort) — the region sorts of mem_sort_dedup_patch
(which = 0, 1) and the chain filter's sort by weight (which = 2): ksort.h's introsort is not
stable, so on tied keys only the same sequence of comparisons and swaps gives the reference's order.  Checked against
the reference's own ks_introsort (oracle/_ref/libref_chain.so when present, else the restatement pinned to it) on inputs
with heavy ties, including every small size (the six-record case of profiles/r01_notes.md item 20 among them), sorted /
reversed / organ-pipe inputs that reach the comb-sort depth fallback, and sizes up to the LDS limit of the largest instance
of de-duplication's wave tier (2048 records)."""
import numpy as np
import pytest

from bwams import capi
from chain_cases import antiquicksort as _antiquicksort      # the adversary against ksort.h's introsort, shared with the chaining cases
from oracle import loader
from util import toy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ix():
    _, idx = toy(3000)
    h = capi.Index.from_host(idx, 0)
    yield h
    h.close()


def _want(which, k, s, q, L):
    if which == 0:
        return loader.ars_sort(0, k, L=L)
    return loader.ars_sort(1, s, k, q, L=L)


def _cases():
    rng = np.random.default_rng(7)
    out = []
    for n in list(range(0, 40)) + [63, 64, 65, 100, 129, 300, 777, 1024]:
        for spread in (1, 2, 3, 8, 1 << 20):                   # 1: all keys equal ... 2^20: hardly any tie
            k = rng.integers(0, spread, size=n)
            s = rng.integers(0, min(spread, 4), size=n)
            q = rng.integers(0, 2, size=n)
            out.append((k, s, q))
    for n in (17, 64, 200, 1000):                               # shapes that drive the quicksort to its depth limit
        a = np.arange(n)
        for k in (a, a[::-1], np.minimum(a, n - 1 - a), np.where(a % 2 == 0, a, n - a), np.zeros(n, dtype=np.int64)):
            out.append((k.astype(np.int64), (k % 3).astype(np.int64), (k % 2).astype(np.int64)))
    return out


def test_wave_tier_sorts_equal_ksort(ix):
    L = loader.ref_chain_lib()
    n_tied = 0
    for k, s, q in _cases():
        for which in (0, 1):
            want = _want(which, k, s, q, L)
            for mode in (0, 1, 2):
                got = ix.debug_sort(k, s, q, which, mode)
                assert np.array_equal(got, want), (len(k), which, mode, k[:12], got[:12], want[:12])
            n_tied += len(k) > len(np.unique(k))
    assert n_tied > 100


def test_largest_instance_sizes(ix):
    """1025 to 2048 records — what only the largest instance of de-duplication's wave tier sorts, two arrays of 2048 records in
    dynamic LDS: hardly any tie, keys that tie by the hundred, keys that are all equal; both orders, the three modes."""
    L = loader.ref_chain_lib()
    rng = np.random.default_rng(13)
    for n in (1025, 1537, 2047, 2048):
        for spread in (1 << 20, max(n // 100, 2), 1):
            k = rng.integers(0, spread, size=n)
            s = rng.integers(0, spread, size=n) if spread > 1 else np.zeros(n, np.int64)
            q = rng.integers(0, 2 if spread > 1 else 1, size=n)
            for which in (0, 1):
                want = _want(which, k, s, q, L)
                for mode in (0, 1, 2):
                    got = ix.debug_sort(k, s, q, which, mode)
                    assert np.array_equal(got, want), (n, spread, which, mode, got[:12], want[:12])
    with pytest.raises(capi.BwamsError):
        ix.debug_sort(np.zeros(2049, np.int64), np.zeros(2049, np.int64), np.zeros(2049, np.int64), 0, 0)


def test_chain_filter_sort_equals_ksort(ix):
    """which = 2: weights descending, as heavy_read (wave form, modes 0 and 1) and chain_read (sequential form, mode 2) sort a
    read's chains; 64 / 65 is where the wave form's closing sort changes from the rank sort to the key network, 129 the first
    size whose network (P = 256) has virtual pads."""
    L = loader.ref_chain_lib()
    n_tied = 0
    for w, _, _ in _cases():
        want = loader.flt_sort(w, L)
        for mode in (0, 1, 2):
            got = ix.debug_sort(w, w, w, 2, mode)
            assert np.array_equal(got, want), (len(w), mode, w[:12], got[:12], want[:12])
        n_tied += len(w) > len(np.unique(w))
    assert n_tied > 100


def test_depth_limit_fallback(ix):
    """The comb-sort fallback of ks_introsort's depth limit in the wave tiers (wave_ks_combsort: the whole wavefront, no lane
    sorting alone on LDS): (a) an adversarial permutation on which ksort.h itself exhausts its depth budget — the order must be
    the pinned ks_introsort's; (b) a depth budget of 2 on inputs of every kind — the wave form must equal the sequential form
    operation for operation (ties included)."""
    L = loader.ref_chain_lib()
    for n in (200, 700, 1024):
        k, hit = _antiquicksort(n)
        assert hit, n                                              # the construction really drives ksort to its fallback
        s = (k % 5).astype(np.int64)
        q = (k % 2).astype(np.int64)
        for which in (0, 1):
            want = _want(which, k, s, q, L)
            for mode in (0, 1, 2):
                assert np.array_equal(ix.debug_sort(k, s, q, which, mode), want), (n, which, mode)
    rng = np.random.default_rng(11)
    for n in (3, 17, 18, 40, 65, 130, 500, 1024):
        for spread in (1, 2, 5, 1 << 20):
            k = rng.integers(0, spread, size=n)
            s = rng.integers(0, min(spread, 4), size=n)
            q = rng.integers(0, 2, size=n)
            for which in (0, 1):
                a, b = ix.debug_sort(k, s, q, which, 3), ix.debug_sort(k, s, q, which, 4)
                assert np.array_equal(a, b), (n, spread, which)
                keys = k[a] if which == 0 else np.stack([-s[a], k[a], q[a]], 1)
                srt = np.all(np.diff(keys) >= 0) if which == 0 else all(tuple(keys[i]) <= tuple(keys[i + 1]) for i in range(n - 1))
                assert srt


def test_chain_filter_sort_depth_limit_fallback(ix):
    """The same two checks for which = 2 (the adversary turned for the descending order: weight = n - 1 - key, so that the
    sort makes the comparisons the adversary answered)."""
    L = loader.ref_chain_lib()
    for n in (200, 700, 1024):
        k, hit = _antiquicksort(n)
        assert hit, n
        w = n - 1 - k
        want = loader.flt_sort(w, L)
        for mode in (0, 1, 2):
            assert np.array_equal(ix.debug_sort(w, w, w, 2, mode), want), (n, mode)
    rng = np.random.default_rng(11)
    for n in (3, 17, 18, 40, 65, 130, 500, 1024):
        for spread in (1, 2, 5, 1 << 20):
            w = rng.integers(0, spread, size=n)
            a, b = ix.debug_sort(w, w, w, 2, 3), ix.debug_sort(w, w, w, 2, 4)
            assert np.array_equal(a, b), (n, spread)
            assert np.array_equal(np.sort(a), np.arange(n)) and np.all(np.diff(w[a]) <= 0), (n, spread)
