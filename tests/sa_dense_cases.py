"""Toy indexes for the dense suffix-array table (csrc/fmi_sal.hip) and, from the oracle alone, what its entries must hold.

A case is a seeded random genome of L bases, i.e. an index of 2 L + 1 rows:

  L = 31     63 rows: fewer than a wavefront, and neither a multiple of 2 nor of 4
  L = 100    201 rows: rows whose walk meets the sentinel row
  L = 1000   2001 rows: a 40-base motif planted 12 times, so that its SMEMs have s = 12 occurrences (24 with the other strand);
             with max_occ = 3 the lookup takes the rows k + i * (s / max_occ), which are no multiples of the stride
  L = 2051   4103 rows: more than 4096

The seeds are chosen so that the properties tests/test_sa_dense_cases.py asserts hold; that test says so when one does not.
"""
from __future__ import annotations

import functools

import numpy as np

from bwams import fmindex
from oracle import loader

SIZES = (31, 100, 1000, 2051)
SEEDS = {31: 7, 100: 7, 1000: 24, 2051: 14}            # 1000: a walk of 69 steps; 2051: one of 76, and 24 sentinel walks with steps
MOTIF_LEN, MOTIF_COPIES = 40, 12
COORD_BITS, STEP_SHIFT = 40, 41
SENTINEL = np.uint64(1 << COORD_BITS)


def motif() -> np.ndarray:
    return np.random.default_rng(1234).integers(0, 4, MOTIF_LEN).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(L: int):
    """(genome, FMIndex) of the case with L bases"""
    rng = np.random.default_rng(SEEDS[L])
    g = rng.integers(0, 4, L).astype(np.uint8)
    if L == 1000:
        m = motif()
        for c in range(MOTIF_COPIES):                   # every 80 bases: the copies do not touch
            at = 20 + c * 80
            g[at:at + MOTIF_LEN] = m
    return g, fmindex.build_fmindex(g)


@functools.lru_cache(maxsize=None)
def walks(L: int):
    """For every row r of the case: (coordinate, LF steps, met the sentinel) of the reference's walk from r, each from the oracle's
    lookup of the single-row record k = r, s = 1.  A walk yields 0 either at the sentinel row or at a sample that holds 0 with no
    step taken (r % 8 == 0): only the second is no sentinel walk."""
    g, idx = case(L)
    o = loader.OracleFMI(idx)
    rows = int(idx.ref_seq_len)
    sm = np.zeros(rows, loader.SMEM_DTYPE)
    sm["k"] = np.arange(rows)
    sm["s"] = 1
    sm["l"] = 0
    coord = np.zeros(rows, np.int64)
    steps = np.zeros(rows, np.int64)
    for r in range(rows):
        ctr = loader.Counters()
        c, off = o.sa_lookup(sm[r:r + 1], 500, counters=ctr)
        assert len(c) == 1 and ctr.n_sa_lookups == 1
        coord[r], steps[r] = c[0], ctr.n_lf_steps
    sentinel = (coord == 0) & (np.arange(rows) % 8 != 0)
    coord.setflags(write=False); steps.setflags(write=False); sentinel.setflags(write=False)
    return coord, steps, sentinel


def expected_table(L: int, stride: int) -> np.ndarray:
    """the table's entries as bwams.h lays them out: coordinate | sentinel << 40 | steps << 41, one per stride-th row"""
    coord, steps, sentinel = walks(L)
    r = np.arange(0, len(coord), stride)
    low = np.where(sentinel[r], SENTINEL, coord[r].astype(np.uint64))
    return low | (steps[r].astype(np.uint64) << np.uint64(STEP_SHIFT))


@functools.lru_cache(maxsize=None)
def reads(L: int, n: int = 300):
    """(enc, cum) of reads drawn from the case's genome, both strands, a few mismatches, plus reads that are the motif and the
    motif with flanks; the read length is at most the genome's"""
    g, _ = case(L)
    rng = np.random.default_rng(100 + L)
    rl = min(60, L)
    out = []
    for _ in range(n):
        at = int(rng.integers(0, L - rl + 1))
        r = g[at:at + rl].copy()
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):
            r[int(rng.integers(0, rl))] = rng.integers(0, 4)
        out.append(r)
    m = motif()
    out += [m.copy(), (3 - m[::-1]).astype(np.uint8), np.concatenate([rng.integers(0, 4, 10).astype(np.uint8), m, rng.integers(0, 4, 10).astype(np.uint8)])]
    enc = np.concatenate(out)
    cum = np.concatenate([[0], np.cumsum([len(r) for r in out])]).astype(np.int64)
    return enc, cum


@functools.lru_cache(maxsize=None)
def oracle_seeds(L: int, max_occ: int, min_seed_len: int = 19):
    """(smems, coord, off, Counters) of reads(L) under the oracle; min_seed_len comes down for the 31-base genome"""
    _, idx = case(L)
    enc, cum = reads(L)
    o = loader.OracleFMI(idx)
    opt = loader.default_seed_opt()
    opt.max_occ = max_occ
    opt.min_seed_len = min(min_seed_len, 12) if L < 60 else min_seed_len
    ctr = loader.Counters()
    sm = o.collect_smem(enc, cum, opt, counters=ctr)
    coord, off = o.sa_lookup(sm, max_occ, counters=ctr)
    return sm, coord, off, ctr, opt
