"""One batch for the launch plan of the chaining stage (launch_chain_t, csrc/chain_wave.h): every launch of the plan has a read
to chain at the same time, so that every lane and both fork-join rounds carry work.  Built from the planted-seed blocks of
tests/chain_cases.py and tests/chain_lane_cases.py, default options; tests/test_chain_plan_cases.py proves under the oracle alone
that the batch holds what this text says, tests/test_gpu_chain_plan.py runs it through bwams_chain_run_ert.

  * a read at the lower and the upper seed-count limit of every wave class — 33 and 128 (S), 129 and 256 (M1), 257 and 512 (M),
    513 and 665 (M2), 666 and 850 (L1), 851 and 1275 (L2), 1276 and 1700 (L), 1701 and 4096 (XL) — and one of 4097 (XL2);
  * forty lane-tier reads of 0 .. 32 seeds, reads without a seed among them (no MEM at all, and a MEM without a hit), and one
    that needs a tenth chain (chain_lane_cases.leaf_full's "ten_of_10");
  * a read of 41 seeds that holds a chain position twice (chain_cases.settling's "equal_in_pass": chained again by
    chain_redo_kernel);
  * a lane-tier read of 17 chains and a redo read of 65 (chain_cases.filter_limits' "lane17" and "redo65"): more than
    kLightChains, so they — and the 41 chains of "equal_in_pass" — go through chain_heavy_kernel, in its classes of 64 and of
    128 chains.

plan_batch() returns the case and, per read's note, the seeds planted in it."""
import functools

import numpy as np

import chain_cases as cc
import chain_lane_cases as lc

WAVE_LIMITS = (33, 128, 129, 256, 257, 512, 513, 665, 666, 850, 851, 1275, 1276, 1700, 1701, 4096, 4097)
N_LANE = 40


@functools.lru_cache(maxsize=None)
def plan_batch():
    """(the case, {note: seeds planted})."""
    rng = np.random.default_rng(77)
    base = cc.grid(480, room=480)
    reads, notes, planted = [], [], {}

    def add(note, mems, n_seeds):
        reads.append(mems)
        notes.append(note)
        planted[note] = n_seeds

    lane_reads, lane_notes = lc._mixed_reads(N_LANE, rng)
    lane_seeds = [sum(len(m[2]) for m in rd) for rd in lane_reads]
    for i, n in enumerate(WAVE_LIMITS):
        sel = rng.permutation(base)[:min(n, 500)]
        add("seeds%d" % n, cc.ladder(sel, n, how="fb"[i % 2], order=("rand", "asc", "desc")[i % 3], rng=rng), n)
        # the lane tier's reads between the wave classes', as a chunk of real reads has them
        for j in range(i * N_LANE // len(WAVE_LIMITS), (i + 1) * N_LANE // len(WAVE_LIMITS)):
            add("lane_" + lane_notes[j], lane_reads[j], lane_seeds[j])
    leaf, settle, flt = lc.leaf_full(), cc.settling(), cc.filter_limits()
    add("ten_of_10", leaf.reads[leaf.read("ten_of_10")], 10)
    add("equal_in_pass", settle.reads[settle.read("equal_in_pass")], 41)
    add("lane17", flt.reads[flt.read("lane17")], 17)
    add("redo65", flt.reads[flt.read("redo65")], 65)
    return cc.Case("chain_plan", reads, notes), planted


def planted_class_counts(planted):
    """The ten class counts of chain_count_kernel (reads with more seeds than each limit, in cc.CLASS_ORDER's order) from the
    planted seed counts alone."""
    n = np.array(list(planted.values()), np.int64)
    return {cc.COUNT_KEYS[i]: int((n > t).sum()) for i, t in enumerate(cc.CLASS_ORDER)}
