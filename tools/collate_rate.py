"""A coordinate-sorted BAM collated by read name on one MI355X (bwams_collate_t): what the adds cost per million records, how that
splits over the kernels, and what the copies move per second.

--records (default 10^6) mapped paired records of 150M, all of one size (276 bytes, tools/bam_query_rate.py's layout), in
coordinate order on one reference of --ref-mb (default 100): the first of each pair at a random place, its mate 200 to 500 bases
behind it, and for --far (default 0.02) of the pairs anywhere on the reference.  The records lie in host memory and go through
bwams_collate_add_records in pieces of --piece-records (default 100000), then bwams_collate_finish.  Warm, --reps times:
  add_ms      host clock around all adds and the finish of a round: the host's chain walk and the upload of every piece included
  kernels_ms  device time between events from bwams_collate_info: entry (entry kernel, scan, append), group (the sort), match, place
              (placement and its three scans), copy (pairs, singles, pool)
  copy_GB_per_s  the bytes the three copies wrote (pairs, singles, pooled and compacted) over kernels_ms.copy
The first piece's output is compared with bwams/collate.py.  --once runs one unmeasured round and stops: the run to put under a
kernel trace.  One JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bwams import capi, collate  # noqa: E402
from bam_query_rate import records_150m, stats  # noqa: E402


def sorted_pairs(n_records: int, l_ref: int, far: float, seed: int) -> np.ndarray:
    """n_records / 2 pairs as uint8[n_records, 276] in coordinate order (stable)"""
    rng = np.random.default_rng(seed)
    n_pairs = n_records // 2
    pos1 = rng.integers(0, l_ref - 1000, n_pairs)
    pos2 = np.where(rng.random(n_pairs) < far, rng.integers(0, l_ref - 150, n_pairs), pos1 + rng.integers(200, 501, n_pairs))
    pos = np.concatenate([pos1, pos2])
    pair = np.concatenate([np.arange(n_pairs), np.arange(n_pairs)])
    flag = np.concatenate([np.full(n_pairs, 0x1 | 0x2 | 0x20 | 0x40), np.full(n_pairs, 0x1 | 0x2 | 0x10 | 0x80)]).astype("<u2")
    order = np.argsort(pos, kind="stable")
    pos, pair, flag = pos[order], pair[order], flag[order]
    rec = np.frombuffer(records_150m(np.zeros(len(pos), np.int64), pos, 0, rng), np.uint8).reshape(len(pos), 276).copy()
    rec[:, 36:46] = (pair[:, None] // 10 ** np.arange(9, -1, -1)) % 10 + 48
    rec[:, 18:20] = flag.view(np.uint8).reshape(len(pos), 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ref-mb", type=float, default=100.0)
    ap.add_argument("--far", type=float, default=0.02)
    ap.add_argument("--piece-records", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    rec = sorted_pairs(a.records, int(a.ref_mb * 1e6), a.far, 7)
    pieces = [rec[k:k + a.piece_records].tobytes() for k in range(0, len(rec), a.piece_records)]
    c = capi.Collate()

    def round_of():
        c.reset()
        t = time.perf_counter()
        peak = room = 0
        for p in pieces:
            c.add_records(p)
            i = c.info()
            peak = max(peak, i["pending"])
            room = max(room, i["pool_capacity"])
        n_orphans = c.finish()
        return (time.perf_counter() - t) * 1e3, c.info(), n_orphans, (peak, room)

    c.add_records(pieces[0])                                 # the first piece against the restatement
    want_pairs, want_singles = collate.Collate().add(pieces[0])
    got = c.fetch()
    assert got[0] == collate.pairs_bytes(want_pairs) and got[2] == b"".join(want_singles)
    _, info, n_orphans, peak = round_of()                    # warm-up
    assert 2 * info["pairs"] + n_orphans == len(rec) and info["bytes_compacted"] <= info["bytes_pooled"]
    if a.once:
        return
    ms, kernels = [], {k: [] for k in ("ms_entry", "ms_group", "ms_match", "ms_place", "ms_copy")}
    for _ in range(a.reps):
        t, info, n_orphans, peak = round_of()
        ms.append(t)
        for k in kernels:
            kernels[k].append(info[k])
    per_m = 1e6 / len(rec)
    copied = 276 * (2 * info["pairs"] + info["singles"]) + info["bytes_pooled"] + info["bytes_compacted"]
    k_med = {k[3:]: round(float(np.median(v)), 3) for k, v in kernels.items()}
    print(json.dumps({"collate": True, "records": len(rec), "record_bytes": 276, "pieces": len(pieces), "pairs": info["pairs"],
                      "orphans": n_orphans, "peak_pending": peak[0], "peak_pool_capacity": peak[1], "max_run": info["max_run"], "compactions": info["compactions"],
                      "bytes_pooled": info["bytes_pooled"], "bytes_compacted": info["bytes_compacted"],
                      "add_ms": stats(ms), "add_ms_per_million": round(float(np.median(ms)) * per_m, 2), "kernels_ms": k_med,
                      "kernels_ms_per_million": round(sum(k_med.values()) * per_m, 3),
                      "copy_GB_per_s": round(copied / max(k_med["copy"], 1e-6) / 1e6, 1)}), flush=True)
    c.close()


if __name__ == "__main__":
    main()
