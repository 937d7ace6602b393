"""FASTA -> index on the GPU at GRCh38 size: host read / inflate, device pack (with the text's GB/s against the 8 TB/s HBM peak),
FM-index build and total, from a synthetic FASTA (3.1 Gbp by default: 60-column lines, ~195 large contigs + ~3000 small ones,
~800 N runs totalling ~1.5e8 bases).  One JSON line on stdout.

    python tools/fasta_index_lab.py [--gbp 3.1] [--out results.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bwa-mem-scale_amd"))
from bwams import capi  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E, spec


def synth_fasta(total: int, seed: int = 38) -> bytes:
    rng = np.random.default_rng(seed)
    big = rng.lognormal(0, 0.6, 195); big = big / big.sum() * total * 0.97
    small = rng.integers(2_000, 20_000, 3000).astype(np.float64); small = small / small.sum() * total * 0.03
    lens = np.maximum(np.concatenate([big, small]).astype(np.int64), 100)
    L = int(lens.sum())
    seq = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, L, dtype=np.uint8)]
    n_runs = 800
    run_len = rng.integers(1, max(2, min(375_000, L // 4000)), n_runs)   # ~1.5e8 N in all at 3.1 Gbp
    starts = rng.integers(0, L - int(run_len.max()), n_runs)
    for a, k in zip(starts, run_len):
        seq[a:a + k] = ord("N")
    parts, at = [], 0
    for i, ln in enumerate(lens):
        s = seq[at:at + ln]; at += ln
        rows = (ln + 59) // 60
        m = np.full((rows, 61), ord("\n"), np.uint8)
        pad = np.zeros(rows * 60, np.uint8)
        pad[:ln] = s
        m[:, :60] = pad.reshape(rows, 60)
        body = m.reshape(-1)
        keep = np.ones(rows * 61, bool)
        if ln % 60:                                            # the last line's padding
            keep[(rows - 1) * 61 + ln % 60:rows * 61 - 1] = False
        parts.append(b">chr%d synthetic\n" % i)
        parts.append(body[keep].tobytes())
    return b"".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=3.1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    capi.build()
    t0 = time.time()
    text = synth_fasta(int(a.gbp * 1e9))
    gen_s = time.time() - t0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ref.fa")
        with open(path, "wb") as f:
            f.write(text)
        n_bytes = len(text)
        del text
        t1 = time.time()
        ix = capi.Index.from_fasta_file(path, keep_ref=True)
        wall = time.time() - t1
        st = ix.fasta_stats
        ix.close()
    pack_gbs = n_bytes / (st.ms_device_pack * 1e-3) / 1e9 if st.ms_device_pack > 0 else 0.0
    res = dict(text_bytes=n_bytes, l_pac=st.l_pac, n_seqs=st.n_seqs, n_holes=st.n_holes, n_ambig_bases=st.n_ambig_bases,
               ms_host_read=round(st.ms_host_read, 1), ms_upload=round(st.ms_upload, 1), ms_device_pack=round(st.ms_device_pack, 1),
               pack_text_gbs=round(pack_gbs, 1), pack_frac_of_hbm_peak=round(pack_gbs / HBM_PEAK_GBS, 4),
               ms_fm_build=round(st.ms_fm_build, 1), ms_total_wall=round(wall * 1e3, 1), gen_s=round(gen_s, 1))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
