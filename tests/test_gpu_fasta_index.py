"""FASTA -> index on the GPU (bwams_index_from_fasta / _file, bwams_index_save's .ann / .amb / .pac, bwams_index_load_bns):
the reference's own bytes on the golden cases, the restatement (bwams/bns.py) on a 50 Mbp FASTA, the FM-index files equal to
bwams_index_build's on the restated codes, SAM from three handles byte-identical, and the refusals."""
import gzip
import os

import numpy as np
import pytest
import torch

from bwams import bns, capi, simulate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "bns_cases.npz"))
CASES = sorted({k.split("/")[0] for k in GOLDEN.files})


def _files(prefix, exts=("ann", "amb", "pac")):
    return {e: open(f"{prefix}.{e}", "rb").read() for e in exts}


def _check_golden(ix, case, tmp_path, tag):
    pre = str(tmp_path / f"{case}_{tag}")
    ix.save(pre)
    got = _files(pre)
    ix.close()
    for e in ("ann", "amb", "pac"):
        assert got[e] == bytes(GOLDEN[f"{case}/{e}"]), (case, tag, e)


def test_golden_cases_from_host_device_and_files(tmp_path):
    for case in CASES:
        text = bytes(GOLDEN[case + "/fa"])
        _check_golden(capi.Index.from_fasta(text), case, tmp_path, "host")
        dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        _check_golden(capi.Index.from_fasta(dev), case, tmp_path, "device")
        plain, gz = tmp_path / f"{case}.fa", tmp_path / f"{case}.fa.gz"
        plain.write_bytes(text)
        gz.write_bytes(gzip.compress(text))
        _check_golden(capi.Index.from_fasta_file(str(plain)), case, tmp_path, "file")
        _check_golden(capi.Index.from_fasta_file(str(gz)), case, tmp_path, "gz")


def test_handle_carries_the_contigs():
    t = b">chr1 first contig\nACGTNNNNacgtRYnnNNA\nCCGT\n>chr2\nNNNNGGGG\n"
    ix = capi.Index.from_fasta(t)
    st = ix.fasta_stats
    assert (st.l_pac, st.n_seqs, st.n_holes, st.n_ambig_bases) == (31, 2, 6, 14)
    ix.close()


def make_fasta(seed: int, n_contigs: int = 320, total: int = 52_000_000, n_total: int = 24_000_000) -> bytes:
    """Random FASTA: line widths 50-120 (some CRLF), N runs of 1 .. 10^5 (more than 2^24 N in all), 1 % IUPAC, lowercase runs."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 300, n_contigs).astype(np.float64)
    lens = np.maximum((lens / lens.sum() * total).astype(np.int64), 1000)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(lens.sum()))].copy()
    L = len(seq)
    iu = rng.random(L) < 0.01
    seq[iu] = np.frombuffer(b"RYKMSWBDHVN", np.uint8)[rng.integers(0, 11, int(iu.sum()))]
    for _ in range(2000):                                      # lowercase runs
        a = int(rng.integers(0, L)); seq[a:a + int(rng.integers(1, 5000))] |= 0x20
    placed = 0
    while placed < n_total:                                    # N runs, log-uniform lengths 1 .. 10^5
        k = int(np.exp(rng.uniform(0, np.log(1e5))))
        a = int(rng.integers(0, L - k))
        seq[a:a + k] = ord("n") if rng.random() < 0.1 else ord("N")
        placed += k
    out, at = [], 0
    for i, ln in enumerate(lens):
        w, crlf = int(rng.integers(50, 121)), i % 7 == 3
        s = seq[at:at + ln].tobytes()
        at += ln
        nl = b"\r\n" if crlf else b"\n"
        out.append(b">ctg%d %s%s" % (i, b"desc %d" % i if i % 3 else b"", nl) if i % 3 else b">ctg%d%s" % (i, nl))
        out.append(nl.join(s[j:j + w] for j in range(0, len(s), w)) + nl)
        if i % 11 == 5:
            out.append(nl)                                     # an empty line
    return b"".join(out)


@pytest.fixture(scope="module")
def big():
    text = make_fasta(7)
    want = bns.fasta2bntseq(text)
    assert want["l_pac"] >= 50_000_000 and len(want["names"]) >= 300 and want["n_ambig"] > (1 << 24)
    return text, want


def _fastq(reads, tag):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i // 2 if tag == b"p" else i, bytes(b"ACGTN"[x] for x in r), b"I" * len(r))
                    for i, r in enumerate(reads))


def _sam(ix, se, pe, n_reads, n_bases):
    b = capi.Batch(ix, n_reads, n_bases)
    s1, _ = b.process_chunk(se)
    s2, _ = b.process_chunk(pe, paired=True)
    b.close()
    return s1, s2


def test_at_scale_and_end_to_end(big, tmp_path):
    text, want = big
    a = capi.Index.from_fasta(text)
    st = a.fasta_stats
    assert st.l_pac == want["l_pac"] and st.n_ambig_bases == want["n_ambig"] and st.n_holes == len(want["holes"][0])
    pa = str(tmp_path / "a")
    a.save(pa)
    got = _files(pa, ("ann", "amb", "pac", "bwt.2bit.64", "0123"))
    for e in ("ann", "amb", "pac"):
        assert got[e] == want[e], e
    c = capi.Index.build(want["codes"])
    pc = str(tmp_path / "c")
    c.save(pc)
    wfm = _files(pc, ("bwt.2bit.64", "0123"))
    assert got["bwt.2bit.64"] == wfm["bwt.2bit.64"] and got["0123"] == wfm["0123"]

    # end to end: reads simulated from the codes, single-end and paired-end
    g = want["codes"]
    reads, _, _ = simulate.make_reads(g, 600, seed=5)
    pairs = simulate.make_read_pairs(g, 300, seed=6)
    se, pe = _fastq(reads, b"r"), _fastq(pairs, b"p")
    nr, nb = 1200, 1200 * 160
    names, annos = want["names"], bns.restored_annos(want["comments"])
    ctg = np.zeros(len(names), capi.CONTIG_DTYPE)
    ctg["offset"], ctg["len"] = want["offsets"], want["lens"]
    c.set_contigs(ctg); c.set_contig_names(names); c.set_contig_annos(annos)
    sam_a, sam_c = _sam(a, se, pe, nr, nb), _sam(c, se, pe, nr, nb)
    assert sam_a == sam_c and sam_a[0].count(b"\n") >= 600
    # (b) open + load_bns, with a .alt naming two contigs; (c) with the same alt flags by hand
    with open(pa + ".alt", "w") as f:
        f.write("@SQ\tSN:x\n%s\t0\t*\n%s\t16\t*\n" % (names[5].decode(), names[17].decode()))
    b_ = capi.Index.open(pa)
    b_.load_bns(pa)
    ctg["is_alt"][[5, 17]] = 1
    c.set_contigs(ctg); c.set_contig_names(names); c.set_contig_annos(annos)
    assert _sam(b_, se, pe, nr, nb) == _sam(c, se, pe, nr, nb)
    for ix in (a, b_, c):
        ix.close()


def test_refusals(tmp_path):
    with pytest.raises(capi.BwamsError) as e:
        capi.Index.from_fasta(b">r\nACGT\n+\nIIII\n")
    assert e.value.code == -6                                  # BWAMS_ERR_UNSUPPORTED
    with pytest.raises(capi.BwamsError) as e:
        capi.Index.from_fasta(b"ACGT\nACGT\n")
    assert e.value.code == -3                                  # BWAMS_ERR_ARG
    ix = capi.Index.from_fasta(b">a\nACGTACGTAA\n>b\nCCGTN\n")
    pre = str(tmp_path / "m")
    ix.save(pre)
    ix.close()
    amb = open(pre + ".amb").read().split("\n")
    amb[0] = "15 3 1"
    open(pre + ".amb", "w").write("\n".join(amb))
    o = capi.Index.open(pre)
    with pytest.raises(capi.BwamsError) as e:
        o.load_bns(pre)
    assert e.value.code == -2                                  # BWAMS_ERR_IO: inconsistent .ann and .amb
    o.close()
