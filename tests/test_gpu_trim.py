"""bwams_fastq_trim, bwams_fastq_text and bwams_process_chunk_decoded on the device against bwams/trim.py: the fetched arrays of the
trimmed chunk, the report and the stats, all exact."""
import numpy as np
import pytest

from bwams import capi, simulate, trim

import trim_cases as tc
from bam_reads_util import many_records
from test_host_boundary import _setup

pytestmark = pytest.mark.gpu

ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"              # 33 letters


def _same_chunk(got: dict, reads):
    """a fetched chunk against a list of reads, array for array"""
    assert got["n"] == len(reads)
    assert got["names"] == [r[0] for r in reads] and got["comments"] == [r[1] for r in reads]
    cum = np.concatenate([[0], np.cumsum([len(r[2]) for r in reads])]).astype(np.int64)
    assert np.array_equal(got["cum"], cum)
    assert np.array_equal(got["enc"], np.concatenate([r[2] for r in reads]) if reads else np.zeros(0, np.uint8))
    if reads and reads[0][3] is not None:
        assert np.array_equal(got["quals"], np.concatenate([r[3] for r in reads]))
    else:
        assert got["quals"] is None or len(got["quals"]) == 0


def _check(fq: capi.Fastq, opt, paired: bool):
    """the device against the restatement on the reads of fq -> (report, stats)"""
    reads = trim.from_fetch(fq.fetch())
    kept, rep, st = trim.trim(reads, opt, paired)
    g, grep, gst = fq.trim(capi.trim_opt(opt), paired)
    try:
        for f in trim.READ_DTYPE.names:
            assert np.array_equal(grep[f], rep[f]), (f, np.nonzero((grep[f] != rep[f]).reshape(len(rep), -1).any(axis=1))[0][:8])
        assert gst == st
        assert bool(capi.lib().bwams_fastq_has_qual(g.h)) == bool(capi.lib().bwams_fastq_has_qual(fq.h))
        i = g.info()
        assert (i["n_reads"], i["n_bases"]) == (len(kept), sum(len(k[2]) for k in kept)) == (g.n_reads, g.n_bases)
        _same_chunk(g.fetch(), kept)
        _same_chunk(fq.fetch(), reads)                         # the input is left as it was
    finally:
        g.close()
    return rep, st


def _chunk_of(reads) -> capi.Fastq:
    return capi.Fastq(trim.to_fastq(reads))


CASES = tc.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_case(case):
    _, reads, opt, paired, want = case
    fq = _chunk_of(reads)
    rep, _ = _check(fq, opt, paired)
    fq.close()
    assert [(int(r["start"]), int(r["len"]), int(r["insert"]), int(r["reason"])) for r in rep] == want


LENS = [30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 151, 1024, 1025]


def _edge_pairs():
    """pairs with a planted insert at the limits of T3's geometry and mismatches at the word edges of the overlap -> (reads, the
    planted I per pair or 0 where the pair must not pass through T3)"""
    rng = np.random.default_rng(41)
    reads, planted = [], []
    combos = [(n, n) for n in LENS] + [(LENS[k], LENS[(k + 5) % len(LENS)]) for k in range(len(LENS))]
    for n1, n2 in combos:
        if max(n1, n2) > 1024:                                # skipped by T3: the adapters behind the insert are T4's to find
            I = min(n1, n2, 500) - 20
            a, b = tc.sim_pair(rng, I, n1, n2, err=0.0, adapters=(tc.ADAPTER, ADAPTER2))
            reads += [a, b]; planted.append(0)
            continue
        lo_n, hi_n = min(n1, n2), max(n1, n2)
        for I in sorted({30, lo_n - 1, lo_n, hi_n, hi_n + 1, n1 + n2 - 30}):
            if not 30 <= I <= n1 + n2 - 30:
                continue
            lo, hi = max(0, I - n2), min(n1, I)
            edges = [lo, hi - 1] + [p for m in range(64, hi, 64) for p in (m - 1, m) if lo < p < hi - 1]
            sets = [edges[k:k + 4] for k in range(0, len(edges), 4)]      # every edge: both sides of each multiple of 64 in the overlap
            for s in sets:
                s = sorted(set(s))[:min(4, (hi - lo) // 5)]          # within both limits: d <= 5 and 100 d <= 20 ov
                reads += tc.pair_of(rng, I, n1, n2, mism1=s); planted.append(I)
            reads += tc.pair_of(rng, I, n1, n2, mism1=sorted(set(edges))[:6] if len(set(edges)) >= 6 else range(lo, lo + 6))
            planted.append(-1)                                # six mismatches: I itself must not pass
    # 70 and 140 candidates in front of the hit; the hit in the last lane of the first round and in the first lane of the second
    for I in (200, 130, 270 - 63, 270 - 64):
        reads += tc.pair_of(rng, I, 150, 150, mism1=(I // 2,)); planted.append(I)
    return tc.named(reads, True), planted


def test_overlap_at_the_word_edges():
    reads, planted = _edge_pairs()
    fq = _chunk_of(reads)
    opt = trim.identity_opt(overlap=1, adapter1=tc.ADAPTER, adapter2=ADAPTER2)
    rep, st = _check(fq, opt, True)
    fq.close()
    ins = rep["insert"][0::2]
    n_skip = 0
    for k, I in enumerate(planted):
        if I > 0:
            assert ins[k] >= I, (k, I, ins[k])
        elif I == 0:                                                 # longer than the limit: counted, and T4 cut both ends at the adapters
            n_skip += 1
            assert rep["steps"][2 * k] == rep["steps"][2 * k + 1] == trim.STEP_SKIPPED | 1 << trim.S_ADAPTER
            assert rep["len"][2 * k] == rep["len"][2 * k + 1] and ins[k] == 0
    assert st["pairs_skipped"] == n_skip >= 3
    assert (ins[[k for k, I in enumerate(planted) if I > 0]] == [I for I in planted if I > 0]).mean() > 0.95


def _quality(rng, n):
    """good in the middle, a ragged front and tail"""
    q = rng.integers(25, 41, n)
    f, t = int(rng.integers(0, max(n // 3, 1) + 1)), int(rng.integers(0, max(n // 3, 1) + 1))
    q[:f] = rng.integers(2, 24, f)
    q[n - t:] = rng.integers(2, 24, t)
    return q


@pytest.mark.parametrize("window", [4, 64])
@pytest.mark.parametrize("adapter", [b"G", ADAPTER2, (ADAPTER2 * 4)[:128]], ids=["1", "33", "128"])
def test_quality_windows_and_adapters_by_length(window, adapter):
    rng = np.random.default_rng(len(adapter) * 100 + window)
    A = tc.codes(adapter)
    reads = []
    for n in (1, window - 1, window, 63, 64, 65, 129, 10001):
        for v in range(4):
            body = rng.integers(0, 4, n).astype(np.uint8)
            if len(adapter) == 1:
                body[body == 2] = 0                           # no G in front of the planted one
            p = int(rng.integers(0, n + 1)) if v < 3 else n - 4
            c = np.concatenate([body[:max(p, 0)], A, rng.integers(0, 4, n).astype(np.uint8)])[:n]
            if v == 2 and n > 8:
                c[min(p + 3, n - 1)] = 4                      # an N inside the adapter
            reads.append(tc.rd(c, _quality(rng, n) if v else np.full(n, 40)))
    q = np.full(10001, 2)                                     # the first passing window lies 78 chunks in, the last 31 from the end
    q[5000:8000] = 35
    reads.append(tc.rd(rng.integers(0, 4, 10001).astype(np.uint8), q))
    fq = _chunk_of(tc.named(reads))
    opt = trim.identity_opt(cut_front=1, cut_tail=1, cut_window=window, cut_quality=20, adapter1=adapter)
    rep, st = _check(fq, opt, False)
    fq.close()
    assert (int(rep["start"][-1]), int(rep["removed"][-1][trim.S_CUT_FRONT]), int(rep["removed"][-1][trim.S_CUT_TAIL])) == (5000, 5000, 2001)
    assert st["step_reads"][trim.S_ADAPTER] > 4 and st["step_reads"][trim.S_CUT_TAIL] > 4 and st["step_reads"][trim.S_CUT_FRONT] > 4


@pytest.fixture(scope="module")
def bulk_pairs():
    fq = _chunk_of(tc.bulk(7, 1500, True))
    yield fq
    fq.close()


@pytest.fixture(scope="module")
def bulk_single():
    fq = _chunk_of(tc.bulk(8, 1500, False))
    yield fq
    fq.close()


ALL_ON = dict(trim_front=1, trim_tail=1, cut_front=1, cut_tail=1, overlap=1, adapter1=tc.ADAPTER, adapter2=b"AGATCGGAAGAGCGTCGTGTAGG", max_len=140)


@pytest.mark.parametrize("which", ["default", "all_on"])
def test_bulk_pairs(bulk_pairs, which):
    opt = trim.Opt() if which == "default" else trim.Opt(**ALL_ON)
    rep, st = _check(bulk_pairs, opt, True)
    assert st["pairs_insert"] > 300 and st["dropped"][trim.LEN - 1] > 100 and st["dropped"][trim.MATE - 1] > 0 and st["reads_out"] > 1500
    assert st["step_reads"][trim.S_OVERLAP] > 100 and st["step_reads"][trim.S_CUT_TAIL] > 100
    if which == "all_on":
        assert all(x > 0 for k, x in enumerate(st["step_reads"]) if k != trim.S_CUT_FRONT)      # the fronts are good: test_quality_windows_* cuts them


@pytest.mark.parametrize("which", ["default", "all_on"])
def test_bulk_single(bulk_single, which):
    opt = trim.Opt() if which == "default" else trim.Opt(**ALL_ON)
    rep, st = _check(bulk_single, opt, False)
    assert st["pairs_insert"] == 0 and st["dropped"][trim.LEN - 1] > 50 and st["dropped"][trim.MATE - 1] == 0 and st["reads_out"] > 700
    if which == "all_on":
        assert st["step_reads"][trim.S_ADAPTER] > 100


def test_identity_and_nothing_left(bulk_pairs):
    rep, st = _check(bulk_pairs, trim.identity_opt(), True)
    assert st["reads_out"] == st["reads_in"] == 3000 and st["bases_out"] == st["bases_in"] and not rep["steps"].any()
    rep, st = _check(bulk_pairs, trim.Opt(min_len=10**6), True)
    assert st["reads_out"] == 0 and st["bases_out"] == 0 and st["dropped"][trim.LEN - 1] == 3000
    g, _, _ = bulk_pairs.trim(capi.trim_opt(min_len=10**6), True, report=False)
    assert g.fetch()["n"] == 0 and g.text() == b""
    g2, rep2, st2 = g.trim(None, True)                        # a chunk of no reads is a chunk
    assert st2["reads_in"] == 0 and len(rep2) == 0 and g2.fetch()["n"] == 0
    g.close(); g2.close()


def test_fasta_input():
    reads = [(r[0], r[1], r[2], None) for r in tc.bulk(9, 200, True)]
    fq = capi.Fastq(trim.to_fastq(reads))
    assert not capi.lib().bwams_fastq_has_qual(fq.h)
    rep, st = _check(fq, trim.Opt(**ALL_ON), True)
    fq.close()
    assert st["step_reads"][trim.S_CUT_FRONT] == st["step_reads"][trim.S_CUT_TAIL] == st["dropped"][trim.QUAL - 1] == 0
    assert st["pairs_insert"] > 30 and st["step_reads"][trim.S_FIXED] == 400


def test_input_decoded_from_bam_records():
    records, want = many_records(400, 5)
    fq = capi.bam_reads_decode(0, records, b"RGNM")
    assert fq.n_reads == len(want) and fq.n_reads % 2 == 0
    for paired in (False, True):
        rep, st = _check(fq, trim.Opt(adapter1=b"ACGT", adapter2=b"TTGCA", n_limit=20), paired)
        assert 0 < st["reads_out"] < st["reads_in"] and st["step_reads"][trim.S_ADAPTER] > 50
    fq.close()


@pytest.mark.parametrize("field,value", [("cut_window", 0), ("cut_window", 65), ("overlap_min", 0), ("adapter_min_match", 0),
                                         ("adapter_mismatch_per", 0), ("min_len", 0), ("trim_front", -1), ("n_limit", -1),
                                         ("adapter1", b"ACGN"), ("adapter2", b"acgt"), ("adapter1", b"A" * 129), ("paired", 1)])
def test_refusals(field, value):
    fq = _chunk_of(tc.named([tc.rd("ACGT")] * 3))
    o = capi.trim_opt()
    if field != "paired":
        if isinstance(value, bytes) and len(value) == 129:
            C = capi.C
            C.memmove(C.addressof(o) + getattr(capi.TrimOpt, field).offset, value, 129)      # no NUL within the field
        else:
            setattr(o, field, value)
    with pytest.raises(capi.BwamsError) as e:
        fq.trim(o, field == "paired")
    fq.close()
    assert e.value.code == -3 and f"bwams_fastq_trim: {field}:" in str(e.value)


@pytest.mark.parametrize("with_comment", [True, False])
def test_text_round_trip(bulk_single, with_comment):
    g, _, _ = bulk_single.trim(capi.trim_opt(), False, report=False)
    for fq in (bulk_single, g):
        d = fq.fetch()
        reads = trim.from_fetch(d)
        text = fq.text(with_comment)
        assert text == trim.to_fastq(reads, with_comment)
        addr, n = fq.text(with_comment, fetch=False)
        assert n == len(text) and addr
        back = capi.Fastq(addr, n_bytes=n)                    # decoded from the device text
        _same_chunk(back.fetch(), reads if with_comment else [(r[0], None) + r[2:] for r in reads])
        back.close()
    g.close()


def test_text_of_a_chunk_without_qualities():
    reads = [(r[0], r[1], r[2], None) for r in tc.bulk(10, 20, False)]
    fq = capi.Fastq(trim.to_fastq(reads))
    assert fq.text() == trim.to_fastq(reads) and fq.text().startswith(b">s0 c:0\n")
    fq.close()


def _primary_cigars(sam: bytes) -> dict:
    out = {}
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) > 5 and not int(f[1]) & 0x900:
            out[(f[0], int(f[1]) & 0xC0)] = f[5]
    return out


@pytest.mark.parametrize("mode", ["se", "pe"])
def test_trimmed_chunk_through_the_mapper(mode):
    g, ix, _, _ = _setup()
    rng = np.random.default_rng(31)
    paired = mode == "pe"
    reads = []
    for k in range(120 if paired else 200):
        I = int(rng.integers(60, 320))
        at = int(rng.integers(0, len(g) - 400))
        F = np.asarray(g[at:at + I], np.uint8)
        ends = []
        for e, src in enumerate((F, tc.rc(F))):
            x = np.concatenate([src, tc.codes((tc.ADAPTER, ADAPTER2)[e]), rng.integers(0, 4, 150).astype(np.uint8)])[:150].copy()
            err = rng.random(150) < 0.005
            x[err] = (x[err] + 1) % 4
            q = np.clip(39 - np.arange(150) // 12 + rng.integers(-3, 3, 150), 2, 41)
            q[150 - int(rng.integers(0, 12)):] = 4
            ends.append(tc.rd(x, q))
        reads += ends if paired else ends[:1]
    reads = tc.named(reads, paired, b"m")
    text = trim.to_fastq(reads)
    opt = trim.Opt(adapter1=tc.ADAPTER, adapter2=ADAPTER2)
    kept, _, st = trim.trim(reads, opt, paired)
    assert st["step_reads"][trim.S_ADAPTER if not paired else trim.S_OVERLAP] > 20
    b = capi.Batch(ix, len(reads), len(reads) * 160)
    raw, _ = b.process_chunk(text, paired=paired, n_processed=10)
    want, _ = b.process_chunk(trim.to_fastq(kept), paired=paired, n_processed=10)
    fq = capi.Fastq(text)
    t, _, gst = fq.trim(capi.trim_opt(opt), paired)
    fq.close()
    assert gst == st
    got, off = b.process_chunk_decoded(t, paired=paired, n_processed=10)
    assert not t.h and b._nseq == len(kept) == len(off) - 1
    assert got == want and got.count(b"\n") >= len(kept)
    a, c = _primary_cigars(raw), _primary_cigars(got)
    assert sum(1 for k in c if a[k] != c[k]) > 10             # the step reached the mapper
    # an odd chunk as paired-end is refused, and the chunk is consumed all the same
    odd = capi.Fastq(trim.to_fastq(reads[:3]))
    with pytest.raises(capi.BwamsError) as e:
        b.process_chunk_decoded(odd, paired=True)
    assert e.value.code == -3 and "bwams_process_chunk_decoded" in str(e.value) and not odd.h
    b.close(); ix.close()


def test_command_line_round_trip(tmp_path, capsys):
    """tools/fastq_trim.py through main(): interleaved pairs to BGZF in several deflater pieces, two files in and two out (one gz in,
    one gz out), single-end to plain text; the outputs and the stats of the whole run against the restatement, chunk sizes apart"""
    import gzip
    import importlib.util
    import json
    import os
    spec = importlib.util.spec_from_file_location("fastq_trim", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                            "tools", "fastq_trim.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    reads = [(r[0], None) + r[2:] for r in tc.bulk(12, 600, True)]
    recs = [trim.to_fastq([r]) for r in reads]
    p = lambda name: str(tmp_path / name)
    with open(p("il.fq"), "wb") as f:
        f.write(b"".join(recs))
    with gzip.open(p("r1.fq.gz"), "wb") as f:
        f.write(b"".join(recs[0::2]))
    with open(p("r2.fq"), "wb") as f:
        f.write(b"".join(recs[1::2]))
    ad = ["--adapter1", tc.ADAPTER.decode(), "--adapter2", ADAPTER2.decode(), "--cut-front", "1"]
    opt = trim.Opt(cut_front=1, adapter1=tc.ADAPTER, adapter2=ADAPTER2)

    def run(args):
        assert cli.main(args + ad) == 0
        return json.loads(capsys.readouterr().out)

    kept, _, want = trim.trim(reads, opt, True)
    cli.Out.PIECE = 70_000                                   # the text of a chunk goes through the deflater in several pieces
    try:
        st = run(["--interleaved", "--chunk-bases", "60000", "-o", p("o.fq.gz"), p("il.fq")])
    finally:
        cli.Out.PIECE = 32 << 20
    assert gzip.open(p("o.fq.gz")).read() == trim.to_fastq(kept) and st == want
    st = run(["--chunk-bases", "30000", "-o", p("o1.fq"), "-O", p("o2.fq.gz"), p("r1.fq.gz"), p("r2.fq")])
    assert open(p("o1.fq"), "rb").read() == trim.to_fastq(kept[0::2]) and gzip.open(p("o2.fq.gz")).read() == trim.to_fastq(kept[1::2])
    assert st == want
    kept1, _, want1 = trim.trim(reads[1::2], opt, False)
    st = run(["-o", p("s.fq"), p("r2.fq")])
    assert open(p("s.fq"), "rb").read() == trim.to_fastq(kept1) and st == want1 and 0 < want1["reads_out"] < want1["reads_in"]
