"""The validity graph of a batch's products (csrc/stage_valid.h): replacing a product outdates what was computed from it, and a call
that reads an outdated product is refused (BWAMS_ERR_ARG, the entry point's own "run ... first" text) before it launches anything.
Everything through capi on a genome of 3000 bases: chunk A, 6 reads of 60 to 100 bases (as a paired-end chunk: three pairs), and
chunk B, 2 reads of 40 bases, smaller and shorter, so that a coordinate kept from A would lie outside B."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bwams import capi, simulate

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = simulate.make_genome(3000, seed=3, repeat_frac=0.0)
EMF_L = 40                                                      # reads of A that match the genome exactly are resolved by the filter

# the header's direct edges, restated: producer -> what is computed directly from it
EDGES = [("reads", "names"), ("reads", "seeds"), ("reads", "probe"), ("reads", "chains"), ("reads", "er"),
         ("seeds", "chains"), ("probe", "er"),
         ("chains", "built"), ("built", "ext"), ("ext", "dedup"), ("dedup", "pair"),
         ("dedup", "al"), ("pair", "al"),
         ("al", "sam"), ("names", "sam"), ("er", "sam"),
         ("sam", "bam"), ("bam", "sorted"), ("bam", "templates"), ("templates", "template_locs")]
# one order in which every product can be made (built stands apart: bwams_extend_run plans its own tasks and outdates the flat lists)
ORDER = ["reads", "names", "probe", "er", "seeds", "chains", "ext", "dedup", "pair", "al", "sam", "bam", "sorted", "templates",
         "template_locs"]


def _derived(p):
    out, grew = set(), True
    while grew:
        grew = False
        for a, b in EDGES:
            if (a == p or a in out) and b not in out:
                out.add(b)
                grew = True
    return out


def _ancestors(d):
    return {p for p, _ in EDGES if d in _derived(p)}


def _chunk(lens, seed, exact):
    """reads cut from the genome (every other one reverse-complemented); those not in `exact` get one mismatch"""
    rng = np.random.default_rng(seed)
    reads = []
    for i, ln in enumerate(lens):
        st = int(rng.integers(0, len(GENOME) - ln))
        rd = GENOME[st:st + ln].copy()
        if i not in exact:
            rd[ln // 2] ^= 1
        reads.append(simulate.revcomp(rd) if i % 2 else rd)
    enc, cum = simulate.flatten_reads(reads)
    return {"enc": enc, "cum": cum, "n": len(lens), "quals": np.full(len(enc), ord("F"), np.uint8)}


A = _chunk([60, 100, 73, 88, 95, 67], 11, exact={0, 3, 4})
B = _chunk([40, 40], 12, exact={0})


def _pair_chunk(lens, seed):
    """ends of pair p at 2p, 2p + 1: the second end reverse-complemented, about 150 bases downstream"""
    rng = np.random.default_rng(seed)
    reads = []
    for p in range(len(lens) // 2):
        l0, l1 = lens[2 * p], lens[2 * p + 1]
        st = int(rng.integers(0, len(GENOME) - 150 - l1))
        reads += [GENOME[st:st + l0].copy(), simulate.revcomp(GENOME[st + 150:st + 150 + l1])]
    enc, cum = simulate.flatten_reads(reads)
    return {"enc": enc, "cum": cum, "n": len(lens), "quals": np.full(len(enc), ord("F"), np.uint8)}


PA = _pair_chunk([60, 100, 73, 88, 95, 67], 21)
PB = _pair_chunk([40, 40], 22)
PES0 = np.zeros(4, capi.PESTAT_DTYPE)
PES0["failed"] = [1, 0, 1, 1]
PES0["low"][1], PES0["high"][1], PES0["avg"][1], PES0["std"][1] = 1, 600, 200.0, 50.0


@pytest.fixture(scope="module")
def index():
    ix = capi.Index.build(GENOME, 0)
    ix.set_contig_names([b"chr1"])
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def emf(index):
    e = capi.Emf.build(index, seed_len=EMF_L, slack=1.1)
    yield e
    e.close()


def _last_error():
    return capi.lib().bwams_last_error().decode()


def _refused(rc, text=None):
    assert rc == ERR_ARG
    if text is not None:
        assert _last_error() == text


class Pipe:
    """A batch and, per product, the call that makes it from a chunk (make), the bytes it holds (fetch) and a raw call that reads it
    with the text of its refusal (reader).  Single-end behind the exact-match filter, so that every product of the graph exists."""

    def __init__(self, index, emf):
        self.b = capi.Batch(index, 8, 1000)
        self.e = emf
        self.opt = capi.default_mem_opt()
        self.sopt = capi.default_sam_opt()
        self.c = None
        b, L, o = self.b, capi.lib(), C.byref(self.opt)
        self.make = {
            "reads": lambda: b.seed_upload(self.c["enc"], self.c["cum"]),
            "names": lambda: b.sam_upload([b"q%d" % i for i in range(self.c["n"])], self.c["quals"]),
            "probe": lambda: b.emf_run(self.e),
            "er": self._er_run,
            "seeds": lambda: b.seed_run(with_sa=True),
            "chains": lambda: b.chain_run(self.opt),
            "built": lambda: b.extend_build(self.opt),
            "ext": lambda: b.extend_run(self.opt),
            "dedup": lambda: b.dedup_run(self.opt),
            "pair": lambda: b.mark_primary_se(self.opt, id_base=0),
            "al": lambda: b.reg2aln(self.opt, 1),
            "sam": lambda: b.sam_run_emf(self.e, self.opt, self.sopt),
            "bam": b.bam_run,
            "sorted": b.bam_sort,
            "templates": b.bam_templates,
            "template_locs": b.bam_templates2,
        }
        arrs = lambda t: b"".join(np.ascontiguousarray(x).tobytes() for x in t)    # noqa: E731
        self.fetch = {
            "names": lambda: b"",                                                  # (seen through the text only)
            "probe": lambda: arrs(b.emf_fetch(self.c["n"])),
            "er": lambda: arrs(self._er_fetch()),
            "seeds": lambda: arrs(b.seed_fetch()),
            "chains": lambda: arrs(self._chains_fetch()),
            "built": lambda: arrs(b.extend_tasks_fetch(0)) + arrs(b.extend_tasks_fetch(1)),
            "ext": lambda: arrs(b.extend_fetch()),
            "dedup": lambda: arrs(b.dedup_fetch()),
            "pair": lambda: arrs(b.pair_fetch()),
            "al": lambda: arrs(self._al_fetch()),
            "sam": lambda: b.sam_fetch()[0],
            "bam": lambda: b.bam_fetch()[0],
            "sorted": lambda: b.bam_sorted_fetch()[0],
            "templates": lambda: arrs(b.bam_templates_fetch()),
            "template_locs": lambda: arrs([b.bam_templates_fetch_loc()]),
        }
        n, h = C.c_int64(0), b.h
        # product: (a raw call that reads it and nothing else that could be missing, bwams_last_error of its refusal)
        self.reader = {
            "names": (lambda: L.bwams_sam_run_emf(h, o, C.byref(self.sopt), self.e.h, C.byref(n)),
                      "bwams_sam_run: run bwams_sam_upload for this chunk first"),
            "probe": (lambda: L.bwams_emf_regs_run(h, self.e.h, o, C.byref(n)), "bwams_emf_regs_run: run bwams_emf_run first"),
            "er": (lambda: L.bwams_emf_regs_fetch(h, None, 0, None, None), "bwams_emf_regs_fetch: run bwams_emf_regs_run first"),
            "seeds": (lambda: L.bwams_chain_run(h, o, None, None), "bwams_chain_run: run bwams_seed_run(with_sa = 1) first"),
            "chains": (lambda: L.bwams_extend_run(h, o, None), "bwams_extend_run: run bwams_chain_run (or bwams_chain_upload) first"),
            "built": (lambda: L.bwams_extend_tasks_fetch(h, 0, None, 0, None, 0, None, 0, None, None, None),
                      "bwams_extend_tasks_fetch: no task lists on the device"),
            "ext": (lambda: L.bwams_dedup_run(h, o, None), "bwams_dedup_run: run bwams_extend_run first"),
            "dedup": (lambda: L.bwams_dedup_fetch(h, None, 0, None), "bwams_dedup_fetch: run bwams_dedup_run first"),
            "pair": (lambda: L.bwams_pair_fetch(h, None, 0, None, None), "bwams_pair_fetch: run bwams_pair_run first"),
            "al": (lambda: L.bwams_reg2aln_fetch(h, None, 0, None, 0, None, 0), "bwams_reg2aln_fetch: run bwams_reg2aln_run first"),
            "sam": (lambda: L.bwams_sam_fetch(h, None, 0, None, None, 0), "bwams_sam_fetch: run bwams_sam_run first"),
            "bam": (lambda: L.bwams_bam_fetch(h, None, 0, None), "bwams_bam_fetch: run bwams_bam_run first"),
            "sorted": (lambda: L.bwams_bam_sorted_fetch(h, None, 0, None), "bwams_bam_sorted_fetch: run bwams_bam_sort first"),
            "templates": (lambda: L.bwams_bam_templates_fetch(h, None, 0, None, 0),
                          "bwams_bam_templates_fetch: run bwams_bam_templates (and bwams_bam_sort for sorted = 1) on the current records first"),
            "template_locs": (lambda: L.bwams_bam_templates_fetch_loc(h, None, 0),
                              "bwams_bam_templates_fetch_loc: run bwams_bam_templates2 on the current records first"),
        }

    def _er_run(self):
        n = C.c_int64(0)
        capi._chk(capi.lib().bwams_emf_regs_run(self.b.h, self.e.h, C.byref(self.opt), C.byref(n)), "bwams_emf_regs_run")
        self.n_er = n.value

    def _er_fetch(self):
        regs, off, rev = np.zeros(max(self.n_er, 1), capi.ALNREG_DTYPE), np.zeros(self.c["n"] + 1, np.int64), np.zeros(self.c["n"], np.uint8)
        capi._chk(capi.lib().bwams_emf_regs_fetch(self.b.h, capi._p(regs), len(regs), capi._p(off), capi._p(rev)), "bwams_emf_regs_fetch")
        return regs[:self.n_er], off, rev

    def _chains_fetch(self):
        """the chains as chaining leaves them: the extension writes its marks (done, aln) into the chain seeds where they lie"""
        chains, seeds, off = self.b.chain_fetch()
        return [chains, off] + [seeds[f] for f in ("rbeg", "qbeg", "len", "score")]

    def replace_templates(self):
        """new templates of the same records: bwams_bam_templates keeps what it has, a rewrite of the qualities makes it start over"""
        import test_recal_model as M
        m = capi.RecalModel(M.zero_tables(0, 128), 128)
        a = capi.RecalApply(m, None, 0)
        m.close()
        a.batch(self.b)
        a.close()
        self.b.bam_templates()

    def _al_fetch(self):
        b, n = self.b, self.b._n_pair_regs
        aln, cig, md = np.zeros(max(n, 1), capi.ALN_DTYPE), np.zeros(4096, np.uint32), np.zeros(4096, np.uint8)
        capi._chk(capi.lib().bwams_reg2aln_fetch(b.h, capi._p(aln), len(aln), capi._p(cig), len(cig), capi._p(md), len(md)), "bwams_reg2aln_fetch")
        return aln[:n], cig, md

    def run(self, chunk, upto=None, only=None):
        """the products of ORDER (those in `only`) made in order for `chunk`, through `upto`"""
        self.c = chunk
        for p in ORDER:
            if only is None or p in only:
                self.make[p]()
            if p == upto:
                break

    def close(self):
        self.b.close()


@pytest.fixture(scope="module")
def want(index, emf):
    """what every product of chunk A and of chunk B holds after one run in order, on a batch nothing else touched"""
    out = {}
    for key, chunk in (("A", A), ("B", B)):
        p = Pipe(index, emf)
        p.run(chunk, upto="chains")
        p.make["built"]()
        built = p.fetch["built"]()
        p.run(chunk)
        out[key] = {d: p.fetch[d]() for d in ORDER[1:]}
        out[key]["built"] = built
        p.close()
    assert out["A"]["sam"].count(b"\n") >= A["n"] and out["B"]["sam"].count(b"\n") >= B["n"] and out["A"]["er"] != out["B"]["er"]
    return out


def test_edges_are_the_headers():
    """the Python copy of the edge list is the header's table, edge for edge"""
    text = open(os.path.join(ROOT, "bwa-mem-scale_amd", "csrc", "stage_valid.h")).read()
    table = re.search(r"constexpr Edge kEdges\[\] = \{(.*?)\n\};", text, re.S).group(1)
    got = re.findall(r"\{Product::(\w+), Product::(\w+)\}", table)
    assert len(got) == len(EDGES) == 20 and sorted(got) == sorted(EDGES)
    names = re.search(r"enum class Product \{([^}]*)\}", text).group(1).replace(" ", "").split(",")
    assert names[:-1] == ["reads", "names", "seeds", "probe", "chains", "built", "ext", "dedup", "pair", "er", "al", "sam", "bam", "sorted",
                          "templates", "template_locs"] and names[-1] == "kCount"
    assert set(ORDER) | {"built"} == set(names[:-1])


@pytest.mark.parametrize("paired", [False, True])
def test_in_order_twice(paired, index):
    """A, then B, then A again on one batch: the second A's SAM and BAM bytes are the first's"""
    b = capi.Batch(index, 8, 1000)
    opt, sopt = capi.default_mem_opt(), capi.default_sam_opt()

    def through(c):
        b.seed_upload(c["enc"], c["cum"])
        b.sam_upload([b"p%d" % (i // 2 if paired else i) for i in range(c["n"])], c["quals"])
        b.seed_run(with_sa=True); b.chain_run(opt); b.extend_run(opt); b.dedup_run(opt)
        if paired:
            b.pair_run(PES0, opt)
            b.reg2aln_sam(opt, sopt, pes=PES0, fetch=False)
            b.sam_run_pe(PES0, opt, sopt)
        else:
            b.mark_primary_se(opt, id_base=0)
            b.reg2aln_sam(opt, sopt, fetch=False)
            b.sam_run(opt, sopt)
        sam = b.sam_fetch()[0]
        b.bam_run()
        return sam, b.bam_fetch()[0]
    ca, cb = (PA, PB) if paired else (A, B)
    first = through(ca)
    other = through(cb)
    assert through(ca) == first and other != first
    assert first[0].count(b"\n") >= ca["n"] and other[0].count(b"\n") >= cb["n"] and len(first[1]) > len(other[1]) > 0
    b.close()


@pytest.mark.parametrize("producer,derived", EDGES)
def test_edge(producer, derived, index, emf, want):
    """after the producer ran again on the same inputs, what reads the derived product is refused with its own text; the stages
    between, run again in order, give the first run's bytes"""
    p = Pipe(index, emf)
    if derived == "built":
        p.run(A, upto="chains")
        p.make["built"]()
    else:
        p.run(A)
    first = p.fetch[derived]()
    assert first == want["A"][derived]
    if producer == "templates":
        p.replace_templates()
    else:
        p.make[producer]()
    call, text = p.reader[derived]
    if derived == "names":                                      # the text reads the names last: everything else it reads is made anew
        p.run(A, only=(_derived(producer) & _ancestors("sam")) - {"names"})
    _refused(call(), text)
    # everything the producer outdated, in order, through the derived product (a seed run reads the skip flags a probe sets, so the
    # stages beside the straight line run again too)
    again = _derived(producer)
    if derived == "built":
        p.run(A, only=again, upto="chains")
        p.make["built"]()
    else:
        p.run(A, only=again, upto="sam" if derived == "names" else derived)
    assert p.fetch[derived]() == first
    if derived == "names":
        assert p.fetch["sam"]() == want["A"]["sam"]
    p.close()


def test_independent_products_stay(index, emf, want):
    p = Pipe(index, emf)
    p.run(A)
    p.make["seeds"]()                                           # a new seed run: the filter's regions and the names stay
    assert p.fetch["er"]() == want["A"]["er"] and p.fetch["probe"]() == want["A"]["probe"]
    p.run(A, only={"chains", "ext", "dedup", "pair", "al", "sam"})
    assert p.fetch["sam"]() == want["A"]["sam"]                 # ... accepted by the text, which reads both
    p.make["names"]()                                           # new names: the alignment records stay
    assert p.fetch["al"]() == want["A"]["al"]
    p.run(A, only={"sam", "bam"})
    p.make["sorted"]()                                          # a sort: the text stays
    assert p.fetch["sam"]() == want["A"]["sam"] and p.fetch["bam"]() == want["A"]["bam"]
    p.close()


def _stale_calls(p):
    """every run and fetch that reads something made from the reads: (name, raw call)"""
    L, h, o, n = capi.lib(), p.b.h, C.byref(p.opt), C.c_int64(0)
    calls = [(k, c) for k, (c, _) in p.reader.items()]
    calls += [
        ("bwams_extend_run", lambda: L.bwams_extend_run(h, o, None)),
        ("bwams_dedup_run", lambda: L.bwams_dedup_run(h, o, None)),
        ("bwams_pair_run", lambda: L.bwams_pair_run(h, o, capi._p(PES0), 0, 4, None, None)),
        ("bwams_reg2aln_run 0", lambda: L.bwams_reg2aln_run(h, o, 0, None, None, None)),
        ("bwams_reg2aln_run 1", lambda: L.bwams_reg2aln_run(h, o, 1, None, None, None)),
        ("bwams_sam_run", lambda: L.bwams_sam_run(h, o, C.byref(p.sopt), C.byref(n))),
        ("bwams_bam_run", lambda: L.bwams_bam_run(h, None, None)),
        ("bwams_emf_regs_run", lambda: L.bwams_emf_regs_run(h, p.e.h, o, C.byref(n))),
        ("bwams_emf_regs_merge", lambda: L.bwams_emf_regs_merge(h, C.byref(n))),
        ("bwams_seed_fetch", lambda: L.bwams_seed_fetch(h, None, 0, None, 0, None)),
        ("bwams_chain_fetch", lambda: L.bwams_chain_fetch(h, None, 0, None, 0, None)),
        ("bwams_extend_fetch", lambda: L.bwams_extend_fetch(h, None, 0, None, None)),
        ("bwams_emf_fetch", lambda: L.bwams_emf_fetch(h, None, None)),
        ("bwams_bam_sort", lambda: L.bwams_bam_sort(h, None)),
        ("bwams_bam_templates", lambda: L.bwams_bam_templates(h, None, None)),
    ]
    return calls


@pytest.mark.parametrize("how", ["seed_upload", "emf_probe"])
def test_new_chunk(how, index, emf, want):
    """A to the end, then B's reads: nothing of A is handed out or computed on, and B then runs in order to its own bytes"""
    p = Pipe(index, emf)
    p.run(A)
    d = capi.Deflater(0, 1 << 20)
    L, n = capi.lib(), C.c_int64(0)
    calls = _stale_calls(p)
    calls += [("bwams_sam_fetch_bgzf", lambda: L.bwams_sam_fetch_bgzf(p.b.h, d.h, None, 0, 0, C.byref(n))),
              ("bwams_bam_fetch_bgzf", lambda: L.bwams_bam_fetch_bgzf(p.b.h, d.h, None, 0, 0, C.byref(n)))]
    if how == "seed_upload":
        p.b.seed_upload(B["enc"], B["cum"])
    else:
        p.b.emf_probe(emf, B["enc"], B["cum"])                  # the probe's own upload is no bwams_seed_upload: the seed run goes too
        so = capi.default_seed_opt()
        calls.append(("bwams_seed_run", lambda: L.bwams_seed_run(p.b.h, C.byref(so), 1)))
    for name, call in calls:
        assert call() == ERR_ARG, name
    p.run(B)                                                    # the refusals left nothing behind
    for k in ("er", "pair", "al", "sam", "bam", "sorted", "templates", "template_locs"):
        assert p.fetch[k]() == want["B"][k], k
    d.close()
    p.close()


def test_documented_gap_is_closed(index, emf, want):
    """a new chain run outdates the text and the records: bwams_sam_fetch and the record consumers refuse, each with its text"""
    p = Pipe(index, emf)
    p.run(A)
    p.make["chains"]()
    L, n = capi.lib(), C.c_int64(7)
    _refused(L.bwams_sam_fetch(p.b.h, None, 0, None, None, 0), "bwams_sam_fetch: run bwams_sam_run first")
    handles = {"bwams_depth_add_batch": capi.Depth([len(GENOME)]), "bwams_pileup_add_batch": capi.Pileup([len(GENOME)]),
               "bwams_qc_add_batch": capi.Qc(), "bwams_recal_add_batch": capi.Recal([len(GENOME)])}
    for sym, hd in handles.items():
        _refused(getattr(L, sym)(hd.h, p.b.h, C.byref(n)), sym + ": run bwams_bam_run or bwams_bam_upload first")
        hd.close()
    assert n.value == 7
    p.run(A, only=_derived("chains") - {"built"})
    for k in ("sam", "bam", "sorted", "template_locs"):
        assert p.fetch[k]() == want["A"][k], k
    p.close()
