"""Builders shared by test_dup_join.py and test_gpu_dup_join.py: the names of rule J1's test, the equivalence input (one set of
records in query-grouped order and in coordinate order, on which the adjacent-run rules and the name join must agree), and small
helpers over records."""
import struct

import numpy as np

from bwams import bam, markdup
from test_markdup import P1, P2, R, rec

# rule J1's vectors: name -> (k0, k1)
VECTORS = {
    b"": (0x9ca066f1a4ab2eea, 0x0ff2e69699c4857e),
    b"r1": (0xf725c5a0830ac16d, 0xb55003a821483129),
    b"read/1:x": (0xd42f88ba882ae719, 0xd04e53c85105c70b),
    b"read/1:xy": (0x668dd5c4adcadc45, 0x377db6df6717d7dd),
    b"A" * 17: (0xc9d199ad14f70290, 0x8e60ec9c43d9bb4b),
    b"HWI:1:FC:2:1101:1000:2000": (0x9fb5b6d6477062c2, 0x023407d2be740ffb),
}


def key_names() -> list:
    """names of length 0, 1, 7, 8, 9, 16, 17 and 254; two that differ only in their last byte; a name and its proper prefix"""
    base = bytes(33 + k % 90 for k in range(254))
    return [base[:n] for n in (0, 1, 7, 8, 9, 16, 17, 254)] + [b"lane:7:tile:x1", b"lane:7:tile:x2", b"prefix_of_a_name", b"prefix_of"]


def cleared(r: bytes) -> bytes:
    return markdup.set_dup(r, False)


def by_record(marked) -> dict:
    """marked records (bytes, or a list of them) keyed by themselves with 0x400 cleared; the records must be distinct"""
    recs = bam.split_records(marked) if isinstance(marked, (bytes, bytearray)) else list(marked)
    out = {cleared(r): r for r in recs}
    assert len(out) == len(recs)
    return out


def names_of(records) -> list:
    recs = bam.split_records(records) if isinstance(records, (bytes, bytearray)) else list(records)
    return [r[36:36 + r[12] - 1] for r in recs]


QUALS = b"0:DI"                                          # 15, 25, 35, 40: a copy's quality character, each copy of a site another


def equivalence_input(seed: int = 5, n_sites: int = 600):
    """(templates: a list of record lists in query-grouped order, shuffled; the same records in stable coordinate order).  Every
    site holds one template, every third site also 1 to 3 planted copies at the same unclipped 5' coordinates, each with another
    quality character, so that no decision rests on a tie-break by order; the two conditions are asserted below."""
    rng = np.random.default_rng(seed)
    templates = []
    for s in range(n_sites):
        pos = 1000 + 300 * s
        kind = s % 5
        n_copies = 1 + (int(rng.integers(1, 4)) if s % 3 == 0 else 0)     # the site's template and its planted copies
        quals = [QUALS[int(k)] for k in rng.permutation(4)[:n_copies]]
        swap = bool(rng.integers(0, 2))
        for c, q in enumerate(quals):
            name, qual = b"s%d_%d" % (s, c), bytes([q])
            if kind in (0, 1):                               # an FR pair, in either record order
                t = [rec(name, P1, pos, b"120M", qual), rec(name, P2 | R, pos + 150, b"120M", qual)]
                if kind == 1:                                # with a supplementary record on another contig
                    t.append(rec(name, P1 | 0x800, 500 + 100 * s, b"60H60M", qual, ref=b"c1"))
                if swap:
                    t[0], t[1] = t[1], t[0]
            elif kind == 2:                                  # a clipped fragment, forward: the copies clipped differently
                clip = 3 * c
                t = [rec(name, 0, pos + clip, b"%dS%dM" % (clip, 120 - clip) if clip else b"120M", qual)]
            elif kind == 3:                                  # a clipped fragment, reverse
                clip = 2 * c
                t = [rec(name, R, pos, b"%dM%dS" % (110 - clip, 10 + clip), qual)]
            else:                                            # a fragment with an unmapped mate, placed with it
                t = [rec(name, P1 | 0x8, pos, b"120M", qual), rec(name, P2 | 0x4, pos, b"*")]
                if swap:
                    t.reverse()
            templates.append(t)
    templates = [templates[k] for k in rng.permutation(len(templates))]
    grouped = [r for t in templates for r in t]
    assert len(set(grouped)) == len(grouped)
    # the two conditions under which input order cannot matter
    n_t, ends, _ = markdup.ends(grouped)
    groups = {}
    for e in ends:
        key = (e["ref1"], e["pos1"], e["strands"] & 1) + ((e["ref2"], e["pos2"], e["strands"] >> 1) if e["ref2"] >= 0 else ())
        groups.setdefault(key, []).append(e["score"])
        assert (e["ref1"], e["pos1"]) != (e["ref2"], e["pos2"])              # no pair has both ends at one place
    assert all(len(set(v)) == len(v) for v in groups.values())               # no two templates of one key group have equal scores
    assert any(len(v) > 1 for v in groups.values())
    return templates, bam.split_records(bam.coord_sort(b"".join(grouped)))


def flag_of(r: bytes) -> int:
    return struct.unpack_from("<H", r, 18)[0]
