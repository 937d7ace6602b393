"""BAM records viewed as SAM text, without a GPU: the restatement (bwams/samview.py) against hand-written (record, line) pairs, against
the project's own encoder over canonical SAM texts (view(encode(text)) == text) and bam.decode where that does not raise; the host
function bwams_fmt_float (csrc/fmt_g.h, the code the kernels call) against "%g"; rule V6's check, a record per reason.
tests/test_gpu_samview.py runs the same cases through bwams_samview_t."""
import numpy as np
import pytest

from bwams import bam, capi, samview
from samview_cases import LITERALS, NAMED_BITS, NAMED_FLOATS, N_REF, NAMES, OK, REFUSALS, canonical_texts, float_bits


@pytest.mark.parametrize("what,rec,line", LITERALS, ids=[c[0] for c in LITERALS])
def test_literal_pairs(what, rec, line):
    assert samview.check_record(rec, N_REF) is None
    assert samview.format_record(rec, NAMES) == line


def test_literal_pairs_as_one_add():
    recs = [r for _, r, _ in LITERALS]
    text, off = samview.view(b"".join(recs), NAMES)
    assert text == b"".join(ln for _, _, ln in LITERALS)
    assert off.dtype == np.int64 and off.tolist() == np.concatenate([[0], np.cumsum([len(ln) for _, _, ln in LITERALS])]).tolist()
    assert samview.view(b"", NAMES)[0] == b"" and samview.view(b"", NAMES)[1].tolist() == [0]


def test_restatement_against_the_encoder():
    for names, text in canonical_texts():
        enc = bam.encode_records(text, names)
        got, off = samview.view(enc, names)
        assert got == text
        assert [got[a:b] for a, b in zip(off[:-1], off[1:])] == [ln + b"\n" for ln in text.split(b"\n")[:-1]]
        assert bam.decode(enc, names)[2] == got                      # the test helper agrees wherever it does not raise
    with pytest.raises(ValueError):                                  # ... and it raises on B arrays, which the view prints
        bam.decode(LITERALS[8][1], NAMES)


def test_filter():
    recs = bam.split_records(bam.encode_records(canonical_texts()[0][1], NAMES))
    flags = [int.from_bytes(r[18:20], "little") for r in recs]
    mapqs = [r[13] for r in recs]
    for req, exc, mq in ((0, 0, 0), (1, 0, 0), (0, 4, 0), (0, 0, 37), (0x41, 0x800, 1), (0xFFFF, 0, 0), (0, 0, 256)):
        text, off = samview.view(recs, NAMES, req, exc, mq)
        keep = [(f & req) == req and not f & exc and q >= mq for f, q in zip(flags, mapqs)]
        assert text == b"".join(samview.format_record(r, NAMES) for r, k in zip(recs, keep) if k) and len(off) == sum(keep) + 1


def test_fmt_float_against_percent_g():
    """csrc/fmt_g.h on the host: every exponent byte x {0, 1, 0x400000, 0x7FFFFF, 64 random mantissas} x both signs, and the ties
    and edges by name"""
    bits = float_bits()
    assert len(bits) == 2 * 256 * 68 + len(NAMED_FLOATS) + len(NAMED_BITS)
    values = bits.view(np.float32)
    bad = [(hex(b), capi.fmt_float(np.uint32(b)), samview.fmt_g(x)) for b, x in zip(bits, values)
           if capi.fmt_float(np.uint32(b)) != samview.fmt_g(x)]
    assert not bad, bad[:10]
    assert max(len(capi.fmt_float(np.uint32(b))) for b in bits) <= 13
    named = [(1234565, b"1.23456e+06"), (1234575, b"1.23458e+06"), (9999995, b"1e+07"), (999999.5, b"1e+06"),
             (99999.95, b"100000"),                                  # the float is 99999.953125
             (100000, b"100000"), (999999, b"999999"), (1e6, b"1e+06"), (0.0001, b"0.0001"), (1e-5, b"1e-05"), (0.0, b"0"),
             (-0.0, b"-0"), (np.inf, b"inf"), (-np.inf, b"-inf"), (1.17549435e-38, b"1.17549e-38"), (3.40282347e38, b"3.40282e+38")]
    for x, want in named:
        assert capi.fmt_float(x) == want == samview.fmt_g(x), x
    below = np.nextafter(np.float32(0.0001), np.float32(0))          # 9.99999902e-05 still rounds up to six digits of 1.00000e-04
    assert capi.fmt_float(below) == b"0.0001" and capi.fmt_float(np.float32(9.999994e-05)) == b"9.99999e-05"
    assert capi.fmt_float(np.uint32(1)) == b"1.4013e-45" and capi.fmt_float(np.uint32(0x80000001)) == b"-1.4013e-45"
    assert capi.fmt_float(np.uint32(0x7FC00000)) == b"nan" and capi.fmt_float(np.uint32(0xFFC00000)) == b"-nan"


@pytest.mark.parametrize("what,rec,why", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_check_one_record_per_reason(what, rec, why):
    assert samview.check_record(rec, N_REF) == why
    assert samview.check([OK, OK, rec, OK], N_REF) == (2, samview.REASONS[why])
    with pytest.raises(samview.Refused) as e:
        samview.view(OK + rec, NAMES, exclude=0xFFFF)                # filtered records are checked too
    assert (e.value.ordinal, e.value.reason) == (1, samview.REASONS[why])


def test_check_smallest_ordinal():
    assert {w for _, _, w in REFUSALS} == {1, 2, 3, 4, 5}
    assert samview.check([OK] * 5, N_REF) is None and samview.check(b"", N_REF) is None
    first = {w: r for _, r, w in reversed(REFUSALS)}
    assert samview.check([OK, OK, OK, first[5], OK, first[1]], N_REF) == (3, samview.REASONS[5])
    assert samview.check(b"".join([OK, first[3], first[2]]), N_REF) == (1, samview.REASONS[3])
