"""The front door that depth, pileup, QC, recalibration and its apply share (csrc/rec_consumer.h): what each handle's add from a batch
and add from host records refuse before any kernel runs, by code and by the exact text of bwams_last_error, and what an empty add
leaves behind.  One reference of 200 bases and three hand-built records."""
import ctypes as C

import numpy as np
import pytest

from bwams import bam, capi, simulate
import test_recal_model as M

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -3
L_REF = [200]
SAM = (b"r0\t0\tref\t11\t60\t8M\t*\t0\t0\tACGTACGT\tIIIIIIII\n"
       b"r1\t16\tref\t21\t60\t4M1I3M\t*\t0\t0\tACGTTACG\tIIIIHHHH\n"
       b"r2\t0\tref\t31\t30\t8M\t*\t0\t0\tTTGCATGC\t55555555\n")
RECS = bam.encode_records(SAM, [b"ref"])


def _apply(device=0):
    m = capi.RecalModel(M.zero_tables(0, 16), 16)
    a = capi.RecalApply(m, None, device)
    m.close()                                                                   # the handle holds its own copy
    return a


def _state_depth(h):
    h.finish()
    return h.fetch(0).tolist()


def _state_qc(h):
    flags, scalars = h.summary()
    return [flags.tolist(), scalars.tolist()] + [h.table(k).tolist() for k in range(6)]


# name: (open on a device, the add from a batch, the add from host records, what the handle holds)
HANDLES = {
    "depth": (lambda dev=0: capi.Depth(L_REF, device=dev), "bwams_depth_add_batch", "bwams_depth_add_records", _state_depth),
    "pileup": (lambda dev=0: capi.Pileup(L_REF, device=dev), "bwams_pileup_add_batch", "bwams_pileup_add_records",
               lambda h: h.fetch(0).tolist()),
    "qc": (lambda dev=0: capi.Qc(device=dev), "bwams_qc_add_batch", "bwams_qc_add_records", _state_qc),
    "recal": (lambda dev=0: capi.Recal(L_REF, device=dev), "bwams_recal_add_batch", "bwams_recal_add_records",
              lambda h: [h.table(k).tolist() for k in range(4)]),
    "apply": (_apply, "bwams_recal_apply_batch", "bwams_recal_apply_records", lambda h: h.info()["model_bytes"]),    # it holds no table
}


@pytest.fixture(scope="module")
def index():
    ix = capi.Index.build(simulate.make_genome(3000, seed=3, repeat_frac=0.0), 0)
    yield ix
    ix.close()


def _device_count() -> int:
    n = C.c_int(0)
    capi.lib().bwams_device_count(C.byref(n))
    return n.value


def _refused(rc: int, text: str):
    assert rc == ERR_ARG
    assert capi.lib().bwams_last_error().decode() == text


@pytest.mark.parametrize("name", list(HANDLES))
def test_front_door(name, index):
    L = capi.lib()
    make, batch_sym, records_sym, state = HANDLES[name]
    add_batch, add_records = getattr(L, batch_sym), getattr(L, records_sym)
    n = C.c_int64(7)
    h = make()
    bare = capi.Batch(index, 10, 1000)                                          # neither bwams_bam_run nor bwams_bam_upload
    full = capi.Batch(index, 10, 1000)
    try:
        _refused(add_batch(h.h, bare.h, C.byref(n)), batch_sym + ": run bwams_bam_run or bwams_bam_upload first")
        _refused(add_batch(h.h, None, C.byref(n)), batch_sym + ": run bwams_bam_run or bwams_bam_upload first")
        _refused(add_records(h.h, None, 5, C.byref(n)), records_sym + ": a handle and host records are required")
        _refused(add_records(h.h, None, -1, C.byref(n)), records_sym + ": a handle and host records are required")
        cut = np.frombuffer(RECS[:-1], np.uint8).copy()                         # the chain, as bwams_bam_upload checks it
        size = len(bam.split_records(RECS)[2]) - 4
        _refused(add_records(h.h, cut.ctypes.data_as(C.c_void_p), len(cut), C.byref(n)),
                 "%s: record 2: block_size %d runs past n_bytes" % (records_sym, size))
        short = len(RECS) - len(bam.split_records(RECS)[2]) + 3                 # not even the last record's block_size
        _refused(add_records(h.h, cut.ctypes.data_as(C.c_void_p), short, C.byref(n)), records_sym + ": record 2 is cut off")
        assert cut.tobytes() == RECS[:-1] and n.value == 7                      # no refusal touched either
        buf = np.frombuffer(RECS, np.uint8).copy()
        assert add_records(h.h, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(n)) == OK and n.value == 3
        assert full.bam_upload(RECS) == 3
        assert add_batch(h.h, full.h, C.byref(n)) == OK and n.value == 3
        n.value = 7
        assert add_records(h.h, buf.ctypes.data_as(C.c_void_p), 0, C.byref(n)) == OK and n.value == 0     # zero bytes
        n.value = 7
        assert add_records(h.h, None, 0, C.byref(n)) == OK and n.value == 0
        twice = make()                                                          # the two adds and nothing else
        try:
            assert add_records(twice.h, buf.ctypes.data_as(C.c_void_p), len(buf), None) == OK
            assert add_batch(twice.h, full.h, None) == OK
            assert state(h) == state(twice)
        finally:
            twice.close()
        if _device_count() > 1:                                                 # with one GPU the device check does not run
            far = make(1)
            try:
                _refused(add_batch(far.h, full.h, C.byref(n)), batch_sym + ": the handle is on device 1, the batch on device 0")
                _refused(add_batch(far.h, bare.h, C.byref(n)), batch_sym + ": run bwams_bam_run or bwams_bam_upload first")
            finally:
                far.close()
    finally:
        h.close()
        bare.close()
        full.close()


def test_finished_depth(index):
    """a finished depth handle refuses both adds; a batch without BAM records is named first, a cut buffer after"""
    L = capi.lib()
    n = C.c_int64(7)
    d = capi.Depth(L_REF)
    bare = capi.Batch(index, 10, 1000)
    full = capi.Batch(index, 10, 1000)
    try:
        assert d.add_records(RECS) == 3
        want = d.finish().fetch(0).tolist()
        assert full.bam_upload(RECS) == 3
        _refused(L.bwams_depth_add_batch(d.h, full.h, C.byref(n)),
                 "bwams_depth_add_batch: the handle is finished (bwams_depth_reset starts it again)")
        _refused(L.bwams_depth_add_records(d.h, RECS, len(RECS), C.byref(n)),
                 "bwams_depth_add_records: the handle is finished (bwams_depth_reset starts it again)")
        _refused(L.bwams_depth_add_records(d.h, RECS, 0, C.byref(n)),
                 "bwams_depth_add_records: the handle is finished (bwams_depth_reset starts it again)")
        _refused(L.bwams_depth_add_records(d.h, RECS, len(RECS) - 1, C.byref(n)),
                 "bwams_depth_add_records: the handle is finished (bwams_depth_reset starts it again)")
        _refused(L.bwams_depth_add_batch(d.h, bare.h, C.byref(n)), "bwams_depth_add_batch: run bwams_bam_run or bwams_bam_upload first")
        _refused(L.bwams_depth_add_records(d.h, None, 5, C.byref(n)), "bwams_depth_add_records: a handle and host records are required")
        assert n.value == 7 and d.fetch(0).tolist() == want
    finally:
        d.close()
        bare.close()
        full.close()
