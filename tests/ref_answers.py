"""Answers of the reference objects (oracle/_ref) for the tests that pin the restatements to them.

oracle/_ref is compiled from the reference tree only where that tree is present (oracle/Makefile).  There, every answer a test
asks for is computed by the reference objects and checked against the stored one; elsewhere the stored answers stand in for
them.  They live in tests/golden/ref_answers.npz, per test and in call order, and are written by tests/make_ref_answers.py.
"""
import ast
import hashlib
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.npz")
RECORD = False          # set by tests/make_ref_answers.py: collect the live answers instead of checking them
RECORDED = {}           # test id -> list of 1-D arrays, in call order
_stored = None


def _store():
    global _stored
    if _stored is None:
        _stored = dict(np.load(PATH, allow_pickle=False)) if os.path.exists(PATH) else {}
    return _stored


def _test_id():
    """'test_file.py::test_name[params]' of the running test, whatever directory pytest was started from."""
    cur = os.environ["PYTEST_CURRENT_TEST"].rsplit(" ", 1)[0]
    return cur.rsplit("/", 1)[-1]


class Answers:
    """ans(lambda: <call of a reference object>) -> its answer as a 1-D numpy array (a scalar or tuple becomes one)."""

    def __init__(self, live: bool):
        self.key, self.live, self.i = _test_id(), live, 0
        s = _store()
        self.data, self.ends, self.kinds = s.get(self.key + ":data"), s.get(self.key + ":ends"), s.get(self.key + ":kinds")
        self.dtypes = None if self.data is None else [np.lib.format.descr_to_dtype(d)
                                                      for d in ast.literal_eval(str(s[self.key + ":dtypes"]))]
        if RECORD:
            RECORDED[self.key] = []
        elif self.data is None:
            assert live, f"no stored reference answers for {self.key}: run tests/make_ref_answers.py where oracle/_ref is built"

    def _stored(self, i):
        assert i < len(self.ends), f"{self.key}: more reference calls than stored answers ({len(self.ends)})"
        a = 0 if i == 0 else int(self.ends[i - 1])
        return np.frombuffer(self.data[a:int(self.ends[i])].tobytes(), self.dtypes[int(self.kinds[i])])

    def __call__(self, compute):
        i, self.i = self.i, self.i + 1
        if not self.live:
            return self._stored(i).copy()
        v = np.ascontiguousarray(np.asarray(compute())).reshape(-1)
        if RECORD:
            RECORDED[self.key].append(v)
        elif self.data is not None:
            w = self._stored(i)
            assert w.dtype == v.dtype and w.tobytes() == v.tobytes(), f"{self.key}: stored answer {i} differs from the reference objects'"
        return v

    def same(self, ours, compute) -> bool:
        """Whether the integer array `ours` equals the reference's answer; only its SHA-256 is kept (the sorts' large permutations)."""
        return bool(np.array_equal(self(lambda: _digest(compute())), _digest(ours)))


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(np.asarray(a), np.int64).tobytes()).digest(), np.uint8)


def save(path=PATH):
    out = {}
    for key, vals in sorted(RECORDED.items()):
        if not vals:
            continue
        dts = []
        for v in vals:
            if v.dtype not in dts:
                dts.append(v.dtype)
        out[key + ":data"] = np.frombuffer(b"".join(v.tobytes() for v in vals), np.uint8)
        out[key + ":ends"] = np.cumsum([v.nbytes for v in vals]).astype(np.int64)
        out[key + ":kinds"] = np.array([dts.index(v.dtype) for v in vals], np.int8)
        out[key + ":dtypes"] = np.array(repr([np.lib.format.dtype_to_descr(d) for d in dts]))
    np.savez_compressed(path, **out)
    return out
