"""tests/bsw_early_ref.c compiled with the host compiler and wrapped: the scalar banded-SW loop with the early-exit rule
(mode 0: off, 1: after every row, 2: after every fourth row) and the two task families of test_bsw_early_exit_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle.loader import SEQPAIR_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class EarlyRef:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libbsw_early_ref.so")
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               os.path.join(HERE, "bsw_early_ref.c"), "-o", so])
        self.lib = C.CDLL(so)
        self.lib.bsw_early_pairs.restype = None
        self.lib.bsw_early_pairs.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 3
        self.lib.bsw_early_gen_reads.restype = C.c_int64
        self.lib.bsw_early_gen_reads.argtypes = [C.c_uint64, C.c_int64] + [C.c_void_p] * 3
        self.lib.bsw_early_gen_adversarial.restype = None
        self.lib.bsw_early_gen_adversarial.argtypes = [C.c_uint64, C.c_int64] + [C.c_void_p] * 3

    def run(self, pairs, ref, qer, w, opt, mode):
        """-> (pairs with the six outputs, cells per task, rows per task, ended-by-the-rule per task)"""
        p = np.ascontiguousarray(pairs).copy()
        n = len(p)
        cells, rows, by_rule = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        self.lib.bsw_early_pairs(C.byref(opt), _p(p), _p(np.ascontiguousarray(ref)), _p(np.ascontiguousarray(qer)), n, w, mode,
                                 _p(cells), _p(rows), _p(by_rule))
        return p, cells, rows, by_rule.astype(bool)

    def gen_reads(self, seed, cap):
        pairs = np.zeros(cap, SEQPAIR_DTYPE)
        ref, qer = np.zeros(cap * 400 + 1, np.uint8), np.zeros(cap * 150 + 1, np.uint8)
        n = self.lib.bsw_early_gen_reads(seed, cap, _p(pairs), _p(ref), _p(qer))
        return pairs[:n], ref, qer

    def gen_adversarial(self, seed, n):
        pairs = np.zeros(n, SEQPAIR_DTYPE)
        ref, qer = np.zeros(n * 330 + 1, np.uint8), np.zeros(n * 160 + 1, np.uint8)
        self.lib.bsw_early_gen_adversarial(seed, n, _p(pairs), _p(ref), _p(qer))
        return pairs, ref, qer
