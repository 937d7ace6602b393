"""The quality model and the rewriting of QUAL restated in numpy and Python ints: the yardstick of host/recal_model.cpp and
csrc/recal_apply.hip.

The model's definitions and the apply rules A to C are in include/bwams.h above bwams_recal_model_create; the letters below are
theirs.  Every value is an integer: S and P come from their exact definitions by an integer root search, phred() and post() are
comparisons of products, and no float and no log is on the way from the tables to the new QUAL bytes.
"""
from __future__ import annotations

import struct

import numpy as np

from bwams import bam, markdup
from bwams.recal import CONTEXT, CYCLE, N_QUAL, QUAL, RG, _BASE_OF_CODE

MAX_COUNT = 1 << 40                                                                      # a count of the tables stays below this


def _root(x: int, k: int) -> int:
    """the largest r with r ** k <= x"""
    lo, hi = 0, 1 << (x.bit_length() // k + 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid ** k <= x:
            lo = mid
        else:
            hi = mid
    return lo


# S[k], k = 1..60: the largest s with s^20 <= 2^320 * 10^(2k - 1), that is floor(2^16 * 10^((2k - 1) / 20)); S[0] is not used
S = [0] + [_root((1 << 320) * 10 ** (2 * k - 1), 20) for k in range(1, 61)]
# P[q], q = 0..93: the largest p with p^10 * 10^q <= 2^400, that is floor(2^40 * 10^(-q / 10))
P = [_root((1 << 400) // 10 ** q, 10) for q in range(N_QUAL)]


def phred(num: int, den: int, cap: int) -> int:
    """the number of k in 1..cap with num * S[k] <= den << 16: round(-10 log10(num / den)) clamped to [0, cap]"""
    return sum(1 for k in range(1, cap + 1) if num * S[k] <= den << 16)


def post(n: int, e: int, qp: int, m: int, cap: int) -> int:
    """the quality of a cell of n observations and e errors after m pseudo-observations at the prior quality qp"""
    return phred((e << 40) + m * P[qp], (n + m) << 40, cap)


class ModelRefusal(ValueError):
    """.code: "arg" (an option out of range: BWAMS_ERR_ARG) or "unsupported" (a count the model does not take)"""

    def __init__(self, code: str, what: str):
        super().__init__(what)
        self.code = code


class ApplyRefusal(ValueError):
    """Rule B (BWAMS_ERR_ARG); .record is the record's index in the call, .why "bounds", "cycle" or "aux"."""

    def __init__(self, record: int, why: str):
        super().__init__(f"record {record}: {why}")
        self.record, self.why = record, why


class Model:
    """tables: the four count tables in the shapes of recal.Recal.tables (int64 pairs)."""

    def __init__(self, tables, max_cycle: int, exclude: int = 0, preserve_below: int = 6, max_q: int = 60, prior_obs: int = 1024,
                 reserved: int = 0):
        if not (0 <= exclude <= 0xFFFF and 0 <= preserve_below <= 93 and 1 <= max_q <= 60 and 1 <= prior_obs <= 1 << 20 and reserved == 0):
            raise ModelRefusal("arg", "options")
        if max_cycle < 1:
            raise ModelRefusal("arg", "max_cycle")
        t = [np.asarray(x, np.int64) for x in tables]
        g = t[RG].shape[0]
        cols = 2 * max_cycle + 1
        assert t[RG].shape == (g, 2) and t[QUAL].shape == (g, N_QUAL, 2) and t[CYCLE].shape == (g, N_QUAL, cols, 2)
        assert t[CONTEXT].shape == (g, N_QUAL, 16, 2)
        for x in t:
            if (x < 0).any() or (x[..., 1] > x[..., 0]).any() or (x >= MAX_COUNT).any():
                raise ModelRefusal("unsupported", "a negative count, more errors than observations, or a count of 2^40 or more")
        self.n_rg, self.max_cycle = g - 1, max_cycle
        self.exclude, self.preserve_below, self.max_q, self.prior_obs = exclude, preserve_below, max_q, prior_obs
        m, cap = prior_obs, max_q
        self.rg = np.zeros((g, 3), np.int16)
        self.b = np.zeros((g, N_QUAL), np.int16)
        self.dc = np.zeros((g, N_QUAL, cols), np.int16)
        self.dx = np.zeros((g, N_QUAL, 16), np.int16)
        for k in range(g):
            n, e = int(t[RG][k, 0]), int(t[RG][k, 1])
            if n > 0:
                err = sum(int(t[QUAL][k, q, 0]) * P[q] for q in range(N_QUAL))
                qrep = phred(err, n << 40, cap)
                qg = post(n, e, qrep, m, cap)
                self.rg[k] = [qrep, qg, qg - qrep]
            else:
                self.rg[k] = [-1, -1, 0]
            for q in range(N_QUAL):
                qp = min(max(q + int(self.rg[k, 2]), 0), 93)
                n, e = int(t[QUAL][k, q, 0]), int(t[QUAL][k, q, 1])
                b = post(n, e, qp, m, cap) if n > 0 else qp
                self.b[k, q] = b
                for c in np.flatnonzero(t[CYCLE][k, q, :, 0]):
                    self.dc[k, q, c] = post(int(t[CYCLE][k, q, c, 0]), int(t[CYCLE][k, q, c, 1]), b, m, cap) - b
                for x in np.flatnonzero(t[CONTEXT][k, q, :, 0]):
                    self.dx[k, q, x] = post(int(t[CONTEXT][k, q, x, 0]), int(t[CONTEXT][k, q, x, 1]), b, m, cap) - b

    def table(self, what: int) -> np.ndarray:
        """int16: RG [n_rg + 1][3] = (Qrep, QG, G); QUAL B [n_rg + 1][94]; CYCLE DC [n_rg + 1][94][2 max_cycle + 1]; CONTEXT DX [..][94][16]"""
        return [self.rg, self.b, self.dc, self.dx][what]


def _head(rec: bytes):
    """(FLAG, l_seq, where SEQ, QUAL and the aux fields start) of one record with its block_size"""
    l_name, n_cig, flag, l_seq = struct.unpack_from("<BxxxHHi", rec, 12)
    seq_at = 36 + l_name + 4 * n_cig
    qual_at = seq_at + (l_seq + 1) // 2
    return flag, l_seq, seq_at, qual_at, qual_at + l_seq


def apply(records: bytes, model: Model, rg_ids=None):
    """Rules A to C over the records of `records` -> (the new bytes, the records rewritten).  rg_ids: the read groups' IDs by
    ordinal, or None for a model without read groups."""
    ids = None if rg_ids is None else [x if isinstance(x, bytes) else x.encode() for x in rg_ids]
    assert (0 if ids is None else len(ids)) == model.n_rg
    raw = bam.split_records(records)
    todo = []
    for k, rec in enumerate(raw):                                                        # rule B: all of them before any byte is written
        flag, l_seq, seq_at, qual_at, aux_at = _head(rec)
        if flag & model.exclude or l_seq <= 0:                                           # rule A
            continue
        if aux_at > len(rec):
            raise ApplyRefusal(k, "bounds")
        if rec[qual_at] == 0xFF:
            continue
        if l_seq > model.max_cycle:
            raise ApplyRefusal(k, "cycle")
        g = 0
        if ids is not None:
            try:
                v = markdup.read_group(rec)
            except ValueError:
                raise ApplyRefusal(k, "aux") from None
            g = ids.index(v) if v in ids else model.n_rg
        todo.append((k, g))
    out = [bytearray(r) for r in raw]
    for k, g in todo:
        rec = raw[k]
        flag, l_seq, seq_at, qual_at, _ = _head(rec)
        packed = np.frombuffer(rec, np.uint8, (l_seq + 1) // 2, seq_at)
        base = _BASE_OF_CODE[np.stack([packed >> 4, packed & 15], 1).reshape(-1)[:l_seq]]
        qual = np.frombuffer(rec, np.uint8, l_seq, qual_at).astype(np.int64)
        rev, neg = bool(flag & 0x10), flag & 0x81 == 0x81
        i = np.arange(l_seq)
        cyc = (l_seq - i if rev else i + 1) * (-1 if neg else 1)                         # recalibration rule 6
        nb = np.full(l_seq, -1, np.int64)
        if rev:
            nb[:-1] = base[1:]
            ctx = np.where((nb >= 0) & (base >= 0), 4 * (3 - nb) + (3 - base), -1)
        else:
            nb[1:] = base[:-1]
            ctx = np.where((nb >= 0) & (base >= 0), 4 * nb + base, -1)
        q = np.minimum(qual, N_QUAL - 1)
        v = model.b[g, q].astype(np.int64) + model.dc[g, q, cyc + model.max_cycle]
        v += np.where(ctx >= 0, model.dx[g, q, np.maximum(ctx, 0)], 0)
        v = np.clip(v, 1, model.max_q)                                                   # rule C
        new = np.where(qual < model.preserve_below, qual, v).astype(np.uint8)
        out[k][qual_at:qual_at + l_seq] = new.tobytes()
    return b"".join(bytes(r) for r in out), len(todo)
