"""A coordinate-sorted BAM collated by read name: rules C1-C5 of include/bwams.h (above bwams_collate_open) restated with a dict, as
the yardstick of csrc/collate.hip.  Nothing here knows of keys, sorts or pools (rules C7 and C8 are the device's business).

"Add order" is the order of the adds, then record order within each; a record's ORDINAL is its 0-based place in add order, skipped
records included.
  C1  records with FLAG 0x100 or 0x800 are skipped (and counted);
  C2  a kept record with 0x1 clear is single; with 0x1 set it is first (0x40 without 0x80) or last (0x80 without 0x40); 0x1 with
      both or neither is refused;
  C3  kept records in ordinal order: a single is emitted at once; a paired record whose name does not wait waits; one whose name
      waits with a record of the other segment completes the pair, and the name leaves the table; one whose name waits with a record
      of its own segment is refused.  Nothing remembers emitted names;
  C4  an add gives (pairs, singles): the pairs it completed, first record then last, in the order of the completing ordinals, and
      its singles in ordinal order, every record byte for byte;
  C5  the finish gives the waiting records in ordinal order, the orphans.
A refusal (C6) raises Refused with the ordinal and the reason; the state is as before the add.
"""
from __future__ import annotations

import struct

from . import bam

REASONS = ["FLAG 0x1 with both or neither of 0x40 and 0x80",
           "a second record of its segment while its name waits for the mate"]
BITS, SEGMENT = 0, 1
SKIP, SINGLE, FIRST, LAST = 0, 1, 2, 3


class Refused(Exception):
    """C6: .ordinal is the smallest ordinal at which the walk meets a fault, .reason an index into REASONS"""

    def __init__(self, ordinal: int, reason: int):
        self.ordinal, self.reason = ordinal, reason
        super().__init__(f"record {ordinal}: {REASONS[reason]}")


def flag_of(r: bytes) -> int:
    return struct.unpack_from("<H", r, 18)[0]


def name_of(r: bytes) -> bytes:
    """the name without its NUL"""
    return r[36:36 + max(r[12] - 1, 0)]


def segment(r: bytes, ordinal: int = 0) -> int:
    """C1 and C2: SKIP, SINGLE, FIRST or LAST"""
    f = flag_of(r)
    if f & 0x900:
        return SKIP
    if not f & 0x1:
        return SINGLE
    if (f & 0xC0) == 0x40:
        return FIRST
    if (f & 0xC0) == 0x80:
        return LAST
    raise Refused(ordinal, BITS)


def _records(add) -> list:
    return bam.split_records(add) if isinstance(add, (bytes, bytearray)) else list(add)


class Collate:
    """The walk as a handle: add() per piece, finish() once.  The counters are those of bwams_collate_info."""

    def __init__(self):
        self.pending = {}                                    # name -> (ordinal, segment, record); insertion order is not relied on
        self.records = self.skipped = self.pairs = self.singles = self.orphans = self.adds = 0
        self.bytes_pooled = 0
        self.finished = False

    def add(self, add):
        """-> (pairs: a list of (first, last), singles: a list of records); Refused leaves the state as it was"""
        assert not self.finished
        pending = dict(self.pending)
        pairs, singles, skipped = [], [], 0
        recs = _records(add)
        for k, r in enumerate(recs):
            ordinal = self.records + k
            seg = segment(r, ordinal)
            if seg == SKIP:
                skipped += 1
            elif seg == SINGLE:
                singles.append(r)
            else:
                name = name_of(r)
                if name not in pending:
                    pending[name] = (ordinal, seg, r)
                    continue
                _, pseg, p = pending[name]
                if pseg == seg:
                    raise Refused(ordinal, SEGMENT)
                del pending[name]
                pairs.append((r, p) if seg == FIRST else (p, r))
        pooled = sum(len(r) for o, _, r in pending.values() if o >= self.records)
        self.pending = pending
        self.records += len(recs)
        self.skipped += skipped
        self.pairs += len(pairs)
        self.singles += len(singles)
        self.bytes_pooled += pooled
        self.adds += 1
        return pairs, singles

    def pending_bytes(self) -> int:
        return sum(len(r) for _, _, r in self.pending.values())

    def finish(self) -> list:
        """-> the orphans in ordinal order"""
        self.finished = True
        out = [r for _, _, r in sorted(self.pending.values(), key=lambda x: x[0])]
        self.pending = {}
        self.orphans += len(out)
        return out


def collate(adds):
    """adds: byte strings of whole records (or lists of records) -> ([(pairs, singles) per add], orphans), pairs as lists of
    (first, last); raises Refused"""
    c = Collate()
    outs = [c.add(a) for a in adds]
    return outs, c.finish()


def pairs_bytes(pairs) -> bytes:
    return b"".join(a + b for a, b in pairs)
