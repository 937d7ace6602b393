"""Builders shared by test_collate.py and test_gpu_collate.py: the hand cases of rules C1-C6 (include/bwams.h above
bwams_collate_open) with the outputs written out here, the cuts of a record list into adds, and small helpers over records."""
import struct

from test_markdup import P1, P2, R, rec

SUP, SEC = 0x800, 0x100

A1, A2 = rec(b"a", P1, 100), rec(b"a", P2 | R, 300)
B1, B2 = rec(b"b", P1 | R, 250), rec(b"b", P2, 120)
S1, S2 = rec(b"s", 0, 150), rec(b"t", R, 260)
A_SUP = rec(b"a", P1 | SUP, 200, b"30H20M")
A_SEC = rec(b"a", P2 | SEC, 210)
A1_AGAIN, A1_FAR = rec(b"a", P1, 900), rec(b"a", P1 | R, 5000)
BOTH, NEITHER = rec(b"x", 0x1 | 0x40 | 0x80, 400), rec(b"y", 0x1, 410)

# (case, adds as lists of records, the (pairs, singles) of each add, the orphans)
CASES = [
    ("mates_adjacent", [[A1, A2]], [([(A1, A2)], [])], []),
    ("mates_apart", [[A1, B2, S1, B1, S2, A2]], [([(B1, B2), (A1, A2)], [S1, S2])], []),            # by completing ordinal: b, then a
    ("mates_apart_two_adds", [[A1, B2, S1], [B1, S2, A2]], [([], [S1]), ([(B1, B2), (A1, A2)], [S2])], []),
    ("last_before_first", [[A2, A1]], [([(A1, A2)], [])], []),
    ("last_before_first_two_adds", [[A2], [A1]], [([], []), ([(A1, A2)], [])], []),
    ("single_between_mates", [[A1, S1, A2]], [([(A1, A2)], [S1])], []),
    ("supplementary_between_mates", [[A1, A_SUP, A_SEC, A2]], [([(A1, A2)], [])], []),
    ("supplementary_in_another_add", [[A1], [A_SUP], [A2]], [([], []), ([], []), ([(A1, A2)], [])], []),
    ("orphan", [[A1, B1, S1], [B2]], [([], [S1]), ([(B1, B2)], [])], [A1]),
    ("orphans_in_ordinal_order", [[B2, S1], [A2]], [([], [S1]), ([], [])], [B2, A2]),
    ("name_reused_after_its_pair", [[A1, A2, A1_AGAIN]], [([(A1, A2)], [])], [A1_AGAIN]),
    ("name_reused_in_a_later_add", [[A1, A2], [A1_AGAIN]], [([(A1, A2)], []), ([], [])], [A1_AGAIN]),
    ("nothing", [[]], [([], [])], []),
    ("only_skipped", [[A_SUP, A_SEC]], [([], [])], []),
]

# (case, adds, the add that is refused, the ordinal it names, the reason: 0 C2's bits, 1 C3's segment)
REFUSALS = [
    ("first_first_within_one_add", [[S1, A1, B1, A1_AGAIN, B2]], 0, 3, 1),
    ("first_first_at_a_distance", [[A1, S1], [B1], [S2, A1_FAR, A2]], 2, 4, 1),
    ("last_last", [[A2, A2]], 0, 1, 1),
    ("both_segment_bits", [[A1, BOTH, A2]], 0, 1, 0),
    ("neither_segment_bit", [[A1], [A2, S1, NEITHER]], 1, 3, 0),
    ("segment_fault_before_bits_fault", [[A1, A1_AGAIN, BOTH]], 0, 1, 1),                          # the smallest ordinal, whichever rule
    ("bits_fault_before_segment_fault", [[BOTH, A1, A1_AGAIN]], 0, 0, 0),
    ("skipped_records_have_ordinals", [[A_SUP, A_SEC, A1, A_SUP, A1_AGAIN]], 0, 4, 1),
]


def flag_of(r: bytes) -> int:
    return struct.unpack_from("<H", r, 18)[0]


def kept(r: bytes) -> bool:
    return not flag_of(r) & 0x900


def renamed(r: bytes, name: bytes) -> bytes:
    """record r with another read name (0 to 254 bytes): block_size and l_read_name follow"""
    old = r[12]
    body = r[4:12] + bytes([len(name) + 1]) + r[13:36] + name + b"\0" + r[36 + old:]
    return struct.pack("<I", len(body)) + body


def cuts(recs, how: str) -> list:
    """the records cut into adds: "one", "each", "thirds" (uneven) or "empty_middle" """
    n = len(recs)
    if how == "one":
        return [recs]
    if how == "each":
        return [[r] for r in recs]
    if how == "thirds":
        c0, c1 = n // 5, (2 * n) // 3
        return [recs[:c0], recs[c0:c1], recs[c1:]]
    assert how == "empty_middle"
    return [recs[:n // 2], [], recs[n // 2:]]


def joined(adds) -> list:
    return [b"".join(a) for a in adds]
