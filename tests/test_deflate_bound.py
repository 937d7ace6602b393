"""bwams_deflate_bound (host arithmetic, no GPU): n + 31 per started 65280-byte member + the 28-byte EOF member."""
import pytest

from bwams import bgzf, capi


@pytest.mark.parametrize("n", [0, 1, 100, 65279, 65280, 65281, 2 * 65280, 3 * 65280, 3 * 65280 + 1, 1 << 30, (1 << 40) + 7])
def test_bound_is_the_formula(n):
    members = -(-n // bgzf.BLOCK)
    assert capi.deflate_bound(n) == n + 31 * members + 28


def test_bound_of_nothing_is_the_eof_member():
    assert capi.deflate_bound(0) == len(bgzf.EOF_MEMBER)
