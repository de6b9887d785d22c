"""The grouped candidate verify of d_index_at (scan_rowops.h), on the CPU
against tools/host_rowops/librowops.so: the result must equal Python's
bytes.find for every input, and no byte read of the verify may fall outside
the row.  h_dev_index_checked runs d_index_at over an accessor that records
out-of-row byte reads and reports them as -2.
"""

import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tools", "host_rowops", "librowops.so")

G = 4   # kVerifyGroup
LENS = list(range(1, 2 * G + 2)) + [15, 16, 17, 33]


@pytest.fixture(scope="module")
def index_checked():
    if not os.path.exists(LIB):
        pytest.skip("librowops.so not built (make rowops)")
    dev = ctypes.CDLL(LIB)
    fn = dev.h_dev_index_checked
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_char_p, ctypes.c_long, ctypes.c_long,
                   ctypes.c_char_p, ctypes.c_long]

    def call(row, align, pat):
        return fn(row, len(row), align, pat, len(pat))
    return call


def pattern(n):
    """n distinct-ish bytes; '#' and '.' never occur."""
    return bytes(ord("a") + (7 * i + i // 26) % 26 for i in range(n))


def rows_for(pat):
    n = len(pat)
    rows = [
        b"",
        pat,                                  # offset 0 and pos == last
        pat + b" tail",                       # offset 0
        b"head " + pat,                       # ends on the row's last byte
        b"." * 19 + pat,
        b"." * 40 + pat + b".",
        b"nothing here at all " * 3,
        pat[:-1],                             # shorter than the pattern
    ]
    for k in range(1, n):
        miss = pat[:k] + b"#"
        rows.append(miss + b"." * n)                  # near miss only
        rows.append(miss + pat)                       # near miss, then match
        rows.append(b"." * 13 + miss * 3 + pat)       # match on the last byte
        rows.append(pat[:k])                          # row ends inside
        rows.append(b"." * 7 + pat[:k])
    return rows


@pytest.mark.parametrize("n", LENS)
def test_verify_groups_against_find(index_checked, n):
    pat = pattern(n)
    checked = 0
    for row in rows_for(pat):
        want = row.find(pat)
        for align in range(16):
            got = index_checked(row, align, pat)
            assert got != -2, (
                f"verify read outside the row: n={n} align={align} row={row!r}")
            assert got == want, (
                f"n={n} align={align} row={row!r}: got {got} want {want}")
            checked += 1
    assert checked >= 16 * 8


def test_verify_groups_repeated_bytes(index_checked):
    """Patterns of one repeated byte: every position is a candidate."""
    for n in LENS:
        pat = b"a" * n
        for row in (b"a" * (n - 1) + b"b" + b"a" * n,
                    b"a" * (n - 1),
                    (b"a" * (n - 1) + b"b") * 3,
                    b"b" + b"a" * n):
            for align in (0, 5, 15):
                got = index_checked(row, align, pat)
                assert got == row.find(pat), (n, align, row)
