"""Scan-kernel operand cache, literal-regexp routing and short-row
super-group choice: GPU bitmaps must equal the CPU oracle's bit for bit.

The kernel keeps a leaf's pattern bytes in an LDS slot of
kOperandSlotBytes (scan_types.h), refilled per chunk and per leaf; literal
regexps take the phrase clone; the short-row loop's super-group size `sg` is
picked at staging from the block's actual byte spans.  Every part here is one
block of a little more than one chunk (8192 rows), so the slot is filled
twice and the last bitmap word is ragged.
"""

import json

import pytest

from victorialogs_amd import (Filter, OracleScanner, Part, Stage,
                              write_custom_part)

SLOT = 512          # kOperandSlotBytes
TILE = 17408        # kWaveTileBytes
ROWS = 8192 + 65    # two chunks, ragged last word
SG_ROWS = 8192 + 512 + 65

gpu = pytest.mark.gpu


def assert_parity(part_dir, fjson, lo=0, hi=-1):
    """Copy of tests/test_gpu_parity.py::assert_parity; returns the hits."""
    part = Part(part_dir)
    filt = Filter(fjson)
    st = Stage(part, filt, device=0, lo=lo, hi=hi)
    try:
        gpu_hits = st.scan()
        hi_eff = part.blocks if hi < 0 else hi
        nwords = sum((part.block_rows(i) + 63) // 64 for i in range(lo, hi_eff))
        gpu_bits = st.fetch_bitmaps(nwords)

        orc = OracleScanner(part_dir)
        try:
            orc_hits, orc_bits = orc.scan(fjson, lo=lo, hi=hi, with_bitmaps=True)
        finally:
            orc.close()

        assert gpu_hits == orc_hits, (
            f"hits mismatch for {fjson}: gpu={gpu_hits} oracle={orc_hits}")
        if gpu_bits != orc_bits:
            for i in range(0, len(gpu_bits), 8):
                if gpu_bits[i:i + 8] != orc_bits[i:i + 8]:
                    raise AssertionError(
                        f"bitmap mismatch for {fjson} at word {i // 8}: "
                        f"gpu={gpu_bits[i:i+8].hex()} oracle={orc_bits[i:i+8].hex()}")
            raise AssertionError(f"bitmap length mismatch for {fjson}")
        return gpu_hits
    finally:
        st.close()
        filt.close()
        part.close()


def _ts(n):
    return [1700000000000000000 + i * 1000 for i in range(n)]


def _write(tmp_path_factory, name, columns):
    d = str(tmp_path_factory.mktemp("opcache") / name)
    n = len(columns[0][1])
    write_custom_part(d, {"blocks": [{
        "stream": 0, "timestamps": _ts(n),
        "columns": [{"name": c, "values": v} for c, v in columns]}]})
    return d


def phrase_f(field, phrase):
    return {"type": "phrase", "field": field, "phrase": phrase}


def regexp_f(field, re):
    return {"type": "regexp", "field": field, "re": re}


def and_f(*fs):
    return {"type": "and", "filters": list(fs)}


def or_f(*fs):
    return {"type": "or", "filters": list(fs)}


def not_f(f):
    return {"type": "not", "filter": f}


# ---- verify loop ----

def make_phrase(n):
    """n bytes of space-separated words; first and last byte are letters and
    '#' never occurs."""
    s = ""
    i = 0
    while len(s) < n:
        s += f"w{i}q "
        i += 1
    s = s[:n]
    if s[-1] == " ":
        s = s[:-1] + "e"
    return s


def verify_rows(ph):
    """Rows holding the phrase at offset 0, at the very end, after a run of
    near misses, or nowhere; rows sharing the phrase's first k bytes and then
    differing, for every k in 1..len-1 (all at least as long as the phrase,
    so the verify loop is reached); empty rows."""
    n = len(ph)
    base = [
        lambda i: f"{ph} tail {i}",
        lambda i: f"{i} head {ph}",
        lambda i: f"{i} nothing to see here " + "z" * (n % 40),
        lambda i: "" if i % 2 else f"{i}",
        lambda i: f"{i} {ph[:max(1, n // 2)]}# {ph[:max(1, n - 1)]}# {ph}",
        lambda i: f"{i} {ph[:max(1, n - 1)]}# " + "y" * n,
    ]
    rows = []
    i = 0
    cycle = 0
    while len(rows) < ROWS:
        for mk in base:
            rows.append(mk(i))
            i += 1
        # long phrases: a stride of near-miss prefixes per cycle keeps the
        # part small; 37 cycles (of ~20 rows) cover every k in 1..n-1
        ks = range(1, n) if n <= 17 else range(1 + cycle % 37, n, 37)
        cycle += 1
        for k in ks:
            rows.append(f"{ph[:k]}#{i} " + "x" * n)
            i += 1
    return rows[:ROWS]


VERIFY_LENS = [1, 2, 15, 16, 17, SLOT - 1, SLOT, SLOT + 1]


@gpu
@pytest.mark.parametrize("n", VERIFY_LENS)
def test_verify_loop_phrase_lengths(tmp_path_factory, n):
    """The last length takes the generic clone (operand in global memory)."""
    ph = make_phrase(n)
    rows = verify_rows(ph)
    if n > 17:
        seen = {k for k in range(1, n)
                if any(r.startswith(ph[:k] + "#") for r in rows)}
        assert seen == set(range(1, n))
    d = _write(tmp_path_factory, f"verify{n}", [("_msg", rows)])
    hits = assert_parity(d, json.dumps(phrase_f("_msg", ph)))
    assert 0 < hits < ROWS


# ---- stale-slot reuse ----

PA, PB, PC = "alpha one", "bravo two", "charlie three"


@pytest.fixture(scope="module")
def two_col_part(tmp_path_factory):
    """Both columns hold every phrase on different rows, so evaluating a
    leaf with another leaf's operand changes the result."""
    a, b = [], []
    for i in range(ROWS):
        pad = "p" * (150 + i % 9)
        a.append(f"{i} {[PA, PB, PC, 'none'][i % 4]} mid "
                 f"{[PC, 'zip', PA, PB, 'zap'][i % 5]} {pad}")
        b.append(f"{i} {[PB, PC, 'none', PA, PA][i % 5]} mid "
                 f"{[PA, 'zip', PC][i % 3]} {pad}")
    return _write(tmp_path_factory, "twocol", [("_msg", a), ("colb", b)])


STALE_TREES = [
    and_f(phrase_f("_msg", PA), phrase_f("colb", PB)),
    or_f(phrase_f("_msg", PA), phrase_f("colb", PB)),
    and_f(phrase_f("_msg", PA), not_f(phrase_f("colb", PB))),
    or_f(not_f(phrase_f("_msg", PA)), phrase_f("colb", PA)),
    not_f(or_f(phrase_f("colb", PC), phrase_f("_msg", PB))),
    and_f(phrase_f("_msg", PA), phrase_f("colb", PB), phrase_f("_msg", PC)),
    or_f(phrase_f("_msg", PA), phrase_f("colb", PB), phrase_f("_msg", PC)),
    or_f(and_f(phrase_f("_msg", PA), phrase_f("colb", PB)),
         not_f(phrase_f("colb", PC))),
    and_f(or_f(phrase_f("colb", PA), phrase_f("_msg", PB)),
          not_f(phrase_f("_msg", PC))),
    # fused same-column pairs; the absent token makes a bloom gate miss
    or_f(phrase_f("_msg", PA), phrase_f("_msg", PB)),
    and_f(phrase_f("colb", PA), not_f(phrase_f("colb", PB))),
    or_f(phrase_f("_msg", "absenttoken one"), phrase_f("_msg", PB)),
    or_f(phrase_f("_msg", PA), phrase_f("_msg", "bravo absenttoken")),
    or_f(phrase_f("_msg", "absenttoken one"), phrase_f("_msg", PB),
         phrase_f("colb", PC)),
    and_f(not_f(phrase_f("_msg", PA)),
          not_f(phrase_f("_msg", "bravo absenttoken"))),
]


@gpu
@pytest.mark.parametrize("tree", STALE_TREES,
                         ids=[f"tree{i}" for i in range(len(STALE_TREES))])
def test_stale_slot_trees(two_col_part, tree):
    hits = assert_parity(two_col_part, json.dumps(tree))
    assert 0 < hits < ROWS


# ---- headline shape in small ----

@pytest.fixture(scope="module")
def headline_part(tmp_path_factory):
    """_msg ~256 B rows (per-word loop), var_0 30-33 B rows (short-row
    loop)."""
    msg, var = [], []
    for i in range(ROWS):
        m = (f"{i} message for the stream {i % 7} "
             if i % 5 else f"{i} message for a stream {i % 7} ")
        msg.append(m + "f" * (250 + i % 11 - len(m)))
        v = "some value " if i % 3 else "some valve "
        var.append(v + f"{i:04d}" + "0" * (15 + i % 4))
    assert all(30 <= len(v) <= 33 for v in var)
    return _write(tmp_path_factory, "headline", [("_msg", msg), ("var_0", var)])


@gpu
def test_headline_shape(headline_part):
    f = and_f(phrase_f("_msg", "message for the stream"),
              regexp_f("var_0", "some value"))
    hits = assert_parity(headline_part, json.dumps(f))
    assert 0 < hits < ROWS
    assert_parity(headline_part,
                  json.dumps(regexp_f("var_0", "some value")))
    assert_parity(headline_part,
                  json.dumps(phrase_f("var_0", "some value")))


# ---- regexp routing ----

LONG_LIT = ("long literal " * 41)[:SLOT + 9]

REGEXPS = [
    "some value",
    "a",
    r"a\.b",
    LONG_LIT,
    "some value$",
    "^some",
    "(?i)some",
    "some|value",
    "some.*value",
    "",
]


def regexp_rows(pad):
    variants = [
        "some value here", "here some value", "Some Value", "value then some",
        "xx a.b yy", "xx axb yy", "some", "^some value$", "b.c", "nothing",
        "", "SOME", "valu", "some  value",
    ]
    rows = []
    for i in range(ROWS):
        v = variants[i % len(variants)]
        rows.append(f"{v} {i}{pad}" if i % 29 else v)
    return rows


@pytest.fixture(scope="module")
def regexp_part(tmp_path_factory):
    """`wide` takes the per-word loop (~170 B rows, a few hold the long
    literal), `narrow` the short-row loop."""
    wide = regexp_rows(" " + "q" * 150)
    for i in range(7, ROWS, 1000):
        wide[i] = f"{i} {LONG_LIT} end"
        wide[i + 1] = f"{i} {LONG_LIT[:-1]}# end"
    narrow = regexp_rows("")
    return _write(tmp_path_factory, "regexp",
                  [("wide", wide), ("narrow", narrow)])


@gpu
@pytest.mark.parametrize("re", REGEXPS, ids=lambda r: repr(r)[:24])
def test_regexp_routing_string_column(regexp_part, re):
    assert_parity(regexp_part, json.dumps(regexp_f("wide", re)))


@gpu
@pytest.mark.parametrize("re", ["some value", r"a\.b"])
def test_regexp_routing_short_rows(regexp_part, re):
    hits = assert_parity(regexp_part, json.dumps(regexp_f("narrow", re)))
    assert 0 < hits < ROWS


# ---- sg choice ----

def pick_sg(lengths):
    """The staging rule: largest sg in {8,4,2} whose overflowing
    super-groups (16-byte-aligned span above the tile) number at most
    max(1, nsg/32); else 1.  Returns (sg, overflowing super-groups)."""
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + n)
    rows = len(lengths)
    nwords = (rows + 63) // 64
    for sg in (8, 4, 2):
        nsg = (nwords + sg - 1) // sg
        over = 0
        for g in range(nsg):
            ra = g * sg * 64
            rb = min(rows, ra + sg * 64)
            if offs[rb] - (offs[ra] & ~15) > TILE:
                over += 1
        if over <= max(1, nsg // 32):
            return sg, over
    return 1, 0


def sg_rows(width, long_len=0):
    rows = []
    for i in range(SG_ROWS):
        s = f"{i:05d} " + ("some value " if i % 3 else "other thing ")
        rows.append((s + "x" * width)[:width])
    if long_len:
        rows[4000] = "y" * (long_len - 11) + " some value"
    return rows


# name -> (rows, intended sg, intended overflowing super-groups)
SG_CASES = {
    "fixed34": (sg_rows(34), 8, 0),      # 512 x 34 = 17408: fits exactly
    "fixed35": (sg_rows(35), 4, 0),      # overflows at 8
    "fixed20": (sg_rows(20), 8, 0),
    "fixed60": (sg_rows(60), 4, 0),
    "fixed130": (sg_rows(130), 2, 0),
    # 512 x 33 + 167 = 17063 still fits the tile: no fallback at this size
    "one200": (sg_rows(33, 200), 8, 0),
    # 512 x 33 + 567 = 17463: one super-group overflows at 8 and falls back
    "one600": (sg_rows(33, 600), 8, 1),
    # a row longer than the tile overflows its super-group at every sg
    "one30000": (sg_rows(33, 30000), 8, 1),
}


def test_sg_cases_land_as_intended():
    """CPU check of the shapes above against the staging rule."""
    for name, (rows, want_sg, want_over) in SG_CASES.items():
        assert pick_sg([len(r) for r in rows]) == (want_sg, want_over), name


@gpu
@pytest.mark.parametrize("name", list(SG_CASES))
def test_sg_choice(tmp_path_factory, name):
    rows = SG_CASES[name][0]
    d = _write(tmp_path_factory, name, [("_msg", rows)])
    for f in (phrase_f("_msg", "some value"), regexp_f("_msg", "some value"),
              regexp_f("_msg", "some.*x")):
        hits = assert_parity(d, json.dumps(f))
        assert 0 < hits < SG_ROWS
