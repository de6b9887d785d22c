"""Shared part and filter cases for the staging-time bloom gate tests
(tests/test_gpu_staged_bloom.py on the GPU, tests/test_emu_staged_bloom.py
through the CPU emulation build).  Not a test module.

The part has three blocks of 8192+65 rows (two chunks each, ragged last
word).  The token `needleword` occurs in blocks 0 and 2 and nowhere in block
1, so a leaf gated on it misses block 1's bloom filter.
"""

import json

from victorialogs_amd import Filter, OracleScanner, Part, Stage

ROWS = 8192 + 65
NBLOCKS = 3
TOKEN_BLOCKS = (0, 2)


def _ts(n, b):
    return [1700000000000000000 + b * 10**9 + i * 1000 for i in range(n)]


def block_columns(b):
    word = "needleword" if b in TOKEN_BLOCKS else "haystack"
    s, punct = [], []
    for i in range(ROWS):
        k = i % 4
        if k == 0:
            s.append(f"{i} qq {word} zz tail")
        elif k == 1:
            s.append(f"{word} exact")
        elif k == 2:
            s.append(f"{word} start {i}")
        else:
            s.append(f"{i} other")
        # no token in any value: the column's bloom filter has no words
        punct.append("!" * (i % 40) + "-" * (i % 3))
    return [
        {"name": "s", "values": s},
        {"name": "punct", "values": punct},
        {"name": "empty", "values": [""] * ROWS},
    ]


def build_part(write_custom_part, part_dir):
    write_custom_part(part_dir, {"blocks": [
        {"stream": 0, "timestamps": _ts(ROWS, b), "columns": block_columns(b)}
        for b in range(NBLOCKS)]})
    return part_dir


def phrase_f(field, phrase):
    return {"type": "phrase", "field": field, "phrase": phrase}


def or_f(*fs):
    return {"type": "or", "filters": list(fs)}


def and_f(*fs):
    return {"type": "and", "filters": list(fs)}


# name -> (filter, live blocks expected of Stage.live_rows, or None)
CASES = {
    "phrase": (phrase_f("s", "needleword"), TOKEN_BLOCKS),
    "regexp": ({"type": "regexp", "field": "s", "re": "qq needleword zz"},
               TOKEN_BLOCKS),
    "prefix": ({"type": "prefix", "field": "s", "prefix": "needleword sta"},
               TOKEN_BLOCKS),
    "exact": ({"type": "exact", "field": "s", "value": "needleword exact"},
              TOKEN_BLOCKS),
    # block 1 stays live under the negation and is all ones
    "not_phrase": ({"type": "not", "filter": phrase_f("s", "needleword")},
                   (0, 1, 2)),
    # the former fused-pair fallback: same column, one gate misses in block 1
    "or_pair": (or_f(phrase_f("s", "other"), phrase_f("s", "needleword")),
                (0, 1, 2)),
    "or_pair_swapped": (or_f(phrase_f("s", "needleword"),
                             phrase_f("s", "other")), (0, 1, 2)),
    "and_pair": (and_f(phrase_f("s", "tail"), phrase_f("s", "needleword")),
                 TOKEN_BLOCKS),
    "and_not_pair": (and_f(phrase_f("s", "other"),
                           {"type": "not",
                            "filter": phrase_f("s", "needleword")}),
                     (0, 1, 2)),
    # empty bloom filter: the gate passes whatever the hashes are
    "punct_tokens": (phrase_f("punct", "needleword"), (0, 1, 2)),
    "punct_no_tokens": (phrase_f("punct", "!!!"), (0, 1, 2)),
    "empty_phrase": (phrase_f("empty", "needleword"), None),
    "empty_exact": ({"type": "exact", "field": "empty", "value": ""}, None),
}


def check_case(part_dir, name):
    """GPU (or emulation) hits and bitmaps against the oracle, bit for bit,
    and the blocks that staging kept live."""
    f, live_blocks = CASES[name]
    fjson = json.dumps(f)
    part = Part(part_dir)
    filt = Filter(fjson)
    st = Stage(part, filt, device=0)
    orc = OracleScanner(part_dir)
    try:
        assert part.blocks == NBLOCKS
        hits = st.scan()
        nwords = sum((part.block_rows(i) + 63) // 64 for i in range(NBLOCKS))
        bits = st.fetch_bitmaps(nwords)
        orc_hits, orc_bits = orc.scan(fjson, with_bitmaps=True)
        assert hits == orc_hits, f"{name}: hits {hits} oracle {orc_hits}"
        assert bits == orc_bits, f"{name}: bitmap mismatch"
        if live_blocks is not None:
            assert st.live_rows == ROWS * len(live_blocks), (
                f"{name}: live_rows {st.live_rows}")
        if name == "not_phrase":
            wpb = (ROWS + 63) // 64
            blk1 = bits[wpb * 8:2 * wpb * 8]
            want = (1 << ROWS) - 1
            assert int.from_bytes(blk1, "little") == want
        if name in ("phrase", "regexp", "prefix", "exact", "or_pair",
                    "and_pair"):
            assert 0 < hits < ROWS * NBLOCKS
        return hits
    finally:
        orc.close()
        st.close()
        filt.close()
        part.close()
