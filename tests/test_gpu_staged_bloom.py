"""Bloom gates decided at staging, and the grouped candidate verify, on the
GPU: bitmaps and hits must equal the CPU oracle's bit for bit.

Staging probes each gated leaf's token hashes against the block's bloom
filter on the host: a miss stages the leaf as all-false for that block (and
drops the block where the program allows), a hit stages it with no gate.  The
kernel sees no gate.  The cases live in tests/staged_bloom_cases.py and also
run through the emulation build (tests/test_emu_staged_bloom.py).
"""

import json

import pytest

from victorialogs_amd import write_custom_part

from tests import staged_bloom_cases as sbc
from tests.test_gpu_operand_cache import (ROWS, _write, assert_parity,
                                          make_phrase, phrase_f, verify_rows)

gpu = pytest.mark.gpu

VERIFY_GROUP = 4    # kVerifyGroup (scan_rowops.h)


@pytest.fixture(scope="module")
def bloom_part(tmp_path_factory):
    return sbc.build_part(write_custom_part,
                          str(tmp_path_factory.mktemp("stagedbloom") / "p"))


@gpu
@pytest.mark.parametrize("name", list(sbc.CASES))
def test_staged_bloom_gate(bloom_part, name):
    sbc.check_case(bloom_part, name)


# ---- grouped verify through a real scan ----

def padded(rows, width):
    """Non-empty rows shorter than `width` are filled up behind a space, so
    no match appears or disappears."""
    return [r + " " + "p" * (width - len(r) - 1)
            if r and len(r) < width - 1 else r for r in rows]


@gpu
@pytest.mark.parametrize("width", [260, 33], ids=["perword", "shortrow"])
@pytest.mark.parametrize("n", list(range(1, 2 * VERIFY_GROUP + 2)))
def test_verify_groups_scan(tmp_path_factory, n, width):
    """~260 B rows take the per-word tile loop, 33 B rows the short-row
    loop."""
    ph = make_phrase(n)
    rows = padded(verify_rows(ph), width)
    d = _write(tmp_path_factory, f"vg{n}_{width}", [("_msg", rows)])
    hits = assert_parity(d, json.dumps(phrase_f("_msg", ph)))
    assert 0 < hits < ROWS
