"""bench.py's plain-run contract: a run without --full does only the
headline legs, and --dump-outputs writes what the last timed step computed
(hits, per-block hits, result bitmaps) identically from run to run.

The CPU test drives the emulated product pipeline (tools/host_emu); the GPU
test drives the real HIP library on the same small fixture."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "host_emu", "libvlogsql_emu.so")

ROWS = 200_000
NAMES = ["hits", "block_hits", "bitmaps"]


def run_bench(data_dir, out_dir, env_extra):
    env = dict(os.environ, VQL_DATA_DIR=str(data_dir), **env_extra)
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--rows", str(ROWS),
         "--steps", "3", "--warmup", "1", "--workload", "phrase_selective",
         "--dump-outputs", str(out_dir)],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    arrays = {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}
    return line, arrays


def expected_matches(data_dir):
    """The generator's own count of "ip=77." rows, summed over the parts."""
    total = 0
    rank_dir = os.path.join(data_dir, "rank0")
    for d in os.listdir(rank_dir):
        with open(os.path.join(rank_dir, d, "gen_manifest.json")) as f:
            total += json.load(f)["sel_msg_ip77"]
    return total


def check_outputs(line, arrays, data_dir):
    # a plain run leaves the legs behind --full out, and says so
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert line["selectivity_check"] is None
    assert line["cpu_baseline"] is None

    hits, block_hits, bitmaps = (arrays[n] for n in NAMES)
    assert hits.dtype == np.float64 and block_hits.dtype == np.float64
    assert bitmaps.dtype == np.float32
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20

    expected = expected_matches(data_dir)
    assert 0 < expected < ROWS
    assert hits.sum() == expected == line["config"]["matched_rows_per_pass"]
    assert block_hits.sum() == expected

    # bitmaps: 16 bits per value, one bitmap per block padded to 64-bit
    # words; per-block popcounts must equal block_hits, and no bit may be
    # set past a block's last row
    nparts = len(os.listdir(os.path.join(data_dir, "rank0")))
    block_rows = []
    for i in range(nparts):
        # the last part takes the remainder, as in bench.prepare_parts
        left = ROWS // nparts + (ROWS % nparts if i == nparts - 1 else 0)
        while left:
            block_rows.append(min(8192, left))
            left -= block_rows[-1]
    assert len(block_rows) == block_hits.size
    assert bitmaps.size == sum((n + 63) // 64 * 4 for n in block_rows)
    bits = np.unpackbits(bitmaps.astype("<u2").view(np.uint8),
                         bitorder="little")
    pos = 0
    for n, want in zip(block_rows, block_hits):
        padded = (n + 63) // 64 * 64
        assert bits[pos:pos + n].sum() == want
        assert not bits[pos + n:pos + padded].any()
        pos += padded


@pytest.mark.skipif(not os.path.exists(EMU),
                    reason="emu lib not built (make emu)")
def test_bench_dump_outputs_emu(tmp_path):
    data = tmp_path / "data"
    line, first = run_bench(data, tmp_path / "out1", {"VQL_LIB": EMU})
    check_outputs(line, first, str(data))
    # same arguments => identical inputs and outputs
    _, second = run_bench(data, tmp_path / "out2", {"VQL_LIB": EMU})
    for n in NAMES:
        assert np.array_equal(first[n], second[n]), n


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(tmp_path):
    data = tmp_path / "data"
    line, arrays = run_bench(data, tmp_path / "out", {})
    check_outputs(line, arrays, str(data))
