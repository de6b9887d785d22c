"""The staging-time bloom gate cases (tests/staged_bloom_cases.py) through
the CPU emulation build: real filter compile and real staging, so the host
gate decision, the block elimination and the arena rollback are tested
without a GPU."""

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tools", "host_emu", "libvlogsql_emu.so")

pytestmark = pytest.mark.skipif(not os.path.exists(EMU),
                                reason="emu lib not built (make emu)")


def test_emu_staged_bloom_cases():
    """One subprocess for all cases: the product library is cached per
    process, so the emulation build needs a process of its own."""
    code = """
import sys, tempfile, os
sys.path.insert(0, ".")
from victorialogs_amd import write_custom_part
from tests import staged_bloom_cases as sbc
d = sbc.build_part(write_custom_part, os.path.join(tempfile.mkdtemp(), "p"))
for name in sbc.CASES:
    print(name, sbc.check_case(d, name), flush=True)
print("emu staged bloom OK", len(sbc.CASES))
"""
    env = dict(os.environ, VQL_LIB=EMU)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + "\n" + r.stderr[-4000:]
    assert "emu staged bloom OK" in r.stdout
