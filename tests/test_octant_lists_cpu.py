"""The octant lines of the scene grid (csrc/octant_lists.h), checked on the host: tests/cpp/octant_lists_check.cpp is compiled with g++
against the header alone and run.  It round-trips the flag of the flat-table word, and for 300 cells (random surface patches and exact
lattices with duplicates, through the cell or beside it) prunes the cell's stored list per octant with the header's own code and asks
10^4 positions per cell -- a third of them on the octant planes or one float next to them, placed by the kernel's float floor -- whether
the nearest scene point under the product's tie rule, found by a scan over every point, is the answer of the position's octant line.
Once plainly, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "octant_lists_check.cpp")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_octant_lists_check(tmp_path, flags):
    exe = str(tmp_path / "octant_lists_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *flags, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "octant_lists_check: ok" in r.stdout
    m = re.search(r"cells (\d+) \(long (\d+)\), stored entries per cell ([0-9.]+), octants (\d+), fitting a line (\d+), entries per fitting line ([0-9.]+)", r.stdout)
    assert m, r.stdout
    cells, long_cells, fit, per_line = int(m.group(1)), int(m.group(2)), int(m.group(5)), float(m.group(6))
    assert cells >= 300 and long_cells >= 100 and fit >= 800 and 1.0 <= per_line < 8.0
    m = re.search(r"positions checked (\d+) \(on or next to an octant plane (\d+)\)", r.stdout)
    assert m and int(m.group(1)) >= 1000000 and int(m.group(2)) >= 200000, r.stdout
