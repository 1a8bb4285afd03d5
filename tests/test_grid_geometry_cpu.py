"""The host geometry of the scene grid (csrc/grid_geometry.h) without a GPU: tests/cpp/grid_geometry_check.cpp includes that header
alone, is compiled with g++ under the address and undefined-behaviour sanitizers and run directly (a stand-alone program: nothing is
preloaded).  It is fed the centred bounding box and epsilon of every case of grid_cases.py at each of the case's cell edges, and what
it prints -- the float origin, h, inv_h, the cells and the bricks per axis: the quantities check_info compares on the GPU
(test_grid_forms_gpu.py) -- has to equal grid_ref.geometry bit for bit; so do the inclusion radius and the pad behind them.  The
extent cases are the ones whose radius follows the 2^-21 * span rule."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grid_cases as cases  # noqa: E402
import grid_ref as ref  # noqa: E402

SRC = os.path.join(HERE, "cpp", "grid_geometry_check.cpp")
F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grid_geometry") / "grid_geometry_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, SRC])
    return out


def bits(x):
    return int(np.asarray(x, F).view(np.uint32))


def test_the_margin_cases_are_there():
    assert "extent_rod" in cases.NAMES and "extent_max" in cases.NAMES


@pytest.mark.parametrize("name", cases.NAMES)
def test_geometry_matches_the_reference_bit_for_bit(exe, name):
    case = cases.build(name)
    spos, _ = ref.centre(case["spos"])
    p = spos.astype(np.float64)
    mn, mx, eps = p.min(0), p.max(0), float(F(case["eps"]))
    divs = tuple(case["divs"])
    lines = "".join(" ".join([float(v).hex() for v in (*mn, *mx, eps)] + [str(d)]) + "\n" for d in divs)
    r = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    rows = r.stdout.split("\n")[:-1]
    assert len(rows) == len(divs), r.stdout
    for d, row in zip(divs, rows):
        w = row.split()
        g = ref.geometry(spos, case["eps"], d)
        got = dict(origin=[int(x, 16) for x in w[0:3]], h=int(w[3], 16), inv_h=int(w[4], 16), cells=tuple(int(x) for x in w[5:8]),
                   bricks=tuple(int(x) for x in w[8:11]), r=float.fromhex(w[11]), pad=float.fromhex(w[12]))
        want = dict(origin=[bits(v) for v in g["origin"]], h=bits(g["h"]), inv_h=bits(g["inv_h"]), cells=g["cells"], bricks=g["bricks"], r=g["r"], pad=g["pad"])
        assert got == want, (name, d, got, want)
        # the prune slack and the key width, by their definitions (grid.hip: the widened cell box, the octant box inside it)
        hh, margin, oct_hw, cell_bits = float.fromhex(w[13]), float.fromhex(w[14]), float.fromhex(w[15]), int(w[16])
        h = g["h64"]
        side = max(n * h for n in g["cells"])
        assert hh == 0.5 * h + 2.0e-6 * (side + 1.0) * 0.5 + 1.0e-7 and margin == 4.0e-6 * (g["r"] + 2.0 * h) * (g["r"] + 2.0 * h)
        assert oct_hw == 0.25 * h + (hh - 0.5 * h) and hh > 0.5 * h and oct_hw > 0.25 * h
        n_top = math.prod(g["bricks"])
        assert 2 ** cell_bits >= n_top * 512 and (cell_bits == 1 or 2 ** (cell_bits - 1) < n_top * 512)
    if name in ("extent_rod", "extent_max"):      # the extent-aware margin is what these two exercise
        assert all(ref.geometry(spos, case["eps"], d)["r"] > eps * 1.001 for d in divs), name
