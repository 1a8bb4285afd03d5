"""The packed model normal of the queue kernel's gate (csrc/normal_cone.h), checked on the host: tests/cpp/packed_normal_check.cpp is
compiled with g++ against the header alone and run -- the quantisation bound STOCS_MODEL_NORMAL_Q, the "no gate" flag, and the
soundness of the gate on the packed normal against the kernel's own float dot product (with a floor on how much it rules out), and the
two inequalities of the header's derivation asserted in double, because the spare room of the older margin m would hide a missing
s K from the sampled dot products: with STOCS_MODEL_NORMAL_SLACK set to 0 the program fails 499 555 checks, with Q / 2 58 537, and
with the term taken out of model_normal_gate_threshold alone 6 424; as shipped the quantisation uses up to 0.98 of s K.
Once plainly, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "packed_normal_check.cpp")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_packed_normal_check(tmp_path, flags):
    exe = str(tmp_path / "packed_normal_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", *flags, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "packed_normal_check: ok" in r.stdout
    m = re.search(r"gate: (\d+) trials, ruled out by the exact-normal gate (\d+), by the packed one (\d+)", r.stdout)
    assert m, r.stdout
    trials, exact, packed = (int(x) for x in m.groups())
    assert trials >= 1000000 and 5 * exact >= trials and 5 * packed >= trials
    m = re.search(r"margin: the packed normal moved the support function by at most ([0-9.]+) of s K", r.stdout)
    assert m and 0.5 < float(m.group(1)) <= 1.0, r.stdout
