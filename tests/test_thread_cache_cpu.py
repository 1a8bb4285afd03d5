"""The bookkeeping of the calling thread's cached memory (csrc/thread_cache.h: the arena per device, the pinned block's growth rule, trim),
checked on the host: tests/cpp/thread_cache_check.cpp replaces the HIP allocation calls by malloc / free with a ledger, is compiled with
g++ against the header and the HIP headers (no HIP library is linked, no device is touched) and drives two instances from each of two
std::threads, twice over.  Once plainly, once under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "thread_cache_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_thread_cache_check(tmp_path, flags):
    exe = str(tmp_path / "thread_cache_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), *flags, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "thread_cache_check: ok" in r.stdout and "none live" in r.stdout
