"""The checksum kernel's per-packet plan (wireguard_amd/csrc/wgcs_cs_plan.h) as
host code under AddressSanitizer + UBSan (CPU only).

tests/cs_plan_host/cs_plan_host.cpp is a stand-alone program that includes the
header the kernel includes and walks packets exactly as a row of lanes does:
edge chunks with their masks, interior chunks slot by slot, the per-lane folds,
the parity swap and the pseudo-header term.  It compares the 16-bit result
with a per-byte RFC 1071 sum of its own, for all five modes, every length 0-200
and 1,400-1,520 at every alignment 0-127 with a 16- and a 128-byte chunk grid
origin, IPv4 and IPv6, csum_start equal to, below and above the length, header
lengths 20 / 24 and 40 / 48, odd csum_start, and the checksum field in the
first, a middle and the last chunk and past the end; and checks that every
chunk it reads lies inside the packet's chunk grid and is read once."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cs_plan_host", "cs_plan_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("cs_plan_host") / "cs_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", str(exe), SRC],
                   check=True, timeout=300)
    return str(exe)


def test_cs_plan_under_sanitizers(prog):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.split()[-2:] == ["cs_plan_host:", "ok"]
