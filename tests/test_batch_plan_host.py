"""The batch-list planner of wgcs_checksum_batches
(wireguard_amd/csrc/wgcs_batch_plan.h) as host code under AddressSanitizer +
UBSan (CPU only).

tests/batch_plan_host/batch_plan_host.cpp is a stand-alone program that
includes the header the library and the kernel include and checks, on random
lists of 0-100 batches (sizes around the block and the cap, outputs that are
disjoint, identical tuples, partially overlapping, nested or abutting), the
group boundaries against a per-byte ownership model of its own, the prefix
sums, the multiples of 8, the 32-batch cap, that every non-empty batch appears
exactly once and in order, and the lookup the kernel does on the table.  It
runs once as it is and once with WGCS_FUSE=0 in the environment."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "batch_plan_host", "batch_plan_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("batch_plan_host") / "batch_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", str(exe), SRC],
                   check=True, timeout=300)
    return str(exe)


@pytest.mark.parametrize("fuse", [None, "0", "1"])
def test_batch_plan_under_sanitizers(prog, fuse):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("WGCS_FUSE", None)
    if fuse is not None:
        env["WGCS_FUSE"] = fuse
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.split()[-2:] == ["batch_plan_host:", "ok"]
