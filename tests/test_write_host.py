"""The scalar Write-call rule (wireguard_amd/csrc/wgcs_write_plan.h) as host
code under AddressSanitizer + UBSan (CPU only).

tests/write_host/write_host.cpp is a stand-alone program that includes the
header the library and the kernel include and checks write_plan_batch, table
for table, against a model of its own that sorts (peer, row) pairs instead of
walking the rows.  Every input and output array is a heap block of exactly its
size and every output starts as a marker, so a row touched outside a batch's
share, or left out inside it, is a sanitizer report or a difference."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "write_host", "write_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("write_host") / "write_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", str(exe), SRC, "-lpthread"],
                   check=True, timeout=300)
    return str(exe)


def test_write_plan_under_sanitizers(prog):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.split()[-2:] == ["write_host:", "ok"]
