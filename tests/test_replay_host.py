"""The scalar replay filter (wireguard_amd/csrc/wgcs_replay.h) as host code
under AddressSanitizer + UBSan (CPU only).

tests/replay_host/replay_host.cpp is a stand-alone program that includes the
header the library and the kernels include and runs its validate against two
brute-force models of its own: a flag per ring value that starts from any
filter's bytes, and a set of accepted values for filters that start empty.
Every filter is a heap block of exactly 1,032 bytes and starts all-zero,
all-ones or random, so an index that leaves the ring is a sanitizer report."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "replay_host", "replay_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("replay_host") / "replay_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", str(exe), SRC, "-lpthread"],
                   check=True, timeout=300)
    return str(exe)


def test_replay_filter_under_sanitizers(prog):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.split()[-2:] == ["replay_host:", "ok"]
