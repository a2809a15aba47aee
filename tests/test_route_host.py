"""The host router (wireguard_amd/csrc/router.cpp) and the image walk that the
kernels share with it (wgcs_route_walk.h) as host code under AddressSanitizer +
UBSan (CPU only).

tests/route_host/route_host.cpp is a stand-alone program that compiles
router.cpp, and with it the walk header the kernels include.  It repeats the
random insert / remove run against a brute-force match of its own, then walks
damaged images -- truncated at every length, every word overwritten with
hostile values, child indices at and past the node count, nodes that are their
own children, a bad magic -- each in a heap block of exactly its size, and
looks sessions up in built slot arrays.  Every call must return a peer,
WGCS_PEER_NONE or WGCS_ERR_INVALID_ARG with no sanitizer report.  This is the
only place a damaged image is walked: none goes to a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "route_host", "route_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("route_host") / "route_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", str(exe), SRC, "-lpthread"],
                   check=True, timeout=300)
    return str(exe)


def test_router_and_walk_under_sanitizers(prog):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
    assert p.stdout.split()[-2:] == ["route_host:", "ok"]
