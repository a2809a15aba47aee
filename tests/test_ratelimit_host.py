"""The row functions of wireguard_amd/csrc/wgcs_ratelimit.h (find or claim, the
positions, the cleanup row) and the host forms of ratelimit.cpp as host code
under AddressSanitizer + UBSan (CPU only).

tests/ratelimit_host/ratelimit_host.cpp is a stand-alone program with its own
main that includes the header the kernels include and links ratelimit.cpp as
it is.  Every table sits in a heap buffer of exactly n_slots rows and every row
array in one of exactly n rows, so a probe that does not wrap at the table's
end, or a look back or ahead past the first or last position, is a sanitizer
report.  The calls are written here; what the program prints is compared with
the library's host form, which tests/test_ratelimit_ref.py pins to the
restatement.  Nothing loaded into Python is built with a sanitizer."""
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from ratelimit_cases import COST, ERR_MAC1, HS_COOKIE, HS_PASS, SECOND, by_home, colliding, srcs
from wireguard_amd import _lib, ratelimit as rl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "ratelimit_host", "ratelimit_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("ratelimit") / "ratelimit_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "ratelimit.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "ratelimit_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def i64(v) -> bytes:
    return struct.pack("<q", v)


def sequences():
    """(table before, step) pairs with the library's answers: batches and cleanups over small tables."""
    rng = random.Random(99)
    for n_slots in (1, 2, 8, 64):
        homes = [n_slots - 1] * 3 + [rng.randrange(n_slots) for _ in range(min(n_slots, 12))]
        pool = [(ip, 3) for ip in by_home(n_slots, homes)] + [("fe80::1", 4), ("::ffff:10.0.0.1", 4)]
        tab, now = rl.table(n_slots), 5 * SECOND
        for step in range(14):
            now += rng.choice([0, COST - 1, COST, 4 * COST, SECOND, SECOND + 1])
            if step % 5 == 4:
                new, live = rl.cleanup_host(tab, now)
                yield ("clean", tab.copy(), now), [hx(struct.pack("<I", live)), hx(new)]
                tab = new
                continue
            rows = [rng.choice(pool) if rng.random() < 0.6 else pool[0] for _ in range(rng.choice([0, 1, 7, 30]))]
            s = srcs(rows)
            gate = np.array([HS_PASS if rng.random() < 0.9 else rng.choice([HS_COOKIE, ERR_MAC1]) for _ in rows], np.int32)
            if rows and step % 3 == 0:
                s["len"][rng.randrange(len(rows))] = 17
            before, stats = tab.copy(), np.zeros(4, np.uint32)
            v = rl.allow_host(gate, s, tab, now, stats=stats)
            yield ("batch", gate, s, before, now), [hx(v), hx(stats), hx(tab)]


def test_row_functions_and_host_forms(prog):
    lines, want = [], []
    for call, out in sequences():
        for how in ("row", "host"):
            lines.append(" ".join([call[0], how] + [hx(i64(x)) if isinstance(x, int) else hx(x) for x in call[1:]]))
            want.append(out)
    assert len(lines) > 100
    assert run(prog, lines) == want


def test_allow_and_home_slot(prog):
    L = _lib.load()
    tab, lines, want = rl.table(4), [], []
    pool = srcs([(ip, 1) for ip in colliding(4, 3, 5)] + [("fe80::2", 9)])
    for k in range(60):
        i = (k // 2) % 6 if k % 2 else 0  # every other call is the first address: it runs out of tokens
        s, now = pool[i:i + 1], SECOND + k * (COST // 3)
        lines.append(" ".join(["allow", "host", hx(s), hx(tab), hx(i64(now))]))
        rc = L.wgcs_ratelimit_allow(tab.ctypes.data, 4, s.ctypes.data, now)
        want.append([hx(struct.pack("<i", rc)), hx(tab)])
    assert {w[0] for w in want} == {hx(struct.pack("<i", c)) for c in (0, 1, rl.ERR_RATE_TABLE_FULL)}
    for n_slots in (1, 4, 1 << 24):
        for s in pool:
            lines.append(" ".join(["home", "host", hx(s), hx(struct.pack("<I", n_slots))]))
            want.append([hx(struct.pack("<I", rl.home_slot(s, n_slots)))])
    assert run(prog, lines) == want
