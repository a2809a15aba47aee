"""The row functions of wireguard_amd/csrc/wgcs_keypairs.h (keypairs_begin,
keypairs_received_claim, keypairs_received_commit, delete_session and the
slot probe under them) and the host forms of keypairs.cpp as host code under
AddressSanitizer + UBSan (CPU only).

tests/keypairs_host/keypairs_host.cpp is a stand-alone program with its own
main that includes the header the kernels include and links keypairs.cpp as it
is.  Every table sits in a heap buffer of exactly its size -- the descriptors
end with the batch, the slot arrays with their last slot, the key table with
its last row -- so a byte read or written outside a row or a table is a
sanitizer report, a gated row's included: its status must come from the gate
alone.  The calls are the named cases of tests/keypairs_cases.py, step by step;
what the program prints is compared with the library's host form, which
tests/test_keypairs_ref.py pins to the restatement.  Nothing loaded into
Python is built with a sanitizer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import keypairs_cases as cases
from keypairs_cases import TABLES

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "keypairs_host", "keypairs_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("keypairs") / "keypairs_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "keypairs.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "keypairs_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def line_of(w, t, s, how) -> str:
    tail = " ".join(hx(t[k]) for k in TABLES)
    now = struct.pack("<q", getattr(s, "now", 0)).hex()
    if s.kind == "resp":
        return f"resp {how} {hx(s.resp)} {hx(s.gate)} {now} {hx(w.table)} {tail}"
    if s.kind == "init":
        return (f"init {how} {hx(s.arena)} {hx(s.pkts)} {hx(s.gate)} {now} {hx(w.hs_slots)} {hx(w.states)} "
                f"{hx(w.table)} {tail}")
    return f"recv {how} {hx(s.pkts)} {hx(s.verdict)} {hx(w.peer_rows)} {tail}"


def test_named_cases_row_functions_and_host_form(prog):
    lines, want = [], []
    for c in cases.named():
        w, t = c.world, cases.tables_of(c.world)
        for s in c.steps:
            before = {k: v.copy() for k, v in t.items()}
            out = cases.run_host(w, t, s)
            for how in ("row", "host"):
                lines.append(line_of(w, before, s, how))
                want.append([hx(out)] + [hx(t[k]) for k in TABLES])
    assert len(lines) > 60
    assert run(prog, lines) == want
