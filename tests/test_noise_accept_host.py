"""The responder's stateful tail of wireguard_amd/csrc/wgcs_noise.h (the row
functions noise_accept_claim, noise_accept_verdict, noise_accept_commit and
noise_accept_tail) and the host functions wgcs_handshake_accept_host /
wgcs_peer_rows_build of noise.cpp as host code under AddressSanitizer + UBSan
(CPU only).

tests/noise_accept_host/noise_accept_host.cpp is a stand-alone program that
includes the headers the kernels include and links noise.cpp as it is.  Every
table sits in a heap buffer of exactly its size -- the init rows end with the
batch, the peer rows with the table, the id map where n_ids says -- so a byte
read or written outside a row or a table is a sanitizer report, a gated row's
included: its verdict must come from the gate alone.  The batches are the named
cases of tests/noise_accept_cases.py, step by step; what the program prints is
compared with the library's host form, which tests/test_noise_accept_ref.py pins
to the restatement."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import noise_accept_cases as cases
from noise_accept_cases import FILL
from wireguard_amd import noise
from wireguard_amd.noise import HS_RESP_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "noise_accept_host", "noise_accept_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("noise_accept") / "noise_accept_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "noise.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "noise_accept_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def test_named_cases_row_functions_and_host_form(prog):
    lines, want = [], []
    for c in list(cases.named()) + [cases.wide()]:
        peers = c.peers
        for s in c.steps:
            p = peers.copy()
            verdict = np.full(len(s.init), -1, np.int32)
            resp = np.full(80 * len(s.tickets), FILL, np.uint8).view(HS_RESP_DTYPE)
            count = np.full(1, 0xEEEEEEEE, np.uint32)
            noise.accept_host(s.init, s.gate, s.now, c.table, c.peer_rows, p, s.tickets, resp, count, verdict)
            for how in ("row", "host"):
                lines.append(f"accept {how} {hx(s.init)} {hx(s.gate)} {struct.pack('<q', s.now).hex()} {hx(c.table)} "
                             f"{hx(c.peer_rows)} {hx(peers)} {hx(s.tickets)}")
                want.append([hx(verdict), hx(p), hx(resp), hx(count)])
            peers = p
    assert run(prog, lines) == want


def test_peer_rows_build(prog):
    table, rows, n_ids = cases.table_of(6)
    got = run(prog, [f"rows host {hx(table)} {struct.pack('<I', n_ids).hex()}",
                     f"rows host - {struct.pack('<I', 3).hex()}"])
    assert got == [[hx(rows)], ["ff" * 12]]
