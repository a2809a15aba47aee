"""The bodies and row functions of wireguard_amd/csrc/wgcs_rekey.h (RekeyRecvGate,
RekeySendGate, RekeySent, RekeyReceived, RekeyResponded and the three
passes of the start call) and the host forms of rekey.cpp as host code under
AddressSanitizer + UBSan (CPU only).

tests/rekey_host/rekey_host.cpp is a stand-alone program with its own main
that includes the header the kernels include and links rekey.cpp as it is.
Every table sits in a heap buffer of exactly its size -- the jobs end with the
batch, the keypairs and the wgcs_rekey rows with their last peer, the nonces
with the last key row, the descriptors with the last ticket -- so a byte read
or written outside a row or a table is a sanitizer report.  The calls are the
named cases of tests/rekey_cases.py, step by step; what the program prints is
compared with the library's host form, which tests/test_rekey_ref.py pins to
the restatement.  Nothing loaded into Python is built with a sanitizer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rekey_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "rekey_host", "rekey_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("rekey") / "rekey_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "rekey.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "rekey_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def line_of(w, st, s, how) -> str:
    now, u4, u8 = struct.pack("<q", s.now), lambda v: struct.pack("<I", v), lambda v: struct.pack("<Q", v)  # noqa: E731
    if s.kind == "recv":
        f = [s.pkts, now, st.key_peer, w.peer_rows, st.kp]
    elif s.kind == "gate":
        f = [s.peer, s.count, s.status_in, u4(s.max_segs), now, w.peer_rows, st.kp, st.send_nonce, u8(s.limit), st.rekey]
    elif s.kind == "sent":
        f = [s.peer, s.count, s.status, s.job_key, u4(s.max_segs), now, w.peer_rows, st.kp, st.send_nonce, u8(s.limit),
             st.rekey]
    elif s.kind == "rcvd":
        f = [s.groups, u4(s.calls_per_batch), now, w.peer_rows, st.kp, st.rekey]
    elif s.kind == "resp":
        f = [s.resp, s.gate, now, st.rekey]
    else:
        f = [now, st.rekey, st.hs_peers, s.tickets]
    return " ".join([s.kind, how] + [hx(x) for x in f])


def test_named_cases_row_functions_and_host_form(prog):
    lines, want = [], []
    for c in cases.named():
        w, st = c.world, cases.state_of(c.world)
        for s in c.steps:
            before = cases.state_of(st)
            out = cases.run_host(w, st, s)
            for how in ("row", "host"):
                lines.append(line_of(w, before, s, how))
                want.append([hx(out[k]) for k in cases.OUTS[s.kind]] + ([hx(st.rekey)] if s.kind != "recv" else []))
    assert len(lines) > 90
    assert run(prog, lines) == want
