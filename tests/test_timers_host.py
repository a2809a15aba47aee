"""The bodies and row functions of wireguard_amd/csrc/wgcs_timers.h (the six event rows and
the three passes of the expire call) and the host forms of timers.cpp as host
code under AddressSanitizer + UBSan (CPU only).

tests/timers_host/timers_host.cpp is a stand-alone program with its own main
that includes the header the kernels include and links timers.cpp as it is.
Every table sits in a heap buffer of exactly its size -- the jobs end with the
batch, the wgcs_timers, wgcs_rekey and wgcs_keypairs rows with their last peer,
the slot arrays with their last slot, the key rows with the last key, the
keepalive jobs with n_ka_max -- so a byte read or written outside a row or a
table is a sanitizer report.  The calls are the named cases of
tests/timers_cases.py, step by step; what the program prints is compared with
the library's host form, which tests/test_timers_ref.py pins to the
restatement.  Nothing loaded into Python is built with a sanitizer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import timers_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "timers_host", "timers_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("timers") / "timers_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "timers.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "timers_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else (b"" if a is None else np.ascontiguousarray(a).tobytes())
    return b.hex() if b else "-"


WRITTEN = dict(sent=("timers",), rcvd=("timers",), init=("timers",), resp=("timers",), fin=("timers", "rekey"),
               rot=("timers", "rekey"), exp=("timers", "rekey", "kp", "slots", "peer_keys", "keys", "key_peer"))


def line_of(w, st, s, how) -> str:
    now, u4 = struct.pack("<q", s.now), lambda v: struct.pack("<I", v)  # noqa: E731
    if s.kind == "sent":
        f = [s.sizes, s.peer, s.count, s.status, s.job_key, u4(s.max_segs), now, u4(s.jitter_seed), w.peer_rows, st.timers]
    elif s.kind == "rcvd":
        f = [s.groups, u4(s.calls_per_batch), now, w.peer_rows, st.timers]
    elif s.kind == "init":
        f = [s.reasons, s.start_peer, s.init_status, now, u4(s.jitter_seed), st.timers]
    elif s.kind == "resp":
        f = [s.resp, s.gate, now, st.timers]
    elif s.kind == "fin":
        f = [s.arena, s.pkts, s.gate, s.begun, now, w.hs_slots, w.states, st.timers, st.rekey]
    elif s.kind == "rot":
        f = [s.pkts, s.rotated, now, st.key_peer, w.peer_rows, st.timers, st.rekey]
    else:
        f = [now, st.timers, st.rekey, w.table, s.staged, st.kp, st.slots, st.peer_keys, st.keys, st.key_peer, u4(s.n_ka_max)]
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
                want.append([hx(out[k]) for k in (cases.EXP_OUTS if s.kind == "exp" else ())] +
                            [hx(getattr(st, k)) for k in WRITTEN[s.kind]])
    assert len(lines) > 150
    assert run(prog, lines) == want
