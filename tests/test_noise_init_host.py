"""The initiator's half of wireguard_amd/csrc/wgcs_noise.h (the row functions
noise_initiate_row, noise_finish_row and noise_finish_commit) and the host forms
wgcs_handshake_initiate_host / wgcs_handshake_finish_host of noise.cpp as host
code under AddressSanitizer + UBSan (CPU only).

tests/noise_init_host/noise_init_host.cpp is a stand-alone program that includes
the headers the kernels include and links noise.cpp as it is.  Every table sits
in a heap buffer of exactly its size -- the state and key tables end where
n_states and n_keys say, the arena ends with its last response -- so a byte read
or written outside a row, a table or a message is a sanitizer report.  The
batches are those of tests/noise_init_cases.py, the duplicate-response batch
among them; what the program prints is compared with the library's host forms,
which tests/test_noise_init_ref.py pins to the restatements."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import noise_init_cases as cases
from noise_init_cases import N_PEERS, PITCH, WORK, world
from noise_ref import ERR_AUTH
from wireguard_amd import noise
from wireguard_amd.noise import HS_STATE_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "noise_init_host", "noise_init_host.cpp")
FILL = 0xEE


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("noise_init") / "noise_init_host"
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
    assert out[-1] == "noise_init_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def initiate_line(how, n):
    w = world()
    d, n_states, n_keys = cases.start_batch(n)
    states = np.full(n_states * 128, FILL, np.uint8)
    return f"initiate {how} {hx(d)} {w.public.hex()} {hx(w.table)} {struct.pack('<I', n_keys).hex()} {hx(states)}"


def test_initiate_rows_and_host_form(prog):
    w = world()
    lines, want = [], []
    for n in (1, 40):
        d, n_states, n_keys = cases.start_batch(n)
        states = np.full(n_states * 128, FILL, np.uint8).view(HS_STATE_DTYPE)
        msgs, status = np.full(n * PITCH, FILL, np.uint8), np.full(n, -1, np.int32)
        noise.initiate_host(d, w.public, w.table, states, msgs, status, n_keys)
        for how in ("row", "host"):
            lines.append(initiate_line(how, n))
            want.append([hx(status), hx(msgs), hx(states)])
    assert run(prog, lines) == want


def finish_line(how, c, states, keys, use_gate=True, psk=True):
    w = world()
    end = int(c.pkts["off"][c.n - 1]) + 92  # the arena ends with its last response
    return (f"finish {how} {hx(c.arena[:end])} {hx(c.pkts)} {hx(c.types)} {hx(c.gate) if use_gate else '-'} "
            f"{hx(w.responder)} {hx(c.slots)} {hx(states[:c.n_states])} {hx(w.psk) if psk else '-'} "
            f"{struct.pack('<I', N_PEERS).hex()} {hx(keys[:c.n_keys])}")


def test_finish_rows_and_host_form_with_the_duplicate_responses(prog):
    lines, want = [], []
    for n in (1, 48):
        c = cases.finish_case(n)
        if n > 1:
            q = c.kinds.index("forged")
            assert c.kinds[q:q + 3] == ["forged", "first", "copy"] and c.want[q] == ERR_AUTH
        fresh_keys = np.full(c.n_keys * 48, FILL, np.uint8).view(AEAD_KEY_DTYPE)
        for use_gate, psk in ((True, True), (False, False)):
            states, keys, work, verdict = cases.finish_expect(c, keys=fresh_keys, use_gate=use_gate,
                                                              psk="table" if psk else None)
            if use_gate and psk:
                assert verdict[:n].tolist() == c.want.tolist()
            out = [hx(verdict[:n]), hx(states[:c.n_states]), hx(keys[:c.n_keys]), hx(work[:WORK * n])]
            for how in ("row", "host"):
                lines.append(finish_line(how, c, c.states, fresh_keys, use_gate, psk))
                want.append(out)
            if use_gate and psk:  # again on the finished tables: nothing moves
                again = cases.finish_expect(c, states=states, keys=keys)
                assert again[0].tobytes() == states.tobytes() and again[1].tobytes() == keys.tobytes()
                lines.append(finish_line("host", c, states, keys))
                want.append([hx(again[3][:n]), out[1], out[2], out[3]])
    assert run(prog, lines) == want
