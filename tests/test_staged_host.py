"""The row functions of wireguard_amd/csrc/wgcs_staged.h and the host forms of
staged.cpp as host code under AddressSanitizer + UBSan (CPU only).

tests/staged_host/staged_host.cpp is a stand-alone program with its own main
that includes the header the kernels include and links staged.cpp as it is.
Every table, arena, ring, job table and scratch area sits in a heap buffer of
exactly its size, and the last slot of each ends where the buffer ends, so a
ring position that is not masked, a slot index past the table or a copy of one
byte too many is a sanitizer report.  The calls are those of
tests/staged_cases.py, recorded here; what the program prints is compared with
the library's host forms, which tests/test_staged_ref.py pins to the
restatement.  Nothing loaded into Python is built with a sanitizer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import staged_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "staged_host", "staged_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("staged") / "staged_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "staged.cpp")],
                   check=True, timeout=300)
    return str(exe)


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def u32(v) -> str:
    return struct.pack("<I", v).hex()


def u64(v) -> str:
    return struct.pack("<Q", v).hex()


class Recorder:
    """the host forms, every call written down with what it read and what it wrote"""

    def __init__(self, w, lines, want):
        self.w, self.host, self.lines, self.want = w, sc.HostSide(w), lines, want

    @property
    def st(self):
        return self.host.st

    def stage(self, jb):
        st, w = self.st, self.w
        line = ["stage", u64(w.stride), u32(jb.max_segs), u32(w.cap), hx(jb.arena), hx(jb.sizes), hx(jb.peer), hx(jb.count),
                hx(jb.status_in), hx(jb.status_out), hx(jb.job_key), hx(w.peer_rows)] + [hx(a) for a in st.arrays()]
        where = self.host.stage(jb)
        if len(jb.count):  # n_jobs == 0 is a no-op: where is not written
            self.lines.append(" ".join(line))
            self.want.append([hx(where)] + [hx(a) for a in st.arrays()])
        return where

    def release(self, now, n_out_max):
        st, w = self.st, self.w
        line = ["release", struct.pack("<q", now).hex(), u64(w.limit), u64(w.stride), u32(w.cap), u32(n_out_max), hx(w.table),
                hx(w.kp), hx(w.nonce), hx(w.rekey), hx(st.len), hx(st.head), hx(st.slot_size), hx(st.ring)]
        o = self.host.release(now, n_out_max, w.rekey)
        self.lines.append(" ".join(line))
        out = np.full(len(o.out), 0xEE, np.uint8)  # the program's job table starts as 0xEE
        for k in range(o.n_out):
            a, b = k * w.stride + 16, k * w.stride + 16 + int(o.sizes[k])
            out[a:b] = o.out[a:b]
        self.want.append([hx(o.status), u32(o.n_out), hx(out), hx(o.peer), hx(o.count), hx(o.sizes), hx(o.out_status),
                          hx(w.rekey), hx(st.len), hx(st.head)])
        return o

    def flush(self, actions):
        st = self.st
        line = ["flush", u32(actions is None), hx(b"" if actions is None else actions), hx(st.len), hx(st.head), hx(st.lost)]
        self.host.flush(actions)
        self.lines.append(" ".join(line))
        self.want.append([hx(st.len), hx(st.head), hx(st.lost)])


def test_host_forms_under_sanitizers(prog):
    lines, want = [], []
    for case, n_peers, cap in sc.CASES:
        rng = np.random.default_rng(77)
        case(Recorder(sc.world(rng, n_peers, cap), lines, want), rng)
    for seed in range(40):
        sc.random_sequence(Recorder(sc.random_world(seed), lines, want), seed)
    assert len(lines) > 400 and {ln.split()[0] for ln in lines} == {"stage", "release", "flush"}
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "staged_host: ok" and len(out) == len(lines) + 1
    for i, (got, exp) in enumerate(zip(out[:-1], want)):
        assert got.split() == exp, f"call {i}: {lines[i].split()[0]}"
