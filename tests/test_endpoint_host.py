"""The bodies of wireguard_amd/csrc/wgcs_endpoint.h (the control-message walk,
one slot's endpoint, claim and commit, read and clear over the sources of wgcs_events.h) and the
host forms of endpoint.cpp as host code under AddressSanitizer + UBSan (CPU only).

tests/endpoint_host/endpoint_host.cpp is a stand-alone program with its own main
that includes the header the kernels include and links endpoint.cpp as it is.
Every table and every row array sits in a heap buffer of exactly its size -- the
control buffers in one of exactly n * oob_stride bytes, the last message of the
arena ending where the buffer ends -- so a walk past a slot, a source row past
d_ep or a job's lengths past its segments is a sanitizer report.  The calls are
written here; what the program prints is compared with the library's host forms,
which tests/test_endpoint_ref.py pins to the restatement.  Nothing loaded into
Python is built with a sanitizer."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from cookiegen_cases import arena_of
from endpoint_cases import ADDRS, CLEAR_SRC, World, addr_row, control_cases, ep_rows, finished_rows, oob_of, random_endpoints
from wireguard_amd import _lib, endpoint as ep, noise
from wireguard_amd._lib import HS_FINISHED, HS_INITIATED, HS_NONE, HS_RESPONDED, PEER_NONE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "endpoint_host", "endpoint_host.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("endpoint") / "endpoint_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "endpoint.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "endpoint_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def u32(v) -> str:
    return struct.pack("<I", v).hex()


def calls():
    """(line fields, the library's answer) for the control cases and for sequences of the seven calls."""
    L = _lib.load()
    for control in control_cases().values():
        g = C.c_int(-1)
        rc = L.wgcs_get_gso_size(control, len(control), C.byref(g))
        yield ["gso", hx(control)], [str(rc), str(g.value)], False
    cases = list(control_cases().values())
    for seed in range(4):
        rng = np.random.default_rng(700 + seed)
        w = World(rng)
        # the tightest stride that holds the longest case: the last slot's control ends with the buffer
        stride = (max(len(c) for c in cases) + 3) // 4 * 4
        for step in range(10):
            n_msgs, nb = int(rng.choice([1, 5])), int(rng.choice([1, 3]))
            n = n_msgs * nb
            controls = [cases[int(rng.integers(0, len(cases)))] for _ in range(n - 1)] + [max(cases, key=len)]
            oob, nn = oob_of(controls, stride)
            addrs = np.concatenate([addr_row(ADDRS[int(rng.integers(0, 4))]) for _ in range(n)])
            frm = np.array([int(rng.choice([-1, -1, 0, n_msgs - 1, n_msgs, -2])) for _ in range(n)], np.int32)
            size = rng.choice([0, 60, 148], n).astype(np.int32)
            use_from = step % 2 == 0
            eps, out = ep.recv_host(addrs, frm if use_from else None, size, oob, stride, nn, n_msgs, nb)
            yield (["recv", hx(addrs), hx(frm) if use_from else "-", hx(size), hx(oob), u32(stride), hx(nn), u32(n_msgs)],
                   [hx(eps), hx(out)], True)

            def tables():
                return [hx(w.table), hx(w.claim), hx(w.timers)]

            w.timers["flags"] ^= np.where(rng.random(w.n_peers) < 0.3, CLEAR_SRC, 0).astype(np.uint32)
            kind = ("received", "jobs", "accepted", "init", "finished", "resp")[step % 6]
            if kind == "received":
                groups = w.groups([(int(rng.choice(w.ids + [0, PEER_NONE])), int(rng.integers(-1, n + 1))) for _ in range(6)])
                before = tables()
                ep.set_received_host(groups, 3, eps, w.peer_rows, w.table, w.claim, w.timers)
                yield ["received", hx(groups), u32(3), hx(eps), hx(w.peer_rows)] + before, tables(), True
            elif kind == "accepted":
                d = np.zeros(5, noise.HS_RESP_DTYPE)
                d["init_row"], d["peer_row"] = rng.choice([0, n - 1, n, 0xFFFFFFFF], 5), rng.integers(0, w.n_peers + 1, 5)
                before = tables()
                ep.set_accepted_host(d, eps, w.table, w.claim, w.timers)
                yield ["accepted", hx(d), hx(eps)] + before, tables(), True
            elif kind == "finished":
                peer_rows = [rng.choice([None, 0, 1, 4, 9]) for _ in range(n)]
                gates = [int(rng.choice([HS_FINISHED, HS_NONE])) for _ in range(n)]
                arena, pkts, gate, hs_slots, states = finished_rows(rng, w, peer_rows, gates)
                arena = arena[:int(pkts["off"][-1]) + int(pkts["len"][-1])]  # the last message ends with the buffer
                before = tables()
                ep.set_finished_host(arena, pkts, gate, hs_slots, states, eps, w.table, w.claim, w.timers)
                yield ["finished", hx(arena), hx(pkts), hx(gate), hx(hs_slots), hx(states), hx(eps)] + before, tables(), True
            elif kind == "jobs":
                m, max_segs = 7, 3
                peer = np.full(m * max_segs, PEER_NONE, np.uint32)
                peer[::max_segs] = rng.choice(w.ids + [0], m)
                count, status = rng.integers(0, 5, m).astype(np.int32), rng.choice([0, 0, 0, -26], m).astype(np.int32)
                key = rng.choice([1, 0xFFFFFFFF], m, p=[.9, .1]).astype(np.uint32)
                lens = rng.integers(-3, 1500, m * max_segs).astype(np.int32)
                nbufs = rng.integers(-1, 6, m).astype(np.int32)  # whatever the caller left there: clamped to the segments
                before = [hx(nbufs), hx(w.peer_rows), hx(w.table), hx(w.timers)]
                dst, v6, ds, tx = ep.dst_jobs_host(peer, count, status, key, max_segs, lens, nbufs, w.peer_rows, w.table, w.timers)
                yield (["jobs", hx(peer), hx(count), hx(status), hx(key), u32(max_segs), hx(lens)] + before,
                       [hx(dst), hx(v6), hx(ds), hx(tx), hx(nbufs), hx(w.table), hx(w.timers)], True)
            else:
                dtype, ok, fn = ((noise.HS_START_DTYPE, HS_INITIATED, ep.dst_initiated_host) if kind == "init" else
                                 (noise.HS_RESP_DTYPE, HS_RESPONDED, ep.dst_responded_host))
                d = np.zeros(5, dtype)
                d["peer_row"] = rng.integers(0, w.n_peers + 1, 5)
                status = rng.choice([ok, HS_NONE], 5, p=[.8, .2]).astype(np.int32)
                before = [hx(w.table), hx(w.timers)]
                dst, v6, ds = fn(d, status, w.table, w.timers)
                yield [kind, hx(d), hx(status)] + before, [hx(dst), hx(v6), hx(ds), hx(w.table), hx(w.timers)], True


def test_row_functions_and_host_forms(prog):
    lines, want = [], []
    for call, out, both in calls():
        for how in (("row", "host") if both else ("host",)):
            lines.append(" ".join([call[0], how] + call[1:]))
            want.append(out)
    assert len(lines) > 150 and {ln.split()[0] for ln in lines} == {"gso", "recv", "received", "accepted", "finished", "jobs",
                                                                   "init", "resp"}
    assert run(prog, lines) == want
