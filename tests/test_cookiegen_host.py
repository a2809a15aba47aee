"""The bodies of wireguard_amd/csrc/wgcs_cookiegen.h (claim and commit of
lastMAC1, open and commit of cookie replies, the ageing row) and the host forms
of cookiegen.cpp as host code under AddressSanitizer + UBSan (CPU only).

tests/cookiegen_host/cookiegen_host.cpp is a stand-alone program with its own
main that includes the header the kernels include and links cookiegen.cpp as
it is.  Every table and every row array sits in a heap buffer of exactly its
size, and the last message of every arena ends where the buffer ends, so a
probe that does not wrap at a table's end or a message read past its length is
a sanitizer report.  The calls are written here; what the program prints is
compared with the library's host forms, which tests/test_cookiegen_ref.py pins
to the restatement.  Nothing loaded into Python is built with a sanitizer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from cookiegen_cases import REFRESH, SECOND, UNKNOWN, arena_of, lookup_world, sent_arrays, sent_status
from wireguard_amd import cookiegen as cg
from wireguard_amd._lib import HS_NONE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "cookiegen_host", "cookiegen_host.cpp")
NOW = 1000 * SECOND


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("cookiegen") / "cookiegen_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "cookiegen.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.splitlines()
    assert out[-1] == "cookiegen_host: ok" and len(out) == len(lines) + 1
    return [ln.split() for ln in out[:-1]]


def hx(a) -> str:
    b = a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


def i64(v) -> str:
    return struct.pack("<q", v).hex()


def calls():
    """(line fields, the library's answer) for sequences of the five calls over lookup_world."""
    for seed in range(6):
        rng = np.random.default_rng(500 + seed)
        w = lookup_world(rng)
        yield ["build", hx(w.table)], [hx(cg.gen_build(w.table))]
        now = NOW
        for step in range(8):
            now += int(rng.choice([0, 1, SECOND, REFRESH, REFRESH + 1]))
            kind = ("init", "resp", "consume", "age")[step % 4]
            if kind in ("init", "resp"):
                n = int(rng.choice([0, 1, 9]))
                d, st, msgs, mac1s = sent_arrays(rng, kind, rng.integers(0, w.n_peers + 1, n),
                                                 rng.choice([sent_status(kind), HS_NONE], n, p=[.85, .15]))
                before = w.gen.copy()
                (cg.initiated_host if kind == "init" else cg.responded_host)(d, st, msgs, w.gen)
                w.ref_sent(d["peer_row"], st, sent_status(kind), mac1s)  # so that the replies below open
                yield [kind, hx(d), hx(st), hx(msgs), hx(before)], [hx(w.gen)]
            elif kind == "consume":
                rows = [(3, w.reply(i, r, fast=True)) for i, r in ((0x1001, 0), (0x3001, 2), (0x1001, 0), (UNKNOWN, 1),
                                                                  (0x4001, 0), (0x2001, 1), (0x1002, 3))]
                rows += [(3, rng.bytes(63)), (3, rng.bytes(65)), (1, rng.bytes(64)), (3, w.reply(0x3002, 1, fast=True))]
                rows = [rows[i] for i in rng.permutation(len(rows))][:int(rng.choice([0, 1, 11]))]
                arena, pkts = arena_of([m for _, m in rows], tail=0)  # the last message ends at the buffer's end
                types = np.array([t for t, _ in rows], np.int32)
                gen0, peers0 = w.gen.copy(), w.peers.copy()
                work = np.full(16 * len(rows), 0xEE, np.uint8)
                v = cg.consume_host(arena, pkts, types, now, w.hs_slots, w.states, w.slots, w.key_peer, w.peer_rows,
                                    w.gen, w.peers, work=work)
                yield (["consume", hx(arena), hx(pkts), hx(types), i64(now), hx(w.hs_slots), hx(w.states), hx(w.slots),
                        hx(w.key_peer), hx(w.peer_rows), hx(gen0), hx(peers0)],
                       [hx(v), hx(work), hx(w.gen), hx(w.peers)])
            else:
                before = w.peers.copy()
                cg.age_host(now, w.gen, w.peers)
                yield ["age", i64(now), hx(w.gen), hx(before)], [hx(w.peers)]


def test_row_functions_and_host_forms(prog):
    lines, want, kept = [], [], 0
    for call, out in calls():
        for how in (("host",) if call[0] == "build" else ("row", "host")):
            lines.append(" ".join([call[0], how] + call[1:]))
            want.append(out)
        kept += call[0] == "consume" and struct.pack("<i", cg.HS_COOKIE_KEPT).hex() in out[0]
    assert len(lines) > 80 and kept >= 3
    assert run(prog, lines) == want
