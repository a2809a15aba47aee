"""The scalar code of the handshake response (the second half of
wireguard_amd/csrc/wgcs_noise.h and the host functions
wgcs_noise_create_response / wgcs_noise_consume_response of noise.cpp) as host
code under AddressSanitizer + UBSan, against tests/noise_resp_ref.py (CPU only).

tests/noise_resp_host/noise_resp_host.cpp is a stand-alone program that
includes the headers the kernel includes and links noise.cpp as it is.  Every
input sits in a heap buffer of exactly its size and every output in one of
exactly its size, so a byte read or written outside a key, a row or a message
is a sanitizer report.  The cases are those of tests/test_noise_resp_ref.py."""
import os
import shutil
import struct
import subprocess

import pytest

import cookie_ref
import noise_ref
import noise_resp_ref
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, LOW_ORDER_POINTS
from test_noise_resp_ref import World, failures, flip

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "noise_resp_host", "noise_resp_host.cpp")
FILL32, FILL4 = "ee" * 32, "ee" * 4


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("noise_resp") / "noise_resp_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "noise.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[-2:] == ["noise_resp_host:", "ok"]
    got = out[:-2]
    assert len(got) == len(lines)
    return got


def hx(b) -> str:
    return b.hex() if b else "-"


def le32(n: int) -> str:
    return struct.pack("<I", n).hex()


def respond_line(w, eph, index, psk, cookie, row=None, remote_static=None):
    return (f"respond {(w.row if row is None else row).hex()} {(w.init_public if remote_static is None else remote_static).hex()} "
            f"{hx(psk)} {eph.hex()} {le32(index)} {hx(cookie)}")


def consume_line(w, msg, psk, index=None, chain=None, eph=None):
    return (f"consume {w.init_private.hex()} {w.i_hash.hex()} {(w.i_chain if chain is None else chain).hex()} "
            f"{(w.init_eph if eph is None else eph).hex()} {hx(psk)} {le32(w.init_index if index is None else index)} {msg.hex()}")


def test_round_trips_with_and_without_psk_and_cookie(prog):
    lines, want = [], []
    for with_psk in (False, True):
        for with_cookie in (False, True):
            w = World(494 + 2 * with_psk + with_cookie)
            psk = w.rng.bytes(32) if with_psk else None
            cookie = w.rng.bytes(16) if with_cookie else None
            status, msg, send, recv, h, chain = noise_resp_ref.create_response(w.row, w.init_public, w.resp_eph,
                                                                               w.resp_index, psk, cookie)
            assert status == 0 and cookie_ref.Checker(w.init_public).check_mac1(msg)
            assert msg[76:] == (cookie_ref.mac128(cookie, msg[:76]) if with_cookie else bytes(16))
            lines.append(respond_line(w, w.resp_eph, w.resp_index, psk, cookie))
            want.append(f"0:{(msg + send + recv).hex()}")
            # the scalar pieces on their own
            lines.append(f"mac1key {w.init_public.hex()}")
            want.append(noise_resp_ref.mac1_key(w.init_public).hex())
            lines.append(f"core {w.row[32:64].hex()} {w.row[64:96].hex()} {w.row[96:128].hex()} {w.init_public.hex()} "
                         f"{(psk or bytes(32)).hex()} {w.resp_eph.hex()} {le32(w.resp_index)} {le32(w.init_index)}")
            want.append(f"0:{(msg[:60] + send + recv).hex()}")
            lines.append(f"write {msg[:60].hex()} {noise_resp_ref.mac1_key(w.init_public).hex()} {hx(cookie)}")
            want.append(msg.hex())
            # the initiator's side: the same hash and chaining key mean crossed keys
            i = noise_resp_ref.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, msg, psk)
            assert i[:4] == (0, w.resp_index, recv, send) and i[4:] == (h, chain)
            lines.append(consume_line(w, msg, psk))
            want.append(f"0:{le32(w.resp_index)}{(recv + send).hex()}")
            if with_psk:  # an explicit zero key is no key, and the wrong key does not authenticate
                lines.append(consume_line(w, msg, bytes(32)))
                want.append(f"{ERR_AUTH}:{FILL4}{bytes(64).hex()}")
            else:
                z = noise_resp_ref.create_response(w.row, w.init_public, w.resp_eph, w.resp_index, bytes(32), cookie)
                assert z[1] == msg
                lines.append(respond_line(w, w.resp_eph, w.resp_index, bytes(32), cookie))
                want.append(f"0:{(msg + send + recv).hex()}")
    assert run(prog, lines) == want


def test_every_failure_of_consume_response(prog):
    lines, want = [], []
    for with_psk in (False, True):
        w = World(573 + with_psk)
        psk = w.rng.bytes(32) if with_psk else None
        msg = noise_resp_ref.create_response(w.row, w.init_public, w.resp_eph, w.resp_index, psk, w.rng.bytes(16))[1]
        for name, bad, status in failures(w, msg):
            assert noise_resp_ref.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, bad,
                                                   psk)[0] == status, name
            lines.append(consume_line(w, bad, psk))
            want.append(f"{status}:{FILL4}{bytes(64).hex()}")  # the sender is left, the keys are zeroed
        lines.append(consume_line(w, msg, psk, index=w.init_index ^ 1))
        want.append(f"{ERR_INVALID_ARG}:{FILL4}{bytes(64).hex()}")
        lines.append(consume_line(w, msg, psk, chain=flip(w.i_chain, 31, 7)))
        want.append(f"{ERR_AUTH}:{FILL4}{bytes(64).hex()}")
        lines.append(consume_line(w, msg, psk, eph=w.rng.bytes(32)))
        want.append(f"{ERR_AUTH}:{FILL4}{bytes(64).hex()}")
        ok = noise_resp_ref.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, msg, psk)
        lines.append(consume_line(w, msg[:60] + w.rng.bytes(32), psk))  # the MACs are not this step's
        want.append(f"0:{le32(ok[1])}{(ok[2] + ok[3]).hex()}")
    assert run(prog, lines) == want


def test_low_order_inputs_of_create_response(prog):
    w = World(520)
    lines, want = [], []
    zeros = f"{ERR_LOW_ORDER}:{bytes(92 + 64).hex()}"
    for u in LOW_ORDER_POINTS:
        for point in (u, flip(u, 31, 7)):  # bit 255 is ignored
            bad = w.row[:96] + point
            assert noise_resp_ref.create_response(bad, w.init_public, w.resp_eph, 1)[0] == ERR_LOW_ORDER
            lines.append(respond_line(w, w.resp_eph, 1, None, None, row=bad))
            want.append(zeros)
            lines.append(respond_line(w, w.resp_eph, 1, w.rng.bytes(32), w.rng.bytes(16), remote_static=point))
            want.append(zeros)
        lines.append(f"core {w.row[32:64].hex()} {w.row[64:96].hex()} {u.hex()} {w.init_public.hex()} {bytes(32).hex()} "
                     f"{w.resp_eph.hex()} {le32(1)} {le32(2)}")
        want.append(f"{ERR_LOW_ORDER}:{bytes(60 + 64).hex()}")
    # edge scalars: the clamp makes the all-zero and the all-ones ephemeral keys ordinary ones
    for eph in (bytes(32), b"\xff" * 32):
        r = noise_resp_ref.create_response(w.row, w.init_public, eph, 0xFFFFFFFF, None, None)
        assert r[0] == 0
        lines.append(respond_line(w, eph, 0xFFFFFFFF, None, None))
        want.append(f"0:{(r[1] + r[2] + r[3]).hex()}")
    assert run(prog, lines) == want
