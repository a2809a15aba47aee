"""The handshake screen on the CPU: tests/cookie_ref.py pinned to published
vectors, then the host functions of the C ABI (wireguard_amd.cookie over
cookie.cpp) against it, and the cookie round trip through the C ABI alone."""
import os
import subprocess

import numpy as np
import pytest

import cookie_ref
from wireguard_amd import _lib, cookie

SUNSCREEN = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
             b"sunscreen would be it.")


# ------------------------------------------------------------ the restatement
def test_rfc_7693_appendix_b():
    assert cookie_ref.hash256(b"abc").hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"


def test_xchacha_draft_hchacha20():
    got = cookie_ref.hchacha20(bytes(range(32)), bytes.fromhex("000000090000004a0000000031415927"))
    assert got.hex() == "82413b4227b27bfed30e42508a877d73a0f9e4d58a74a853c12ec41326d3ecdc"


def test_xchacha_draft_a3_aead():
    key, nonce = bytes(range(0x80, 0xA0)), bytes(range(0x40, 0x58))
    aad = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    sealed = cookie_ref.xseal(key, nonce, SUNSCREEN, aad)
    assert len(sealed) == len(SUNSCREEN) + 16
    assert sealed[:16].hex() == "bd6d179d3e83d43b9576579493c0e939"
    assert sealed[-16:].hex() == "c0875924c1c7987947deafd8780acf49"
    assert cookie_ref.xopen(key, nonce, sealed, aad) == SUNSCREEN
    assert cookie_ref.xopen(key, nonce, sealed, aad[:-1] + b"\0") is None
    assert cookie_ref.xopen(key, nonce, sealed[:-1] + bytes([sealed[-1] ^ 1]), aad) is None


# ------------------------------------------------------- the host ABI functions
def sources(rng):
    """(what src_addr takes, the bytes the reference hashes)"""
    out = []
    for ip in (rng.bytes(4), rng.bytes(16), bytes(4), b"\xff" * 16):
        port = int(rng.integers(65536))
        out.append(((ip, port), cookie_ref.src_bytes(ip, port)))
    return out


def test_layouts_and_constants():
    assert cookie.COOKIE_CHECKER_DTYPE.itemsize == 96 and cookie.SRC_ADDR_DTYPE.itemsize == 20
    assert (cookie.HS_NONE, cookie.HS_PASS, cookie.HS_COOKIE) == (0, 1, 2) and cookie.ERR_MAC1 == -21
    L = _lib.load()
    assert L.wgcs_abi_version() == 2
    assert L.wgcs_strerror(-21) not in (b"unknown status", b"")
    row = cookie.src_addr("192.0.2.7", 0x1234)
    assert row["b"][0, :6].tobytes() == bytes([192, 0, 2, 7, 0x34, 0x12]) and int(row["len"][0]) == 6
    row = cookie.src_addr("2001:db8::1", 51820)
    assert int(row["len"][0]) == 18 and row["b"][0, 16:18].tobytes() == (51820).to_bytes(2, "little")


def test_header_layouts(tmp_path):
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "t.c"
    src.write_text('#include "wgcsum.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(wgcs_cookie_checker) == 96, "checker");\n'
                   '_Static_assert(offsetof(wgcs_cookie_checker, cookie_key) == 32, "cookie_key");\n'
                   '_Static_assert(offsetof(wgcs_cookie_checker, secret) == 64, "secret");\n'
                   '_Static_assert(sizeof(wgcs_src_addr) == 20, "src");\n'
                   '_Static_assert(offsetof(wgcs_src_addr, len) == 18, "len");\n'
                   '_Static_assert(WGCS_ERR_MAC1 == -21 && WGCS_HS_NONE == 0 && WGCS_HS_PASS == 1 && WGCS_HS_COOKIE == 2, "codes");\n'
                   "int main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "t")], check=True)
    assert [cookie.COOKIE_CHECKER_DTYPE.fields[f][1] for f in ("mac1_key", "cookie_key", "secret")] == [0, 32, 64]
    assert [cookie.SRC_ADDR_DTYPE.fields[f][1] for f in ("b", "len", "pad")] == [0, 18, 19]


def test_host_functions_match_the_restatement():
    rng = np.random.default_rng(20261020)
    for _ in range(8):
        pub, secret = rng.bytes(32), rng.bytes(32)
        ref = cookie_ref.Checker(pub, secret)
        assert cookie.checker_init(pub).tobytes() == cookie_ref.Checker(pub).tobytes()
        ck = cookie.checker_init(pub, secret)
        assert ck.tobytes() == ref.tobytes()
        for type_ in (1, 2):
            blank = cookie_ref.handshake_message(rng, type_, ref.mac1_key)[:-32] + rng.bytes(32)
            want_msg, want_mac1 = cookie_ref.add_macs(ref.mac1_key, blank)
            msg, mac1 = cookie.add_macs(ref.mac1_key, blank)
            assert (msg, mac1) == (want_msg, want_mac1)
            assert cookie.check_mac1(ck, msg) and ref.check_mac1(msg)
            for i in (0, len(msg) - 33, len(msg) - 32, len(msg) - 17):
                bad = msg[:i] + bytes([msg[i] ^ 4]) + msg[i + 1:]
                assert not cookie.check_mac1(ck, bad) and not ref.check_mac1(bad)
            for (ip, port), sb in sources(rng):
                src, nonce = cookie.src_addr(ip, port), rng.bytes(24)
                assert not cookie.check_mac2(ck, msg, src)
                reply = cookie.create_reply(ck, msg, src, nonce)
                assert reply == ref.create_reply(msg, sb, nonce)
                assert cookie.consume_reply(ref.cookie_key, mac1, reply) == ref.cookie(sb)
                assert cookie.consume_reply(ref.cookie_key, mac1, reply[:-1] + bytes([reply[-1] ^ 0x80])) is None
                assert cookie.consume_reply(ref.cookie_key, bytes(16), reply) is None
                with_cookie, _ = cookie.add_macs(ref.mac1_key, blank, ref.cookie(sb))
                assert with_cookie == cookie_ref.add_macs(ref.mac1_key, blank, ref.cookie(sb))[0]
                assert cookie.check_mac2(ck, with_cookie, src)
                for i in (0, len(msg) - 17, len(msg) - 16, len(msg) - 1):
                    bad = with_cookie[:i] + bytes([with_cookie[i] ^ 1]) + with_cookie[i + 1:]
                    assert not cookie.check_mac2(ck, bad, src)


def test_short_messages_and_bad_sources_are_refused():
    rng = np.random.default_rng(31)
    ck = cookie.checker_init(rng.bytes(32), rng.bytes(32))
    src = cookie.src_addr("10.0.0.1", 1)
    for n in (1, 31):
        for call in (lambda m: cookie.check_mac1(ck, m), lambda m: cookie.check_mac2(ck, m, src),
                     lambda m: cookie.create_reply(ck, m, src, bytes(24)), lambda m: cookie.add_macs(bytes(32), m)):
            with pytest.raises(_lib.WgcsError) as ei:
                call(rng.bytes(n))
            assert ei.value.code == _lib.ERR_OUT_OF_RANGE
    for bad_len in (0, 4, 17):
        bad = src.copy()
        bad["len"] = bad_len
        with pytest.raises(_lib.WgcsError) as ei:
            cookie.check_mac2(ck, bytes(148), bad)
        assert ei.value.code == _lib.ERR_INVALID_ARG


# ------------------------------------------------------------------ loopback
def host_screen(ck, msg, src, under_load):
    """The screen's rule on one message, through the C ABI's host functions."""
    if not cookie.check_mac1(ck, msg):
        return cookie.ERR_MAC1
    if not under_load or cookie.check_mac2(ck, msg, src):
        return cookie.HS_PASS
    return cookie.HS_COOKIE


@pytest.mark.parametrize("type_", [1, 2])
@pytest.mark.parametrize("ip", [bytes([203, 0, 113, 9]), bytes.fromhex("20010db8000000000000000000000042")])
def test_cookie_round_trip_through_the_c_abi(type_, ip):
    rng = np.random.default_rng(type_ * 100 + len(ip))
    pub = rng.bytes(32)
    server = cookie.checker_init(pub, rng.bytes(32))  # the responder's checker
    keys = cookie.checker_init(pub)  # the initiator's generator: the same two keys
    mac1_key, cookie_key = keys["mac1_key"][0].tobytes(), keys["cookie_key"][0].tobytes()
    src = cookie.src_addr(ip, 40000)
    body = type_.to_bytes(4, "little") + rng.bytes(cookie_ref.SIZE_OF_TYPE[type_] - 36) + bytes(32)
    # 1-3: MAC1 only passes at rest and earns a cookie reply under load
    msg, last_mac1 = cookie.add_macs(mac1_key, body)
    assert host_screen(server, msg, src, False) == cookie.HS_PASS
    assert host_screen(server, msg, src, True) == cookie.HS_COOKIE
    reply = cookie.create_reply(server, msg, src, rng.bytes(24))
    assert reply[:4] == (3).to_bytes(4, "little") and reply[4:8] == msg[4:8]
    # 4-6: the initiator recovers the cookie and its next message passes under load
    got = cookie.consume_reply(cookie_key, last_mac1, reply)
    assert got is not None and len(got) == 16
    msg2, _ = cookie.add_macs(mac1_key, body, got)
    assert host_screen(server, msg2, src, True) == cookie.HS_PASS
    # 7: the cookie binds the address and the port
    assert host_screen(server, msg2, cookie.src_addr(ip, 40001), True) == cookie.HS_COOKIE
    other = ip[:-1] + bytes([ip[-1] ^ 1])
    assert host_screen(server, msg2, cookie.src_addr(other, 40000), True) == cookie.HS_COOKIE
    # 8: and the secret
    server["secret"][0] = np.frombuffer(rng.bytes(32), dtype=np.uint8)
    assert host_screen(server, msg2, src, True) == cookie.HS_COOKIE
    assert host_screen(server, msg2, src, False) == cookie.HS_PASS
