"""The scalar code of the handshake screen (wireguard_amd/csrc/wgcs_blake2s.h,
wgcs_xchacha.h, wgcs_cookie.h and the host functions of cookie.cpp) as host
code under AddressSanitizer + UBSan, against tests/cookie_ref.py (CPU only).

tests/cookie_host/cookie_host.cpp is a stand-alone program that includes the
headers the kernel includes and links cookie.cpp as it is.  Every input sits in
a heap buffer of exactly its size, so a byte read outside a message, a key, a
source or a reply is a sanitizer report, not a wrong digest that happens to be
right."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import cookie_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "cookie_host", "cookie_host.cpp")
ERR_INVALID_ARG, ERR_OUT_OF_RANGE = -1, -13


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("cookie") / "cookie_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "cookie.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[-2:] == ["cookie_host:", "ok"]
    got = out[:-2]
    assert len(got) == len(lines)
    return got


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def test_blake2s_every_length_key_digest_and_alignment(prog):
    """Message lengths 0..200 (the block edges 0, 1, 63..65, 127..129, 191..193
    among them) x key lengths 0, 16, 32 x digest lengths 16, 32, each at byte
    offsets 0..3 of a heap buffer that ends with the message."""
    rng = np.random.default_rng(7693)
    lines, want = [f"b2s - 32 0 {b'abc'.hex()}"], ["508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"]
    for n in range(0, 201):
        msg = rng.bytes(n) if n else b""
        for klen in (0, 16, 32):
            key = rng.bytes(klen) if klen else b""
            for olen in (16, 32):
                d = hashlib.blake2s(msg, key=key, digest_size=olen).hexdigest()
                for shift in range(4):
                    lines.append(f"b2s {hx(key)} {olen} {shift} {hx(msg)}")
                    want.append(d)
    assert run(prog, lines) == want


def test_blake2s_whole_blocks_and_256(prog):
    """A whole number of blocks ends with a full final block; 256 bytes is the
    longest message the header promises."""
    rng = np.random.default_rng(64)
    lines, want = [], []
    for n in (64, 128, 192, 255, 256):
        for klen in (0, 16, 32):
            key, msg = (rng.bytes(klen) if klen else b""), rng.bytes(n)
            lines.append(f"b2s {hx(key)} 16 1 {msg.hex()}")
            want.append(hashlib.blake2s(msg, key=key, digest_size=16).hexdigest())
    assert run(prog, lines) == want


def test_hchacha20_and_seal_open(prog):
    rng = np.random.default_rng(8439)
    lines = [f"hch {bytes(range(32)).hex()} 000000090000004a0000000031415927"]
    want = ["82413b4227b27bfed30e42508a877d73a0f9e4d58a74a853c12ec41326d3ecdc"]  # draft-irtf-cfrg-xchacha §2.2.1
    for _ in range(16):
        key, n16 = rng.bytes(32), rng.bytes(16)
        lines.append(f"hch {key.hex()} {n16.hex()}")
        want.append(cookie_ref.hchacha20(key, n16).hex())
    for trial in range(24):
        key, nonce, pt, ad = rng.bytes(32), rng.bytes(24), rng.bytes(16), rng.bytes(16)
        if trial == 0:
            key, nonce, pt, ad = b"\xff" * 32, b"\xff" * 24, b"\xff" * 16, b"\xff" * 16
        if trial == 1:
            key, nonce, pt, ad = bytes(32), bytes(24), bytes(16), bytes(16)
        sealed = cookie_ref.xseal(key, nonce, pt, ad)
        lines.append(f"seal {key.hex()} {nonce.hex()} {pt.hex()} {ad.hex()}")
        want.append(sealed.hex())
        lines.append(f"open {key.hex()} {nonce.hex()} {sealed.hex()} {ad.hex()}")
        want.append(pt.hex())

        def flip(b, i, bit=0):
            return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]
        # an altered tag (first and last byte, low and high bit), AD, ciphertext, nonce and key are refused
        for bad in (flip(sealed, 16), flip(sealed, 31, 7), flip(sealed, 0), flip(sealed, 15, 7)):
            lines.append(f"open {key.hex()} {nonce.hex()} {bad.hex()} {ad.hex()}")
            want.append("fail")
        for bad_ad in (flip(ad, 0), flip(ad, 15, 7)):
            lines.append(f"open {key.hex()} {nonce.hex()} {sealed.hex()} {bad_ad.hex()}")
            want.append("fail")
        for bad_nonce in (flip(nonce, 0), flip(nonce, 15, 7), flip(nonce, 16), flip(nonce, 23, 7)):
            lines.append(f"open {key.hex()} {bad_nonce.hex()} {sealed.hex()} {ad.hex()}")
            want.append("fail")
        lines.append(f"open {flip(key, 31, 7).hex()} {nonce.hex()} {sealed.hex()} {ad.hex()}")
        want.append("fail")
    assert run(prog, lines) == want


def sources(rng):
    return [cookie_ref.src_bytes(rng.bytes(4), int(rng.integers(65536))),
            cookie_ref.src_bytes(rng.bytes(16), int(rng.integers(65536))),
            cookie_ref.src_bytes(bytes(4), 0), cookie_ref.src_bytes(b"\xff" * 16, 65535)]


def test_checker_and_generator_on_exact_buffers(prog):
    rng = np.random.default_rng(2870)
    lines, want = [], []
    for _ in range(6):
        pub, secret = rng.bytes(32), rng.bytes(32)
        ref = cookie_ref.Checker(pub, secret)
        ck = ref.tobytes()
        lines.append(f"init {pub.hex()}")
        want.append(cookie_ref.Checker(pub).tobytes().hex())
        for type_ in (1, 2):
            body = cookie_ref.handshake_message(rng, type_, ref.mac1_key)
            blank = body[:-32] + rng.bytes(32)  # AddMACs overwrites MAC1 and, without a cookie, keeps the MAC2 field
            msg, mac1 = cookie_ref.add_macs(ref.mac1_key, blank)
            lines.append(f"add {ref.mac1_key.hex()} - {blank.hex()}")
            want.append(msg.hex() + mac1.hex())
            lines.append(f"mac1 {ck.hex()} {msg.hex()}")
            want.append("1")
            for i in (0, len(msg) - 33, len(msg) - 32, len(msg) - 17):
                bad = msg[:i] + bytes([msg[i] ^ 0x80]) + msg[i + 1:]
                lines.append(f"mac1 {ck.hex()} {bad.hex()}")
                want.append("0")
            for src in sources(rng):
                nonce = rng.bytes(24)
                lines.append(f"mac2 {ck.hex()} {src.hex()} {msg.hex()}")
                want.append("0")
                reply = ref.create_reply(msg, src, nonce)
                lines.append(f"reply {ck.hex()} {src.hex()} {nonce.hex()} {msg.hex()}")
                want.append(reply.hex())
                lines.append(f"consume {ref.cookie_key.hex()} {mac1.hex()} {reply.hex()}")
                want.append(ref.cookie(src).hex())
                assert cookie_ref.consume_reply(ref.cookie_key, mac1, reply) == ref.cookie(src)
                for i in (32, 47, 48, 63, 8, 31):  # ciphertext, tag, nonce: first and last byte
                    bad = reply[:i] + bytes([reply[i] ^ 1]) + reply[i + 1:]
                    lines.append(f"consume {ref.cookie_key.hex()} {mac1.hex()} {bad.hex()}")
                    want.append("fail")
                other_mac1 = bytes([mac1[0] ^ 1]) + mac1[1:]
                lines.append(f"consume {ref.cookie_key.hex()} {other_mac1.hex()} {reply.hex()}")
                want.append("fail")
                with_cookie, _ = cookie_ref.add_macs(ref.mac1_key, msg, ref.cookie(src))
                lines.append(f"add {ref.mac1_key.hex()} {ref.cookie(src).hex()} {blank.hex()}")
                want.append(with_cookie.hex() + mac1.hex())
                lines.append(f"mac2 {ck.hex()} {src.hex()} {with_cookie.hex()}")
                want.append("1")
                for i in (0, len(msg) - 17, len(msg) - 16, len(msg) - 1):
                    bad = with_cookie[:i] + bytes([with_cookie[i] ^ 0x01]) + with_cookie[i + 1:]
                    lines.append(f"mac2 {ck.hex()} {src.hex()} {bad.hex()}")
                    want.append("0")
    assert run(prog, lines) == want


def test_lengths_the_reference_would_panic_on(prog):
    """len < 32 slices out of range in Go: OUT_OF_RANGE, and a source that is
    not an AddrPort's 6 or 18 bytes INVALID_ARG; len == 32 is a message whose
    MACs cover nothing."""
    rng = np.random.default_rng(32)
    ref = cookie_ref.Checker(rng.bytes(32), rng.bytes(32))
    ck, src, nonce = ref.tobytes(), cookie_ref.src_bytes(rng.bytes(4), 51820), rng.bytes(24)
    lines, want = [], []
    for n in (1, 16, 31):
        msg = rng.bytes(n)
        lines += [f"mac1 {ck.hex()} {msg.hex()}", f"mac2 {ck.hex()} {src.hex()} {msg.hex()}",
                  f"reply {ck.hex()} {src.hex()} {nonce.hex()} {msg.hex()}", f"add {ref.mac1_key.hex()} - {msg.hex()}"]
        want += [str(ERR_OUT_OF_RANGE)] * 4
    msg = cookie_ref.handshake_message(rng, 1, ref.mac1_key)
    for bad_src in (b"", rng.bytes(4), rng.bytes(17)):
        lines += [f"mac2 {ck.hex()} {hx(bad_src)} {msg.hex()}", f"reply {ck.hex()} {hx(bad_src)} {nonce.hex()} {msg.hex()}"]
        want += [str(ERR_INVALID_ARG)] * 2
    m32, mac1 = cookie_ref.add_macs(ref.mac1_key, bytes(32), ref.cookie(src))
    lines += [f"add {ref.mac1_key.hex()} {ref.cookie(src).hex()} {bytes(32).hex()}", f"mac1 {ck.hex()} {m32.hex()}",
              f"mac2 {ck.hex()} {src.hex()} {m32.hex()}"]
    want += [m32.hex() + mac1.hex(), "1", "1"]
    assert run(prog, lines) == want
