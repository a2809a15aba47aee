"""The transport AEAD's checker and host arithmetic (CPU only): the RFC 8439
restatement of tests/aead_ref.py against the RFC's own vector and against the
local OpenSSL, the committed golden file, and padding() -- restated, and as the
library's wgcs_padding -- against device/send.go:529-560."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aead_ref
import wireguard_amd
from wireguard_amd import _lib, transport

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_aead_golden  # noqa: E402

# RFC 8439 §2.8.2
RFC_KEY = bytes(range(0x80, 0xA0))
RFC_NONCE = bytes.fromhex("070000004041424344454647")
RFC_AAD = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
RFC_PT = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
          b"sunscreen would be it.")
RFC_CT = bytes.fromhex(
    "d31a8d34648e60db7b86afbc53ef7ec2" "a4aded51296e08fea9e2b5a736ee62d6" "3dbea45e8ca9671282fafb69da92728b"
    "1a71de0a9e060b2905d6a5b67ecd3b36" "92ddbd7f2d778b8c9803aee328091b58" "fab324e4fad675945585808b4831d7bc"
    "3ff4def08e4b7a9de576d26586cec64b" "6116")
RFC_TAG = bytes.fromhex("1ae10b594f09e26a7e902ecbd0600691")


@pytest.fixture(scope="module")
def lc():
    got = aead_ref.libcrypto()
    if got is None:
        pytest.skip("no libcrypto with EVP_chacha20_poly1305")
    return got


def test_rfc_vector_restatement():
    assert aead_ref.aead_seal(RFC_KEY, RFC_NONCE, RFC_PT, RFC_AAD) == RFC_CT + RFC_TAG
    assert aead_ref.aead_open(RFC_KEY, RFC_NONCE, RFC_CT + RFC_TAG, RFC_AAD) == RFC_PT
    bad = bytearray(RFC_CT + RFC_TAG)
    bad[0] ^= 1
    assert aead_ref.aead_open(RFC_KEY, RFC_NONCE, bytes(bad), RFC_AAD) is None
    # §2.4.2 (ChaCha20) and §2.5.2 (Poly1305) on their own
    ct = aead_ref.chacha20_xor(bytes(range(32)), bytes.fromhex("000000000000004a00000000"), 1, RFC_PT)
    assert ct[:16].hex() == "6e2e359a2568f98041ba0728dd0d6981" and ct[-2:].hex() == "874d"
    key = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    assert aead_ref.poly1305(key, b"Cryptographic Forum Research Group").hex() == "a8061dc1305136c6c22b8baf0c0127a9"


def test_rfc_vector_libcrypto(lc):
    assert lc.seal(RFC_KEY, RFC_NONCE, RFC_PT, RFC_AAD) == RFC_CT + RFC_TAG
    assert lc.open(RFC_KEY, RFC_NONCE, RFC_CT + RFC_TAG, RFC_AAD) == RFC_PT
    bad = bytearray(RFC_CT + RFC_TAG)
    bad[-1] ^= 0x80
    assert lc.open(RFC_KEY, RFC_NONCE, bytes(bad), RFC_AAD) is None


def test_restatement_matches_libcrypto(lc):
    rng = np.random.default_rng(20261019)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1420, 1452, 4096, 9000, 65487, 65519]
    lens += [int(x) for x in rng.integers(0, 3000, 12)]
    for n in lens:
        key, pt = rng.bytes(32), rng.bytes(n)
        counter = int(rng.integers(0, 2**64, dtype=np.uint64))
        aad = rng.bytes(int(rng.integers(0, 40))) if n % 2 else b""
        nonce = aead_ref.wg_nonce(counter) if n % 3 else rng.bytes(12)
        sealed = aead_ref.aead_seal(key, nonce, pt, aad)
        assert sealed == lc.seal(key, nonce, pt, aad), n
        assert aead_ref.aead_open(key, nonce, sealed, aad) == pt and lc.open(key, nonce, sealed, aad) == pt


def test_golden_file_regenerates_identically(lc):
    with open(make_aead_golden.OUT) as f:
        committed = f.read()
    assert make_aead_golden.dumps(make_aead_golden.generate(lc)) == committed
    assert len(committed) < 100_000


def test_golden_file_against_restatement():
    """Needs no libcrypto: the committed messages are what RFC 8439 says."""
    import hashlib
    with open(make_aead_golden.OUT) as f:
        g = json.load(f)
    assert len(g["cases"]) >= 30
    for rec in g["cases"]:
        packet, msg = make_aead_golden.expand(rec)
        want = aead_ref.wg_seal(bytes.fromhex(rec["key"]), rec["remote_index"], rec["counter"], packet, rec["mtu"])
        if msg is not None:
            assert want == msg
        else:
            assert len(want) == rec["msg_len"] and want[-16:].hex() == rec["tag"]
            assert want[16:32].hex() == rec["ct_first"] and want[-32:-16].hex() == rec["ct_last"]
            assert hashlib.sha256(want).hexdigest() == rec["msg_sha256"]
        counter, pt = aead_ref.wg_open(bytes.fromhex(rec["key"]), want)
        assert counter == rec["counter"] and pt[:len(packet)] == packet and not any(pt[len(packet):])


def test_padding_worked_examples():
    """The comments of send.go:532-558."""
    assert aead_ref.padding(1300, 0) == 12
    assert aead_ref.padding(1600, 1500) == 12  # 1600 % 1500 = 100 -> 112
    assert aead_ref.padding(1420, 1420) == 0  # min(1424, 1420)
    assert aead_ref.padding(3000, 1500) == 0  # lastUnit = 0
    assert aead_ref.padding(1419, 1420) == 1
    assert aead_ref.padding(0, 0) == 0 and aead_ref.padding(0, 1420) == 0


def go_padding(packet_size: int, mtu: int) -> int:
    """A second, independent spelling (division instead of masks)."""
    last = packet_size
    if mtu == 0:
        return -last % 16
    if last > mtu:
        last = last - (last // mtu) * mtu
    return min(-(-last // 16) * 16, mtu) - last


def test_padding_sweep_and_library():
    L = wireguard_amd.load()
    for mtu in (0, 1, 15, 16, 17, 1280, 1420, 1500):
        for n in range(0, 4501):
            want = go_padding(n, mtu)
            assert want >= 0
            assert aead_ref.padding(n, mtu) == want, (n, mtu)
            assert L.wgcs_padding(n, mtu) == want, (n, mtu)
    assert transport.padding(1300, 0) == 12
    for n in (65535, 65536, 65537, 1 << 20, (1 << 32) + 5):  # past what a descriptor carries
        for mtu in (0, 1420, 65535):
            assert L.wgcs_padding(n, mtu) == go_padding(n, mtu), (n, mtu)


def test_trim_restatement():
    def v4(total, n):
        return bytes([0x45, 0]) + total.to_bytes(2, "big") + bytes(n - 4)

    def v6(payload, n):
        return bytes([0x60, 0, 0, 0]) + payload.to_bytes(2, "big") + bytes(n - 6)
    assert aead_ref.trim(b"") == 0
    assert aead_ref.trim(v4(100, 100)) == 100 and aead_ref.trim(v4(60, 100)) == 60
    assert aead_ref.trim(v4(101, 100)) == aead_ref.trim(v4(19, 100)) == aead_ref.ERR_PACKET_TOO_SHORT
    assert aead_ref.trim(v4(19, 19)) == aead_ref.ERR_PACKET_TOO_SHORT
    assert aead_ref.trim(v6(60, 100)) == 100 and aead_ref.trim(v6(10, 100)) == 50
    assert aead_ref.trim(v6(61, 100)) == aead_ref.trim(v6(0, 39)) == aead_ref.ERR_PACKET_TOO_SHORT
    assert aead_ref.trim(v6(65535, 100)) == 39  # uint16: 65535 + 40 wraps
    assert aead_ref.trim(bytes([0x50]) + bytes(99)) == aead_ref.ERR_PACKET_TOO_SHORT


def test_abi_layouts_and_symbols(tmp_path):
    """Size checks of the two new structs against the header, as tests/test_abi.py
    does for the older ones."""
    src = tmp_path / "t.c"
    src.write_text(
        '#include "wgcsum.h"\n#include <stddef.h>\n'
        '_Static_assert(sizeof(wgcs_aead_key) == 48, "key");\n'
        '_Static_assert(offsetof(wgcs_aead_key, remote_index) == 32, "remote_index");\n'
        '_Static_assert(sizeof(wgcs_aead_pkt) == 24, "pkt");\n'
        '_Static_assert(offsetof(wgcs_aead_pkt, counter) == 8, "counter");\n'
        '_Static_assert(offsetof(wgcs_aead_pkt, len) == 16, "len");\n'
        '_Static_assert(offsetof(wgcs_aead_pkt, key) == 20, "key index");\n'
        '_Static_assert(WGCS_ERR_AUTH == -18, "auth");\n'
        "int main(void) { return 0; }\n")
    inc = os.path.join(os.path.dirname(HERE), "include")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", "-o", str(tmp_path / "t.o"),
                    str(src)], check=True)
    assert transport.AEAD_KEY_DTYPE.itemsize == C.sizeof(_lib.AeadKey) == 48
    assert transport.AEAD_PKT_DTYPE.itemsize == C.sizeof(_lib.AeadPkt) == 24
    for name in ("off", "counter", "len", "key"):
        assert transport.AEAD_PKT_DTYPE.fields[name][1] == getattr(_lib.AeadPkt, name).offset
    assert transport.AEAD_KEY_DTYPE.fields["remote_index"][1] == _lib.AeadKey.remote_index.offset == 32
    L = wireguard_amd.load()
    assert _lib.ERR_AUTH == -18 and b"authentication failed" in L.wgcs_strerror(_lib.ERR_AUTH)
    for name in ("wgcs_padding", "wgcs_aead_seal", "wgcs_aead_open", "wgcs_aead_seal_batch", "wgcs_aead_open_batch"):
        assert name in _lib.declared_symbols() and hasattr(L, name)
