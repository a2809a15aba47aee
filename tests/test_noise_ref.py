"""tests/noise_ref.py against published vectors and a third-party
implementation, and the host functions of the C ABI (wgcs_x25519, wgcs_noise_*,
wgcs_peer_keys_*) against it through wireguard_amd.noise (CPU only).

The X25519 vectors are RFC 7748 §5.2's, carried as literals; the golden file
holds OpenSSL's output for 300 random pairs (tests/golden/make_x25519_golden.py)
and is read, never regenerated, here."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import noise_ref
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, ERR_NO_PEER, HS_CONSUMED, LOW_ORDER_POINTS, P, PEER_NONE
from wireguard_amd import _lib, cookie, noise

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "x25519_vectors.json")

RFC_VECTORS = [
    ("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
     "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
     "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
    ("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
     "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
     "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"),
]
ITER_1 = "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
ITER_1000 = "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"
# RFC 7748 §6.1: Alice's private and public key (a multiplication of the base point)
ALICE = ("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a",
         "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a")


def le(n: int) -> bytes:
    return n.to_bytes(32, "little")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("fn", [noise_ref.x25519, noise.x25519], ids=["ref", "abi"])
def test_rfc7748_vectors(fn):
    for k, u, out in RFC_VECTORS:
        assert fn(bytes.fromhex(k), bytes.fromhex(u)).hex() == out
    assert fn(bytes.fromhex(ALICE[0]), noise_ref.BASE_POINT).hex() == ALICE[1]
    k = u = noise_ref.BASE_POINT
    for i in range(1000):
        k, u = fn(k, u), k
        if i == 0:
            assert k.hex() == ITER_1
    assert k.hex() == ITER_1000


@pytest.mark.parametrize("fn", [noise_ref.x25519, noise.x25519], ids=["ref", "abi"])
def test_openssl_golden_vectors(fn):
    cases = golden()
    assert len(cases) >= 200 and any(int(c["u"][-2:], 16) & 0x80 for c in cases)
    for c in cases:
        assert fn(bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"])).hex() == c["out"]


def test_golden_generator_is_committed_and_names_openssl():
    src = open(os.path.join(HERE, "golden", "make_x25519_golden.py")).read()
    assert "pkeyutl" in src and "-derive" in src


def test_edge_points_on_the_abi():
    rng = np.random.default_rng(77)
    for k in (rng.bytes(32), bytes(32), b"\xff" * 32):
        for u in LOW_ORDER_POINTS:
            assert noise_ref.x25519(k, u) is None and noise.x25519(k, u) is None
            hi = u[:31] + bytes([u[31] | 0x80])
            assert noise.x25519(k, hi) is None
        for u, reduced in ((le(2**255 - 1), le(18)), (le(2**256 - 1), le(18)), (le(P + 2), le(2))):
            assert noise.x25519(k, u) == noise.x25519(k, reduced) == noise_ref.x25519(k, u)
    with pytest.raises(ValueError):
        noise.x25519(bytes(31), bytes(32))


def test_constants_and_layouts(tmp_path):
    assert (noise.HS_CONSUMED, noise.ERR_LOW_ORDER, noise.ERR_NO_PEER) == (3, -22, -23)
    L = _lib.load()
    assert L.wgcs_strerror(-22) not in (None, b"unknown status") and L.wgcs_strerror(-23) != b"unknown status"
    src = tmp_path / "t.c"
    src.write_text('#include "wgcsum.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(wgcs_noise_responder) == 96, "responder");\n'
                   '_Static_assert(sizeof(wgcs_peer_key) == 72 && offsetof(wgcs_peer_key, shared) == 32 && '
                   'offsetof(wgcs_peer_key, peer) == 64 && offsetof(wgcs_peer_key, flags) == 68, "peer_key");\n'
                   '_Static_assert(sizeof(wgcs_hs_init) == 128 && offsetof(wgcs_hs_init, sender) == 4 && '
                   'offsetof(wgcs_hs_init, timestamp) == 8 && offsetof(wgcs_hs_init, hash) == 32 && '
                   'offsetof(wgcs_hs_init, chain_key) == 64 && offsetof(wgcs_hs_init, ephemeral) == 96, "hs_init");\n'
                   '_Static_assert(WGCS_ERR_LOW_ORDER == -22 && WGCS_ERR_NO_PEER == -23 && WGCS_HS_CONSUMED == 3, "codes");\n'
                   "int main(void) { return 0; }\n")
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)
    for dtype, fields in ((noise.PEER_KEY_DTYPE, {"shared": 32, "peer": 64, "flags": 68}),
                          (noise.HS_INIT_DTYPE, {"sender": 4, "timestamp": 8, "hash": 32, "chain_key": 64,
                                                 "ephemeral": 96})):
        for name, at in fields.items():
            assert dtype.fields[name][1] == at


def test_initial_values_match_the_published_protocol():
    """Construction and identifier strings of the WireGuard paper §5.4; the two hashes follow."""
    import hashlib
    ck = hashlib.blake2s(b"Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s").digest()
    assert noise_ref.INITIAL_CHAIN_KEY == ck
    assert noise_ref.INITIAL_HASH == hashlib.blake2s(ck + b"WireGuard v1 zx2c4 Jason@zx2c4.com").digest()
    assert ck.hex() == "60e26daef327efc02ec335e2a025d2d016eb4206f87277f52d38d1988b78cd36"


def test_round_trip_and_failures_on_the_abi():
    rng = np.random.default_rng(344)
    ref = noise_ref.Responder(rng.bytes(32))
    r, pub = noise.responder_init(ref.private)
    assert r.tobytes() == ref.tobytes() and pub == ref.public
    init_private, stopped = rng.bytes(32), rng.bytes(32)
    peers = [(noise_ref.public_key(init_private), 7, 1), (noise_ref.public_key(stopped), 8, 0), (le(1), 9, 1)]
    peers += [(noise_ref.public_key(rng.bytes(32)), 100 + i, 1) for i in range(34)]
    want_table = noise_ref.PeerTable(ref, peers)
    table = noise.peer_keys_build(r, [p[0] for p in peers], [p[1] for p in peers], [p[2] for p in peers])
    assert table.tobytes() == want_table.tobytes()
    for i, row in enumerate(want_table.rows):
        assert noise.peer_keys_find(table, row[0]) == i
    assert noise.peer_keys_find(table, rng.bytes(32)) == -1
    assert len(noise.peer_keys_build(r, [], [])) == 0
    with pytest.raises(_lib.WgcsError):
        noise.peer_keys_build(r, [peers[0][0], peers[0][0]], [1, 2])
    with pytest.raises(_lib.WgcsError):
        noise.peer_keys_build(r, [peers[0][0]], [PEER_NONE])

    def both(msg, t=table, want_t=want_table):
        v, row = noise.consume_initiation(r, t, msg)
        wv, wrow = noise_ref.consume_initiation(ref, want_t, msg)
        assert v == wv and row.tobytes() == (bytes(128) if wrow is None else wrow)
        return v, row

    eph, ts = rng.bytes(32), rng.bytes(12)
    msg, h, chain = noise.create_initiation(init_private, ref.public, eph, ts, 0xDEADBEEF)
    assert (msg, h, chain) == noise_ref.create_initiation(init_private, ref.public, eph, ts, 0xDEADBEEF)
    v, row = both(msg)
    assert v == HS_CONSUMED and row["peer"][0] == 7 and row["sender"][0] == 0xDEADBEEF
    assert row["timestamp"][0].tobytes() == ts and row["hash"][0].tobytes() == h
    assert row["chain_key"][0].tobytes() == chain and row["ephemeral"][0].tobytes() == msg[8:40]
    # with its MACs in place it passes the screen's check and consumes alike
    ck = cookie.checker_init(ref.public)
    with_macs, _ = cookie.add_macs(ck["mac1_key"][0].tobytes(), msg)
    assert cookie.check_mac1(ck, with_macs) and both(with_macs)[0] == HS_CONSUMED

    def flip(b, i):
        return b[:i] + bytes([b[i] ^ 0x10]) + b[i + 1:]
    for i, verdict, peer in ((8, ERR_AUTH, PEER_NONE), (40, ERR_AUTH, PEER_NONE), (87, ERR_AUTH, PEER_NONE),
                             (88, ERR_AUTH, 7), (115, ERR_AUTH, 7)):
        v, row = both(flip(msg, i))
        assert (v, row["peer"][0]) == (verdict, peer) and not row.tobytes()[8:].strip(b"\0")
    assert both(noise_ref.create_initiation(rng.bytes(32), ref.public, eph, ts, 1)[0])[0] == ERR_NO_PEER
    v, row = both(noise_ref.create_initiation(stopped, ref.public, eph, ts, 2)[0])
    assert (v, row["peer"][0]) == (ERR_NO_PEER, 8)
    v, row = both(noise_ref.create_initiation(init_private, ref.public, eph, ts, 3, static_public=le(1),
                                              precomputed=rng.bytes(32))[0])
    assert (v, row["peer"][0]) == (ERR_NO_PEER, 9)
    assert both(msg[:8] + le(P) + msg[40:])[0] == ERR_LOW_ORDER
    assert both(struct.pack("<I", 2) + msg[4:])[0] == ERR_INVALID_ARG
    assert both(msg[:-1])[0] == ERR_INVALID_ARG and both(msg + b"\0")[0] == ERR_INVALID_ARG
    empty = noise.peer_keys_build(r, [], [])
    assert both(msg, empty, noise_ref.PeerTable(ref, []))[0] == ERR_NO_PEER
    with pytest.raises(_lib.WgcsError) as ei:
        noise.create_initiation(init_private, le(1), eph, ts, 0)
    assert ei.value.code == ERR_LOW_ORDER
