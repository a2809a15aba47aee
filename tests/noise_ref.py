"""Checker for X25519 and the handshake consume step (test infrastructure only).

* X25519 from RFC 7748 §5 in Python integers: decodeScalar25519,
  decodeUCoordinate, the Montgomery ladder with its cswap, and the inversion
  as pow(z, p - 2, p).  Like golang.org/x/crypto/curve25519.X25519 it returns
  None ("low order point") for an all-zero result.
* A restatement of the reference's Noise layer (device/noise.go:91-94,
  :324-457, device/noise_helpers.go:18-58) over hashlib.blake2s, hmac and the
  RFC 8439 AEAD of tests/aead_ref.py.
tests/test_noise_ref.py pins both to published vectors and to OpenSSL's output
(tests/golden/x25519_vectors.json) before anything is compared with them.
"""
from __future__ import annotations

import hashlib
import hmac
import struct

import aead_ref

P = 2**255 - 19
A24 = 121665
HS_NONE, HS_PASS, HS_CONSUMED = 0, 1, 3
ERR_INVALID_ARG, ERR_AUTH, ERR_LOW_ORDER, ERR_NO_PEER = -1, -18, -22, -23
PEER_NONE = 0xFFFFFFFF
INITIATION_SIZE = 148
BASE_POINT = (9).to_bytes(32, "little")
ZERO_NONCE = bytes(12)
NOISE_CONSTRUCTION = b"Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s"
WG_IDENTIFIER = b"WireGuard v1 zx2c4 Jason@zx2c4.com"


# -------------------------------------------------------------------- RFC 7748
def decode_scalar(k: bytes) -> int:
    b = bytearray(k)
    b[0] &= 248
    b[31] &= 127
    b[31] |= 64
    return int.from_bytes(b, "little")


def decode_u(u: bytes) -> int:
    b = bytearray(u)
    b[31] &= 127  # "mask the most significant bit in the final byte"
    return int.from_bytes(b, "little")  # a non-canonical value is accepted: arithmetic is mod p


def x25519_raw(k: bytes, u: bytes) -> bytes:
    """The 32 output bytes of RFC 7748 §5, all zero included."""
    assert len(k) == 32 and len(u) == 32
    kk, x1 = decode_scalar(k), decode_u(u) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (kk >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a = (x2 + z2) % P
        aa = a * a % P
        b = (x2 - z2) % P
        bb = b * b % P
        e = (aa - bb) % P
        c = (x3 + z3) % P
        d = (x3 - z3) % P
        da = d * a % P
        cb = c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def x25519(k: bytes, u: bytes) -> bytes | None:
    """curve25519.X25519: None where the result is all zero."""
    out = x25519_raw(k, u)
    return None if out == bytes(32) else out


def public_key(private: bytes) -> bytes:
    return x25519_raw(private, BASE_POINT)


# ------------------------------------------------------- noise_helpers.go:18-58
def hash256(data: bytes) -> bytes:
    return hashlib.blake2s(data, digest_size=32).digest()


def hmac_b2s(key: bytes, *parts: bytes) -> bytes:
    """HMAC1 / HMAC2: HMAC over unkeyed BLAKE2s-256 (64-byte block)."""
    return hmac.new(key, b"".join(parts), lambda: hashlib.blake2s(digest_size=32)).digest()


def kdf1(key: bytes, data: bytes) -> bytes:
    return hmac_b2s(hmac_b2s(key, data), b"\x01")


def kdf2(key: bytes, data: bytes) -> tuple[bytes, bytes]:
    prk = hmac_b2s(key, data)
    t0 = hmac_b2s(prk, b"\x01")
    return t0, hmac_b2s(prk, t0, b"\x02")


def kdf3(key: bytes, data: bytes) -> tuple[bytes, bytes, bytes]:
    prk = hmac_b2s(key, data)
    t0 = hmac_b2s(prk, b"\x01")
    t1 = hmac_b2s(prk, t0, b"\x02")
    return t0, t1, hmac_b2s(prk, t1, b"\x03")


def mix_hash(h: bytes, data: bytes) -> bytes:
    return hash256(h + data)


INITIAL_CHAIN_KEY = hash256(NOISE_CONSTRUCTION)                 # noise.go:92
INITIAL_HASH = mix_hash(INITIAL_CHAIN_KEY, WG_IDENTIFIER)       # :93


# --------------------------------------------------------------- noise.go:344-457
class Responder:
    """d.keys, with what wgcs_noise_responder holds."""

    def __init__(self, private: bytes):
        self.private = private
        self.public = public_key(private)
        self.hash0 = mix_hash(INITIAL_HASH, self.public)
        self.chain0 = INITIAL_CHAIN_KEY

    def tobytes(self) -> bytes:
        return self.private + self.hash0 + self.chain0


class PeerTable:
    """GetPeer: rows (public key, shared, peer id, flags) sorted by public key."""

    def __init__(self, responder: Responder, peers):
        """peers: (public key, peer id, flags) triples."""
        self.rows = sorted(((pub, x25519_raw(responder.private, pub), pid, flags) for pub, pid, flags in peers),
                           key=lambda r: r[0])

    def find(self, pub: bytes):
        for i, row in enumerate(self.rows):
            if row[0] == pub:
                return i
        return -1

    def tobytes(self) -> bytes:
        return b"".join(pub + shared + struct.pack("<II", pid, flags) for pub, shared, pid, flags in self.rows)


def hs_init_bytes(peer: int, sender: int, timestamp: bytes = bytes(12), h: bytes = bytes(32), chain: bytes = bytes(32),
                  ephemeral: bytes = bytes(32)) -> bytes:
    """One wgcs_hs_init row."""
    return struct.pack("<II", peer, sender) + timestamp + bytes(12) + h + chain + ephemeral


def create_initiation(static_private: bytes, remote_static: bytes, ephemeral_private: bytes, timestamp: bytes,
                      sender: int, static_public: bytes | None = None, precomputed: bytes | None = None):
    """CreateMessageInitiation (noise.go:344-403) with the caller's ephemeral
    key, timestamp and sender index: (the 148 bytes with zero MACs, hash, chain
    key), or None where a shared secret is zero.  `static_public` and
    `precomputed` replace the sender's own public key and its static-static
    secret: how a test makes an initiator whose public key is a low-order point."""
    h = mix_hash(INITIAL_HASH, remote_static)
    chain = INITIAL_CHAIN_KEY
    eph = public_key(ephemeral_private)
    chain = kdf1(chain, eph)
    h = mix_hash(h, eph)
    shared = x25519(ephemeral_private, remote_static)
    if shared is None:
        return None
    chain, key = kdf2(chain, shared)
    static_public = public_key(static_private) if static_public is None else static_public
    static = aead_ref.aead_seal(key, ZERO_NONCE, static_public, h)
    h = mix_hash(h, static)
    if precomputed is None:
        precomputed = x25519_raw(static_private, remote_static)
    if precomputed == bytes(32):
        return None
    chain, key = kdf2(chain, precomputed)
    ts = aead_ref.aead_seal(key, ZERO_NONCE, timestamp, h)
    h = mix_hash(h, ts)
    return struct.pack("<II", 1, sender) + eph + static + ts + bytes(32), h, chain


def consume_initiation(responder: Responder, table: PeerTable, msg: bytes | None):
    """(verdict, the wgcs_hs_init row or None where it stays untouched) of
    ConsumeMessageInitiation up to noise.go:457 for a row that was selected."""
    if msg is None or len(msg) != INITIATION_SIZE or struct.unpack_from("<I", msg)[0] != 1:
        return ERR_INVALID_ARG, None
    sender = struct.unpack_from("<I", msg, 4)[0]
    eph, static, ts = msg[8:40], msg[40:88], msg[88:116]
    h = mix_hash(responder.hash0, eph)
    chain = kdf1(responder.chain0, eph)
    shared = x25519(responder.private, eph)
    if shared is None:
        return ERR_LOW_ORDER, hs_init_bytes(PEER_NONE, sender)
    chain, key = kdf2(chain, shared)
    peer_pub = aead_ref.aead_open(key, ZERO_NONCE, static, h)
    if peer_pub is None:
        return ERR_AUTH, hs_init_bytes(PEER_NONE, sender)
    h = mix_hash(h, static)
    row = table.find(peer_pub)
    if row < 0:
        return ERR_NO_PEER, hs_init_bytes(PEER_NONE, sender)
    _, precomputed, pid, flags = table.rows[row]
    if not flags & 1 or precomputed == bytes(32):
        return ERR_NO_PEER, hs_init_bytes(pid, sender)
    chain, key = kdf2(chain, precomputed)
    timestamp = aead_ref.aead_open(key, ZERO_NONCE, ts, h)
    if timestamp is None:
        return ERR_AUTH, hs_init_bytes(pid, sender)
    h = mix_hash(h, ts)
    return HS_CONSUMED, hs_init_bytes(pid, sender, timestamp, h, chain, eph)


def consume_row(responder: Responder, table: PeerTable, type_: int, gate: int | None, msg: bytes | None):
    """One row of wgcs_handshake_consume_batch: gate None stands for d_gate == NULL."""
    if type_ != 1 or (gate is not None and gate != HS_PASS):
        return HS_NONE, None
    return consume_initiation(responder, table, msg)


# the low-order u of RFC 7748 §6.1's check, and their non-canonical forms below 2^255
LOW_ORDER_POINTS = [(0).to_bytes(32, "little"), (1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little"),
                    P.to_bytes(32, "little"), (P + 1).to_bytes(32, "little")]
