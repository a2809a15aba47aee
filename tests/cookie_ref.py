"""Checker for the handshake screen (test infrastructure only): a Python
restatement of the reference's cookie checker and generator (device/cookie.go)
and of the screen at the top of RoutineHandshake (device/receive.go:270-287).

BLAKE2s is hashlib's; HChaCha20 is written on aead_ref's quarter round, and the
XChaCha20-Poly1305 seal / open is aead_ref's RFC 8439 AEAD under the HChaCha20
subkey (draft-irtf-cfrg-xchacha-03 §2).  tests/test_cookie_ref.py pins all of
it to published vectors before anything is compared with it.
"""
from __future__ import annotations

import hashlib
import struct

import numpy as np

import aead_ref

HS_NONE, HS_PASS, HS_COOKIE = 0, 1, 2
ERR_INVALID_ARG = -1
ERR_MAC1 = -21
INITIATION_SIZE, RESPONSE_SIZE, COOKIE_REPLY_SIZE = 148, 92, 64  # device/noise.go
SIZE_OF_TYPE = {1: INITIATION_SIZE, 2: RESPONSE_SIZE}


def mac128(key: bytes, data: bytes) -> bytes:
    return hashlib.blake2s(data, key=key, digest_size=16).digest()


def hash256(data: bytes) -> bytes:
    return hashlib.blake2s(data, digest_size=32).digest()


# ------------------------------------------------------------------ XChaCha20
def hchacha20(key: bytes, nonce16: bytes) -> bytes:
    """draft-irtf-cfrg-xchacha §2.2: rows 0 and 3 of the permuted state."""
    assert len(key) == 32 and len(nonce16) == 16
    words = np.concatenate([aead_ref._SIGMA, np.frombuffer(key, dtype="<u4"), np.frombuffer(nonce16, dtype="<u4")])
    s = [np.array([w], dtype=np.uint32) for w in words]
    with np.errstate(over="ignore"):
        for _ in range(10):
            aead_ref._qr(s, 0, 4, 8, 12); aead_ref._qr(s, 1, 5, 9, 13)
            aead_ref._qr(s, 2, 6, 10, 14); aead_ref._qr(s, 3, 7, 11, 15)
            aead_ref._qr(s, 0, 5, 10, 15); aead_ref._qr(s, 1, 6, 11, 12)
            aead_ref._qr(s, 2, 7, 8, 13); aead_ref._qr(s, 3, 4, 9, 14)
    return b"".join(struct.pack("<I", int(s[i][0])) for i in (0, 1, 2, 3, 12, 13, 14, 15))


def xseal(key: bytes, nonce24: bytes, plaintext: bytes, aad: bytes = b"") -> bytes:
    assert len(nonce24) == 24
    return aead_ref.aead_seal(hchacha20(key, nonce24[:16]), b"\0\0\0\0" + nonce24[16:], plaintext, aad)


def xopen(key: bytes, nonce24: bytes, sealed: bytes, aad: bytes = b"") -> bytes | None:
    assert len(nonce24) == 24
    return aead_ref.aead_open(hchacha20(key, nonce24[:16]), b"\0\0\0\0" + nonce24[16:], sealed, aad)


# ------------------------------------------------------------- cookie.go, restated
class Checker:
    """CookieChecker with the caller's secret (the clock is the caller's)."""

    def __init__(self, pub: bytes, secret: bytes = bytes(32)):
        self.mac1_key = hash256(b"mac1----" + pub)
        self.cookie_key = hash256(b"cookie--" + pub)
        self.secret = secret

    def tobytes(self) -> bytes:
        return self.mac1_key + self.cookie_key + self.secret

    def check_mac1(self, msg: bytes) -> bool:
        return mac128(self.mac1_key, msg[:-32]) == msg[-32:-16]

    def cookie(self, src: bytes) -> bytes:
        return mac128(self.secret, src)

    def check_mac2(self, msg: bytes, src: bytes) -> bool:
        return mac128(self.cookie(src), msg[:-16]) == msg[-16:]

    def create_reply(self, msg: bytes, src: bytes, nonce24: bytes) -> bytes:
        return struct.pack("<I", 3) + msg[4:8] + nonce24 + xseal(self.cookie_key, nonce24, self.cookie(src), msg[-32:-16])


def add_macs(mac1_key: bytes, msg: bytes, cookie: bytes | None = None) -> tuple[bytes, bytes]:
    """AddMACs: (the message, its MAC1); without a cookie the MAC2 field stays."""
    mac1 = mac128(mac1_key, msg[:-32])
    msg = msg[:-32] + mac1 + msg[-16:]
    if cookie is not None:
        msg = msg[:-16] + mac128(cookie, msg[:-16])
    return msg, mac1


def consume_reply(cookie_key: bytes, last_mac1: bytes, reply: bytes) -> bytes | None:
    return xopen(cookie_key, reply[8:32], reply[32:64], last_mac1)


def src_bytes(ip: bytes, port: int) -> bytes:
    return ip + struct.pack("<H", port)


def screen(ck: Checker, type_: int, msg: bytes | None, src: bytes, under_load: bool, nonce24: bytes):
    """(verdict, reply or None) of one row of wgcs_handshake_screen_batch; msg is
    the row's len bytes (None where it must not be read)."""
    if type_ not in (1, 2):
        return HS_NONE, None
    if msg is None or len(msg) != SIZE_OF_TYPE[type_]:
        return ERR_INVALID_ARG, None
    if not ck.check_mac1(msg):
        return ERR_MAC1, None
    if not under_load:
        return HS_PASS, None
    if len(src) not in (6, 18):
        return ERR_INVALID_ARG, None
    if ck.check_mac2(msg, src):
        return HS_PASS, None
    return HS_COOKIE, ck.create_reply(msg, src, nonce24)


def handshake_message(rng: np.random.Generator, type_: int, mac1_key: bytes, cookie: bytes | None = None) -> bytes:
    """A random initiation (1) or response (2) with MAC1 -- and, given a cookie, MAC2 -- in place."""
    body = struct.pack("<I", type_) + rng.bytes(SIZE_OF_TYPE[type_] - 4 - 32) + bytes(32)
    return add_macs(mac1_key, body, cookie)[0]
