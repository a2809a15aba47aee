"""Checker for the transport AEAD (test infrastructure only).

* A pure-Python restatement of RFC 8439 written from the RFC: ChaCha20
  vectorised over blocks with numpy (§2.3-2.4), Poly1305 in Python ints
  (§2.5), the AEAD construction (§2.8), general over nonce and AAD.
* `Libcrypto`: a ctypes wrapper of the local OpenSSL's EVP_chacha20_poly1305,
  found with ctypes.util.find_library; `libcrypto()` returns None when there
  is none (tests that need it skip).
* Restatements of padding() (device/send.go:529-560), of the receive-side
  length trim (device/receive.go:432-482), and of the transport message that
  RoutineEncryption builds and RoutineDecryption takes apart.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import struct

import numpy as np

ERR_PACKET_TOO_SHORT = -8
ERR_AUTH = -18
P1305 = (1 << 130) - 5
_SIGMA = np.frombuffer(b"expand 32-byte k", dtype="<u4")


# ------------------------------------------------------------------ ChaCha20
def _rotl(x: np.ndarray, n: int) -> np.ndarray:
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _qr(s, a, b, c, d):
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 16)
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 12)
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 8)
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 7)


def chacha20_blocks(key: bytes, nonce: bytes, counter: int, nblocks: int) -> bytes:
    """nblocks 64-byte keystream blocks from block counter `counter` (§2.3)."""
    assert len(key) == 32 and len(nonce) == 12
    init = np.empty((16, nblocks), dtype=np.uint32)
    init[0:4] = _SIGMA[:, None]
    init[4:12] = np.frombuffer(key, dtype="<u4")[:, None]
    init[12] = (counter + np.arange(nblocks, dtype=np.uint64)).astype(np.uint32)
    init[13:16] = np.frombuffer(nonce, dtype="<u4")[:, None]
    s = [init[i].copy() for i in range(16)]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(s, 0, 4, 8, 12); _qr(s, 1, 5, 9, 13); _qr(s, 2, 6, 10, 14); _qr(s, 3, 7, 11, 15)
            _qr(s, 0, 5, 10, 15); _qr(s, 1, 6, 11, 12); _qr(s, 2, 7, 8, 13); _qr(s, 3, 4, 9, 14)
        out = np.stack(s) + init
    return out.T.astype("<u4").tobytes()


def chacha20_xor(key: bytes, nonce: bytes, counter: int, data: bytes) -> bytes:
    n = len(data)
    if n == 0:
        return b""
    ks = np.frombuffer(chacha20_blocks(key, nonce, counter, (n + 63) // 64), dtype=np.uint8)[:n]
    return (np.frombuffer(data, dtype=np.uint8) ^ ks).tobytes()


# ------------------------------------------------------------------ Poly1305
def poly1305(key: bytes, msg: bytes) -> bytes:
    """§2.5.1, serial Horner in Python ints."""
    r = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(key[16:32], "little")
    acc = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        acc = (acc + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P1305
    return ((acc + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def _pad16(b: bytes) -> bytes:
    return b"\0" * (-len(b) % 16)


# ---------------------------------------------------------------------- AEAD
def aead_seal(key: bytes, nonce: bytes, plaintext: bytes, aad: bytes = b"") -> bytes:
    """chacha20_aead_encrypt of §2.8: ciphertext | tag."""
    otk = chacha20_blocks(key, nonce, 0, 1)[:32]
    ct = chacha20_xor(key, nonce, 1, plaintext)
    mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    return ct + poly1305(otk, mac)


def aead_open(key: bytes, nonce: bytes, sealed: bytes, aad: bytes = b"") -> bytes | None:
    """The plaintext, or None when the tag does not match."""
    if len(sealed) < 16:
        return None
    ct, tag = sealed[:-16], sealed[-16:]
    otk = chacha20_blocks(key, nonce, 0, 1)[:32]
    mac = aad + _pad16(aad) + ct + _pad16(ct) + struct.pack("<QQ", len(aad), len(ct))
    if poly1305(otk, mac) != tag:
        return None
    return chacha20_xor(key, nonce, 1, ct)


# ----------------------------------------------------------------- libcrypto
class Libcrypto:
    """EVP_chacha20_poly1305 of the local OpenSSL through ctypes."""

    _CTRL_SET_IVLEN, _CTRL_GET_TAG, _CTRL_SET_TAG = 0x9, 0x10, 0x11

    def __init__(self, path: str):
        L = C.CDLL(path)
        vp, i = C.c_void_p, C.c_int
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        L.EVP_chacha20_poly1305.restype = vp
        for name in ("EVP_EncryptInit_ex", "EVP_DecryptInit_ex"):
            getattr(L, name).argtypes = [vp, vp, vp, C.c_char_p, C.c_char_p]
        for name in ("EVP_EncryptUpdate", "EVP_DecryptUpdate"):
            getattr(L, name).argtypes = [vp, C.c_char_p, C.POINTER(i), C.c_char_p, i]
        for name in ("EVP_EncryptFinal_ex", "EVP_DecryptFinal_ex"):
            getattr(L, name).argtypes = [vp, C.c_char_p, C.POINTER(i)]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, i, i, vp]
        self.L = L
        self.cipher = L.EVP_chacha20_poly1305()
        if not self.cipher:
            raise OSError("EVP_chacha20_poly1305 unavailable")

    def seal(self, key: bytes, nonce: bytes, plaintext: bytes, aad: bytes = b"") -> bytes:
        L = self.L
        ctx = L.EVP_CIPHER_CTX_new()
        try:
            n = C.c_int(0)
            assert L.EVP_EncryptInit_ex(ctx, self.cipher, None, None, None) == 1
            assert L.EVP_CIPHER_CTX_ctrl(ctx, self._CTRL_SET_IVLEN, len(nonce), None) == 1
            assert L.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
            if aad:
                assert L.EVP_EncryptUpdate(ctx, None, C.byref(n), aad, len(aad)) == 1
            out = C.create_string_buffer(len(plaintext) + 16)
            assert L.EVP_EncryptUpdate(ctx, out, C.byref(n), plaintext, len(plaintext)) == 1
            got = n.value
            tail = C.create_string_buffer(16)
            assert L.EVP_EncryptFinal_ex(ctx, tail, C.byref(n)) == 1
            assert got + n.value == len(plaintext)
            tag = C.create_string_buffer(16)
            assert L.EVP_CIPHER_CTX_ctrl(ctx, self._CTRL_GET_TAG, 16, tag) == 1
            return out.raw[:len(plaintext)] + tag.raw
        finally:
            L.EVP_CIPHER_CTX_free(ctx)

    def open(self, key: bytes, nonce: bytes, sealed: bytes, aad: bytes = b"") -> bytes | None:
        if len(sealed) < 16:
            return None
        L = self.L
        ct, tag = sealed[:-16], sealed[-16:]
        ctx = L.EVP_CIPHER_CTX_new()
        try:
            n = C.c_int(0)
            assert L.EVP_DecryptInit_ex(ctx, self.cipher, None, None, None) == 1
            assert L.EVP_CIPHER_CTX_ctrl(ctx, self._CTRL_SET_IVLEN, len(nonce), None) == 1
            assert L.EVP_DecryptInit_ex(ctx, None, None, key, nonce) == 1
            if aad:
                assert L.EVP_DecryptUpdate(ctx, None, C.byref(n), aad, len(aad)) == 1
            out = C.create_string_buffer(len(ct) + 16)
            assert L.EVP_DecryptUpdate(ctx, out, C.byref(n), ct, len(ct)) == 1
            tagbuf = C.create_string_buffer(tag, 16)
            assert L.EVP_CIPHER_CTX_ctrl(ctx, self._CTRL_SET_TAG, 16, tagbuf) == 1
            tail = C.create_string_buffer(16)
            if L.EVP_DecryptFinal_ex(ctx, tail, C.byref(n)) != 1:
                return None
            return out.raw[:len(ct)]
        finally:
            L.EVP_CIPHER_CTX_free(ctx)


_libcrypto: list = []


def libcrypto() -> Libcrypto | None:
    if not _libcrypto:
        lc = None
        path = ctypes.util.find_library("crypto")
        if path:
            try:
                lc = Libcrypto(path)
            except (OSError, AttributeError):
                lc = None
        _libcrypto.append(lc)
    return _libcrypto[0]


# ------------------------------------------------- package device, restated
PADDING_MULTIPLE = 16


def padding(packet_size: int, mtu: int) -> int:
    """send.go:529-560."""
    last_unit = packet_size
    if mtu == 0:
        return ((last_unit + PADDING_MULTIPLE - 1) & ~(PADDING_MULTIPLE - 1)) - last_unit
    if last_unit > mtu:
        last_unit %= mtu
    padded_size = (last_unit + PADDING_MULTIPLE - 1) & ~(PADDING_MULTIPLE - 1)
    padded_size = min(padded_size, mtu)
    return padded_size - last_unit


def trim(packet: bytes) -> int:
    """What RoutineSendToInternet keeps of a decrypted packet (receive.go:432-482):
    its trimmed length, 0 for a keepalive, ERR_PACKET_TOO_SHORT for a `continue`."""
    if len(packet) == 0:
        return 0
    ver = packet[0] >> 4
    if ver == 4:
        if len(packet) < 20:
            return ERR_PACKET_TOO_SHORT
        length = int.from_bytes(packet[2:4], "big")
        if length > len(packet) or length < 20:
            return ERR_PACKET_TOO_SHORT
        return length
    if ver == 6:
        if len(packet) < 40:
            return ERR_PACKET_TOO_SHORT
        length = (int.from_bytes(packet[4:6], "big") + 40) & 0xFFFF  # uint16 arithmetic
        if length > len(packet):
            return ERR_PACKET_TOO_SHORT
        return length
    return ERR_PACKET_TOO_SHORT


def wg_nonce(counter: int) -> bytes:
    return b"\0\0\0\0" + struct.pack("<Q", counter)  # send.go:453


def wg_seal(key: bytes, remote_index: int, counter: int, packet: bytes, mtu: int, seal=aead_seal) -> bytes:
    """The transport message RoutineEncryption produces (send.go:438-463)."""
    padded = packet + b"\0" * padding(len(packet), mtu)
    return struct.pack("<IIQ", 4, remote_index, counter) + seal(key, wg_nonce(counter), padded)


def wg_open(key: bytes, msg: bytes, open_=aead_open) -> tuple[int, bytes | None]:
    """(counter, plaintext or None) of a transport message (receive.go:363-383)."""
    counter = struct.unpack_from("<Q", msg, 8)[0]
    return counter, open_(key, wg_nonce(counter), msg[16:])
