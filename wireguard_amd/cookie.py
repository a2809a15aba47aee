"""Host-side mirror of the reference's cookie checker and generator (package
`device`, cookie.go) over the C ABI -- SURVEY.md §8 row f6.

Names and argument meaning follow the reference:
  checker_init(pub)                               CookieChecker.Init / CookieGenerator.Init, cookie.go:102-115
  check_mac1 / check_mac2                         CheckMAC1 / CheckMAC2, :121-176
  create_reply                                    CreateReply + SendHandshakeCookie, :184-243, send.go:176-187
  add_macs                                        AddMACs, :287-314
  consume_reply                                   ConsumeReply, :319-339
  src_addr(ip, port)                              Endpoint.DstToBytes()
  screen_batch                                    the top of RoutineHandshake, receive.go:270-287
The clock and the randomness are the caller's: draw a new `secret` (32 random
bytes) whenever the one in the checker is 120 s old, before a check or a batch,
and hand every reply its own 24 random nonce bytes.  BLAKE2s, XChaCha20-Poly1305
and the kernel live in libwgcsum.so (wgcs_blake2s.h, wgcs_xchacha.h,
cookie_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import ctypes as C
import ipaddress
import struct

import numpy as np

from . import _lib
from ._lib import ERR_MAC1, HS_COOKIE, HS_NONE, HS_PASS, WgcsError
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import _ptr

COOKIE_CHECKER_DTYPE = np.dtype([("mac1_key", "u1", (32,)), ("cookie_key", "u1", (32,)),
                                 ("secret", "u1", (32,))])  # wgcs_cookie_checker
SRC_ADDR_DTYPE = np.dtype([("b", "u1", (18,)), ("len", "u1"), ("pad", "u1")])  # wgcs_src_addr

__all__ = ["COOKIE_CHECKER_DTYPE", "SRC_ADDR_DTYPE", "checker_init", "check_mac1", "check_mac2", "create_reply",
           "add_macs", "consume_reply", "src_addr", "screen_batch", "HS_NONE", "HS_PASS", "HS_COOKIE", "ERR_MAC1"]


def _status(rc: int, what: str) -> int:
    if rc < 0:
        raise WgcsError(rc, f"{what}: {_lib.load().wgcs_strerror(rc).decode()}")
    return rc


def _fixed(b, n: int, what: str) -> bytes:
    b = bytes(b)
    if len(b) != n:
        raise ValueError(f"{what} is {n} bytes, not {len(b)}")
    return b


def _checker(checker) -> np.ndarray:
    ck = np.ascontiguousarray(checker, dtype=COOKIE_CHECKER_DTYPE).reshape(-1)
    if len(ck) != 1:
        raise ValueError("one COOKIE_CHECKER_DTYPE row")
    return ck


def _src(src) -> np.ndarray:
    s = np.ascontiguousarray(src, dtype=SRC_ADDR_DTYPE).reshape(-1)
    if len(s) != 1:
        raise ValueError("one SRC_ADDR_DTYPE row")
    return s


def checker_init(pub, secret=None) -> np.ndarray:
    """One COOKIE_CHECKER_DTYPE row for the static public key `pub`: the keys of
    both the checker and the generator.  `secret` (32 bytes) defaults to zeros."""
    ck = np.zeros(1, COOKIE_CHECKER_DTYPE)
    _status(_lib.load().wgcs_cookie_checker_init(ck.ctypes.data, _fixed(pub, 32, "a public key")),
            "wgcs_cookie_checker_init")
    if secret is not None:
        ck["secret"][0] = np.frombuffer(_fixed(secret, 32, "a secret"), dtype=np.uint8)
    return ck


def src_addr(ip, port: int) -> np.ndarray:
    """One SRC_ADDR_DTYPE row: the address bytes (4 or 16) then the port as LE16."""
    if isinstance(ip, str):
        ip = ipaddress.ip_address(ip)
    a = ip.packed if isinstance(ip, (ipaddress.IPv4Address, ipaddress.IPv6Address)) else bytes(ip)
    if len(a) not in (4, 16) or not 0 <= port <= 0xFFFF:
        raise ValueError("an address of 4 or 16 bytes and a 16-bit port")
    row = np.zeros(1, SRC_ADDR_DTYPE)
    b = a + struct.pack("<H", port)
    row["b"][0, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    row["len"] = len(b)
    return row


def check_mac1(checker, msg) -> bool:
    ck, m = _checker(checker), bytes(msg)
    return bool(_status(_lib.load().wgcs_cookie_check_mac1(ck.ctypes.data, m, len(m)), "wgcs_cookie_check_mac1"))


def check_mac2(checker, msg, src) -> bool:
    ck, m, s = _checker(checker), bytes(msg), _src(src)
    return bool(_status(_lib.load().wgcs_cookie_check_mac2(ck.ctypes.data, m, len(m), s.ctypes.data),
                        "wgcs_cookie_check_mac2"))


def create_reply(checker, msg, src, nonce) -> bytes:
    """The 64-byte MessageCookieReply for `msg` from `src` with the caller's 24 nonce bytes."""
    ck, m, s = _checker(checker), bytes(msg), _src(src)
    out = C.create_string_buffer(64)
    _status(_lib.load().wgcs_cookie_create_reply(ck.ctypes.data, m, len(m), s.ctypes.data, _fixed(nonce, 24, "a nonce"),
                                                 out), "wgcs_cookie_create_reply")
    return out.raw


def add_macs(mac1_key, msg, cookie=None) -> tuple[bytes, bytes]:
    """(the message with MAC1 -- and, given a 16-byte cookie, MAC2 -- filled in, that MAC1)."""
    buf = C.create_string_buffer(bytes(msg), len(msg))
    last = C.create_string_buffer(16)
    ck = None if cookie is None else _fixed(cookie, 16, "a cookie")
    _status(_lib.load().wgcs_cookie_add_macs(_fixed(mac1_key, 32, "a mac1 key"), ck, buf, len(msg), last),
            "wgcs_cookie_add_macs")
    return buf.raw, last.raw


def consume_reply(cookie_key, last_mac1, reply) -> bytes | None:
    """The cookie of a reply that opens, else None."""
    out = C.create_string_buffer(16)
    rc = _status(_lib.load().wgcs_cookie_consume_reply(_fixed(cookie_key, 32, "a cookie key"),
                                                       _fixed(last_mac1, 16, "a MAC1"),
                                                       _fixed(reply, 64, "a cookie reply"), out),
                 "wgcs_cookie_consume_reply")
    return out.raw if rc else None


def screen_batch(dev, arena, pkts, types, checker, src, verdict, under_load: bool = False, nonce=None, reply=None,
                 stream=None, n: int | None = None) -> None:
    """Asynchronous wgcs_handshake_screen_batch over classify_batch's pkts
    (AEAD_PKT_DTYPE rows) and types (int32): verdict[q] (int32) = HS_NONE,
    HS_PASS, HS_COOKIE, ERR_MAC1 or ERR_INVALID_ARG.  checker is one
    COOKIE_CHECKER_DTYPE row and src SRC_ADDR_DTYPE rows on the device; under
    load, nonce holds 24 bytes and reply receives 64 bytes per row."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    dev._check(dev.lib.wgcs_handshake_screen_batch(dev.h, _ptr(arena), _ptr(pkts), _ptr(types), n, _ptr(checker),
                                                   _ptr(src), 1 if under_load else 0, _ptr(nonce), _ptr(verdict),
                                                   _ptr(reply), s))
