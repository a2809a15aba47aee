"""Checker for the cookie generator (test infrastructure only): a literal
restatement of CookieGenerator (device/cookie.go:247-339) on tests/cookie_ref.py
under a passed-in clock, taken message by message, and of the cookie-reply case
of RoutineHandshake (device/receive.go:246-269) over plain dicts.

The reference keeps no "valid" bit: AddMACs compares time.Since(cookieSetAt)
with CookieRefreshTime whenever it writes a message (:306).  `cookie_for(now)`
is that check; a zero time.Time is None here and is older than anything.
"""
from __future__ import annotations

import struct

import cookie_ref

HS_NONE, HS_COOKIE_KEPT = 0, 10
ERR_INVALID_ARG, ERR_AUTH, ERR_NO_PEER, ERR_NO_HANDSHAKE = -1, -18, -23, -24
COOKIE_REFRESH_NS = 120 * 10**9  # CookieRefreshTime, cookie.go:17
COOKIE_REPLY_TYPE, COOKIE_REPLY_SIZE = 3, 64  # device/noise.go


class CookieGenerator:
    """cookie.go:247-339.  The clock is passed in as nanoseconds."""

    def __init__(self, pk: bytes):  # Init, :269-282
        self.mac1_key = cookie_ref.hash256(b"mac1----" + pk)
        self.encryption_key = cookie_ref.hash256(b"cookie--" + pk)
        self.cookie = bytes(16)
        self.cookie_set_at: int | None = None  # the zero time.Time
        self.has_last_mac1 = False
        self.last_mac1 = bytes(16)

    def cookie_for(self, now: int) -> bytes | None:
        """:306: the cookie AddMACs would key MAC2 with at `now`, or None."""
        if self.cookie_set_at is None or now - self.cookie_set_at > COOKIE_REFRESH_NS:
            return None
        return self.cookie

    def add_macs(self, msg: bytes, now: int) -> bytes:  # :287-314
        mac1 = cookie_ref.mac128(self.mac1_key, msg[:-32])
        msg = msg[:-32] + mac1 + msg[-16:]
        self.last_mac1 = mac1  # :301
        self.has_last_mac1 = True  # :302
        cookie = self.cookie_for(now)
        if cookie is None:  # :306-308
            return msg
        return msg[:-16] + cookie_ref.mac128(cookie, msg[:-16])  # :309-313

    def sent(self, mac1: bytes) -> None:
        """:301-302 alone, for a message whose MAC1 is already in place."""
        self.last_mac1 = mac1
        self.has_last_mac1 = True

    def consume_reply(self, nonce: bytes, sealed: bytes, now: int) -> int:  # :319-339
        if not self.has_last_mac1:  # :323-325
            return ERR_NO_HANDSHAKE
        cookie = cookie_ref.xopen(self.encryption_key, nonce, sealed, self.last_mac1)  # :326-332
        if cookie is None:  # :333-335
            return ERR_AUTH
        self.cookie_set_at = now  # :337
        self.cookie = cookie  # :338
        return HS_COOKIE_KEPT


def receive_cookie_reply(type_: int, msg: bytes | None, index_table: dict, generators: list, now: int) -> int:
    """receive.go:246-269 for one element of the handshake queue.  `type_` is
    what the classify step made of the message, `msg` its bytes (None where
    they must not be read), `index_table` {local index: peer row} -- what
    d.indexTable.Lookup finds, for handshakes and keypairs alike, with only
    the indices whose entry has a peer -- and `generators` one CookieGenerator
    per peer row."""
    if type_ != COOKIE_REPLY_TYPE:
        return HS_NONE
    if msg is None or len(msg) != COOKIE_REPLY_SIZE:  # :249-253: unmarshal
        return ERR_INVALID_ARG
    mtype, receiver = struct.unpack_from("<II", msg)
    if mtype != COOKIE_REPLY_TYPE:
        return ERR_INVALID_ARG
    row = index_table.get(receiver)  # :255
    if row is None:  # :256-258; isRunning (:259) is the caller's
        return ERR_NO_PEER
    return generators[row].consume_reply(msg[8:32], msg[32:64], now)  # :263


def seal_reply(encryption_key: bytes, receiver: int, nonce: bytes, cookie: bytes, mac1: bytes) -> bytes:
    """The MessageCookieReply a responder with that cookie key sends for a message with that MAC1."""
    return struct.pack("<II", COOKIE_REPLY_TYPE, receiver) + nonce + cookie_ref.xseal(encryption_key, nonce, cookie, mac1)
