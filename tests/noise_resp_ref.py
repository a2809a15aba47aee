"""Checker for the handshake response (test infrastructure only): a Python
restatement of the reference's CreateMessageResponse (device/noise.go:494-546),
ConsumeMessageResponse (:548-620, the cryptography at :573-604), the key
derivation of BeginSymmetricSession (:636-655) and AddMACs
(device/cookie.go:287-314), and of one row of wgcs_handshake_respond_batch.

It is built on tests/noise_ref.py (X25519, the HMAC / HKDF layer),
tests/aead_ref.py (the RFC 8439 AEAD) and tests/cookie_ref.py (the MACs), which
their own tests pin to published vectors; tests/test_noise_resp_ref.py rebuilds
every step from hashlib and hmac before anything is compared with this file.
"""
from __future__ import annotations

import struct

import aead_ref
import cookie_ref
import noise_ref
from noise_ref import (ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, ERR_NO_PEER, HS_CONSUMED, HS_NONE, ZERO_NONCE, kdf1, kdf2,
                       kdf3, mix_hash, public_key, x25519)

HS_RESPONDED = 4
RESPONSE_SIZE, RESPONSE_PITCH = 92, 96
RESP_COOKIE = 1  # wgcs_hs_resp.flags bit 0
ZERO_PSK = bytes(32)


def mac1_key(remote_static: bytes) -> bytes:
    """CookieGenerator.Init (cookie.go:269-277): the MAC1 key for messages to the holder of remote_static."""
    return cookie_ref.hash256(b"mac1----" + remote_static)


def create_response_core(h: bytes, chain: bytes, remote_ephemeral: bytes, remote_static: bytes, psk: bytes,
                         ephemeral_private: bytes, local_index: int, remote_index: int):
    """noise.go:508-545: (the 60 bytes before the MACs, hash, chaining key) after
    the message, or None where a shared secret is zero (:520-528)."""
    eph = public_key(ephemeral_private)                       # :517
    h = mix_hash(h, eph)                                      # :518
    chain = kdf1(chain, eph)                                  # :519
    shared = x25519(ephemeral_private, remote_ephemeral)      # :520
    if shared is None:
        return None
    chain = kdf1(chain, shared)                               # :524
    shared = x25519(ephemeral_private, remote_static)         # :525
    if shared is None:
        return None
    chain = kdf1(chain, shared)                               # :529
    chain, tau, key = kdf3(chain, psk)                        # :533-539
    h = mix_hash(h, tau)                                      # :540
    empty = aead_ref.aead_seal(key, ZERO_NONCE, b"", h)       # :542
    h = mix_hash(h, empty)                                    # :543
    return struct.pack("<III", 2, local_index, remote_index) + eph + empty, h, chain


def responder_keys(chain: bytes) -> tuple[bytes, bytes]:
    """BeginSymmetricSession for handshakeResponseCreated (noise.go:645-652): (send = encrypt, recv = decrypt)."""
    decrypt, encrypt = kdf2(chain, b"")
    return encrypt, decrypt


def initiator_keys(chain: bytes) -> tuple[bytes, bytes]:
    """BeginSymmetricSession for handshakeResponseConsumed (:637-644): (send = encrypt, recv = decrypt)."""
    encrypt, decrypt = kdf2(chain, b"")
    return encrypt, decrypt


def create_response(init_row: bytes, remote_static: bytes, ephemeral_private: bytes, local_index: int,
                    psk: bytes | None = None, cookie: bytes | None = None):
    """wgcs_noise_create_response for one wgcs_hs_init row (128 bytes):
    (status, the 92 bytes with their MACs, send key, recv key, hash, chaining
    key); zeros and None for the last two where a shared secret is zero."""
    sender = struct.unpack_from("<I", init_row, 4)[0]
    h, chain, remote_eph = init_row[32:64], init_row[64:96], init_row[96:128]
    core = create_response_core(h, chain, remote_eph, remote_static, ZERO_PSK if psk is None else psk,
                                ephemeral_private, local_index, sender)
    if core is None:
        return ERR_LOW_ORDER, bytes(92), bytes(32), bytes(32), None, None
    body, h, chain = core
    msg, _ = cookie_ref.add_macs(mac1_key(remote_static), body + bytes(32), cookie)  # AddMACs; MAC2 stays zero without
    send, recv = responder_keys(chain)
    return 0, msg, send, recv, h, chain


def consume_response(static_private: bytes, h: bytes, chain: bytes, ephemeral_private: bytes, local_index: int,
                     msg: bytes, psk: bytes | None = None):
    """wgcs_noise_consume_response: (status, sender, send key, recv key, hash,
    chaining key), with None / zero keys where it fails.  sessions.Get(msg.Receiver)
    is the comparison with local_index (noise.go:553-557)."""
    fail = (None, bytes(32), bytes(32), None, None)
    if len(msg) != RESPONSE_SIZE:
        return (ERR_INVALID_ARG,) + fail
    type_, sender, receiver = struct.unpack_from("<III", msg)
    if type_ != 2 or receiver != local_index:                 # :549-557
        return (ERR_INVALID_ARG,) + fail
    eph, empty = msg[12:44], msg[44:60]
    h = mix_hash(h, eph)                                      # :573
    chain = kdf1(chain, eph)                                  # :574
    shared = x25519(ephemeral_private, eph)                   # :575
    if shared is None:
        return (ERR_LOW_ORDER,) + fail
    chain = kdf1(chain, shared)                               # :579
    shared = x25519(static_private, eph)                      # :581
    if shared is None:
        return (ERR_LOW_ORDER,) + fail
    chain = kdf1(chain, shared)                               # :585
    chain, tau, key = kdf3(chain, ZERO_PSK if psk is None else psk)  # :590-596
    h = mix_hash(h, tau)                                      # :597
    if aead_ref.aead_open(key, ZERO_NONCE, empty, h) is None:  # :599-603
        return (ERR_AUTH,) + fail
    h = mix_hash(h, empty)                                    # :604
    send, recv = initiator_keys(chain)
    return 0, sender, send, recv, h, chain


def aead_key_bytes(key: bytes, remote_index: int) -> bytes:
    """One wgcs_aead_key row."""
    return key + struct.pack("<I", remote_index) + bytes(12)


def respond_row(desc: dict, init_rows: list[bytes], gate, table_rows, psks, n_keys: int):
    """One descriptor of wgcs_handshake_respond_batch: (status, the 96-byte
    message row or None where it stays untouched, {key row: 48 bytes}).
    desc has the fields of wgcs_hs_resp; gate None stands for d_gate == NULL,
    psks None for d_psk == NULL; table_rows are (public key, shared, peer id,
    flags) as noise_ref.PeerTable.rows."""
    i, p, s, r = desc["init_row"], desc["peer_row"], desc["send_key"], desc["recv_key"]
    if i >= len(init_rows) or p >= len(table_rows) or s >= n_keys or r >= n_keys or s == r:
        return ERR_INVALID_ARG, None, {}
    if gate is not None and gate[i] != HS_CONSUMED:
        return HS_NONE, None, {}
    row = init_rows[i]
    if struct.unpack_from("<I", row)[0] != table_rows[p][2]:
        return ERR_NO_PEER, None, {}
    cookie = desc["cookie"] if desc["flags"] & RESP_COOKIE else None
    status, msg, send, recv, _, _ = create_response(row, table_rows[p][0], desc["ephemeral_private"], desc["local_index"],
                                                    None if psks is None else psks[p], cookie)
    if status != 0:
        return status, bytes(RESPONSE_PITCH), {}
    sender = struct.unpack_from("<I", row, 4)[0]
    return HS_RESPONDED, msg + bytes(4), {s: aead_key_bytes(send, sender), r: aead_key_bytes(recv, 0)}
