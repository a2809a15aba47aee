"""Host-side mirror of X25519 and of the stateless part of the reference's
Noise handshake (package `device`, noise.go and noise_helpers.go) over the C ABI.

Names and argument meaning follow the reference:
  x25519(scalar, point)                           curve25519.X25519, noise_helpers.go:93-105
  responder_init(private)                         d.keys and the first mixHash, noise.go:91-94, :415
  peer_keys_build(responder, keys, peers, flags)  the table GetPeer reads, with precomputedSharedSecret, :305, :432
  consume_initiation                              ConsumeMessageInitiation up to the replay / flood check, :405-457
  create_initiation                               CreateMessageInitiation, :344-403
  create_response                                 CreateMessageResponse, AddMACs and the responder's
                                                  BeginSymmetricSession keys, :494-546, :646-651
  consume_response                                ConsumeMessageResponse and the initiator's keys, :548-620, :638-643
  x25519_batch / consume_batch / respond_batch    the same over device-resident rows
  initiate_batch / finish_batch                   CreateMessageInitiation with AddMACs, and ConsumeMessageResponse
                                                  with the initiator's keys, over device-resident rows joined by
                                                  a table of HS_STATE_DTYPE rows, :344-403, :548-620, :636-662
  initiate_host / finish_host                     those two on host memory (numpy arrays), row by row
  peer_rows_build(table, n_ids)                   peer id -> row of the peer table
  accept_batch / accept_host                      what follows noise.go:457 -- the comparison with lastTimestamp,
                                                  the flood rule, the state update -- over consume_batch's rows
                                                  and a table of HS_PEER_DTYPE rows; out come the HS_RESP_DTYPE
                                                  descriptors respond_batch takes, :458-491
The clock and the randomness are the caller's: the ephemeral private keys, the
timestamp, the session indices and `now` are arguments, the first three of the
responder's side as a pool of HS_TICKET_DTYPE rows.
Curve25519, the HMAC / HKDF layer, the AEAD and the kernels live in
libwgcsum.so (wgcs_x25519.h, wgcs_noise.h, noise_kernels.hip); nothing here
computes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ERR_AUTH, ERR_BATCH_FULL, ERR_FLOOD, ERR_LOW_ORDER, ERR_NO_HANDSHAKE, ERR_NO_PEER, ERR_REPLAY,
                   HS_ACCEPTED, HS_CONSUMED, HS_FINISHED, HS_INITIATED, HS_NONE, HS_PASS, HS_PEER_CONSUMED, HS_PEER_COOKIE,
                   HS_PEER_SEEN, HS_PEER_ZEROED, HS_RESP_COOKIE, HS_RESPONDED, HS_START_COOKIE, HS_STATE_INITIATED,
                   HS_STATE_ZEROED, PEER_NONE, PEER_RUNNING)
from .cookie import _fixed, _status
from .router import SESSION_SLOT_DTYPE
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE, _rows
from .tun import _ptr

NOISE_RESPONDER_DTYPE = np.dtype([("private_key", "u1", (32,)), ("hash0", "u1", (32,)),
                                  ("chain0", "u1", (32,))])  # wgcs_noise_responder
PEER_KEY_DTYPE = np.dtype([("public_key", "u1", (32,)), ("shared", "u1", (32,)), ("peer", "<u4"),
                           ("flags", "<u4")])  # wgcs_peer_key
HS_INIT_DTYPE = np.dtype([("peer", "<u4"), ("sender", "<u4"), ("timestamp", "u1", (12,)), ("pad", "u1", (12,)),
                          ("hash", "u1", (32,)), ("chain_key", "u1", (32,)), ("ephemeral", "u1", (32,))])  # wgcs_hs_init
HS_RESP_DTYPE = np.dtype([("init_row", "<u4"), ("peer_row", "<u4"), ("local_index", "<u4"), ("send_key", "<u4"),
                          ("recv_key", "<u4"), ("flags", "<u4"), ("pad", "<u4", (2,)), ("ephemeral_private", "u1", (32,)),
                          ("cookie", "u1", (16,))])  # wgcs_hs_resp
HS_STATE_DTYPE = np.dtype([("state", "<u4"), ("local_index", "<u4"), ("peer_row", "<u4"), ("remote_index", "<u4"),
                           ("send_key", "<u4"), ("recv_key", "<u4"), ("claim", "<u4"), ("pad", "<u4"),
                           ("hash", "u1", (32,)), ("chain_key", "u1", (32,)),
                           ("ephemeral_private", "u1", (32,))])  # wgcs_hs_state
HS_START_DTYPE = np.dtype([("state_row", "<u4"), ("peer_row", "<u4"), ("local_index", "<u4"), ("send_key", "<u4"),
                           ("recv_key", "<u4"), ("flags", "<u4"), ("timestamp", "u1", (12,)), ("pad0", "u1", (4,)),
                           ("ephemeral_private", "u1", (32,)), ("cookie", "u1", (16,)),
                           ("pad1", "u1", (8,))])  # wgcs_hs_start
HS_PEER_DTYPE = np.dtype([("last_timestamp", "u1", (12,)), ("state", "<u4"), ("last_consumption_ns", "<i8"),
                          ("flags", "<u4"), ("remote_index", "<u4"), ("claim", "<u4"), ("cookie", "u1", (16,)),
                          ("pad", "u1", (12,))])  # wgcs_hs_peer
HS_TICKET_DTYPE = np.dtype([("local_index", "<u4"), ("send_key", "<u4"), ("recv_key", "<u4"), ("pad", "<u4"),
                            ("ephemeral_private", "u1", (32,))])  # wgcs_hs_ticket
HS_CLAIM_NONE = 0xFFFFFFFF  # wgcs_hs_peer.claim outside a call
RESPONSE_SIZE, RESPONSE_PITCH = 92, 96  # MessageResponseSize; a row of respond_batch's msgs
INITIATION_SIZE, INITIATION_PITCH = 148, 160  # MessageInitiationSize; a row of initiate_batch's msgs
FINISH_WORK_BYTES = 64  # finish_batch's scratch per row
assert NOISE_RESPONDER_DTYPE.itemsize == 96 and PEER_KEY_DTYPE.itemsize == 72 and HS_INIT_DTYPE.itemsize == 128
assert HS_RESP_DTYPE.itemsize == 80 and HS_STATE_DTYPE.itemsize == 128 and HS_START_DTYPE.itemsize == 96
assert HS_PEER_DTYPE.itemsize == 64 and HS_TICKET_DTYPE.itemsize == 48

__all__ = ["NOISE_RESPONDER_DTYPE", "PEER_KEY_DTYPE", "HS_INIT_DTYPE", "x25519", "responder_init", "peer_keys_build",
           "peer_keys_find", "consume_initiation", "create_initiation", "x25519_batch", "consume_batch", "HS_NONE",
           "HS_PASS", "HS_CONSUMED", "ERR_AUTH", "ERR_LOW_ORDER", "ERR_NO_PEER", "PEER_NONE", "PEER_RUNNING",
           "HS_RESP_DTYPE", "RESPONSE_SIZE", "RESPONSE_PITCH", "create_response", "consume_response", "respond_batch",
           "HS_RESPONDED", "HS_RESP_COOKIE", "HS_STATE_DTYPE", "HS_START_DTYPE", "INITIATION_SIZE", "INITIATION_PITCH",
           "FINISH_WORK_BYTES", "initiate_batch", "finish_batch", "initiate_host", "finish_host", "HS_INITIATED",
           "HS_FINISHED", "HS_START_COOKIE", "HS_STATE_ZEROED", "HS_STATE_INITIATED", "ERR_NO_HANDSHAKE",
           "HS_PEER_DTYPE", "HS_TICKET_DTYPE", "HS_CLAIM_NONE", "peer_rows_build", "accept_batch", "accept_host",
           "HS_ACCEPTED", "ERR_FLOOD", "ERR_REPLAY", "ERR_BATCH_FULL", "HS_PEER_ZEROED", "HS_PEER_CONSUMED",
           "HS_PEER_SEEN", "HS_PEER_COOKIE"]


def _one(x, dtype: np.dtype, what: str) -> np.ndarray:
    a = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    if len(a) != 1:
        raise ValueError(f"one {what} row")
    return a


def x25519(scalar, point) -> bytes | None:
    """X25519(scalar, point), or None for the all-zero result of a low-order point."""
    out = C.create_string_buffer(32)
    rc = _lib.load().wgcs_x25519(out, _fixed(scalar, 32, "a scalar"), _fixed(point, 32, "a point"))
    if rc == ERR_LOW_ORDER:
        return None
    _status(rc, "wgcs_x25519")
    return out.raw


def responder_init(private_key) -> tuple[np.ndarray, bytes]:
    """(one NOISE_RESPONDER_DTYPE row for the static private key, its public key)."""
    r = np.zeros(1, NOISE_RESPONDER_DTYPE)
    pub = C.create_string_buffer(32)
    _status(_lib.load().wgcs_noise_responder_init(r.ctypes.data, _fixed(private_key, 32, "a private key"), pub),
            "wgcs_noise_responder_init")
    return r, pub.raw


def peer_keys_build(responder, public_keys, peers, flags=None) -> np.ndarray:
    """PEER_KEY_DTYPE rows sorted by public key for the peers' 32-byte static
    public keys, their ids and (optional; default: all running) flags."""
    r = _one(responder, NOISE_RESPONDER_DTYPE, "NOISE_RESPONDER_DTYPE")
    keys = b"".join(_fixed(k, 32, "a public key") for k in public_keys)
    n = len(keys) // 32
    ids = np.ascontiguousarray(peers, dtype=np.uint32).reshape(-1)
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32).reshape(-1)
    if len(ids) != n or (fl is not None and len(fl) != n):
        raise ValueError("one peer id (and one flags word) per public key")
    table = np.zeros(n, PEER_KEY_DTYPE)
    _status(_lib.load().wgcs_peer_keys_build(r.ctypes.data, keys, ids.ctypes.data if n else None,
                                             None if fl is None or n == 0 else fl.ctypes.data, n,
                                             table.ctypes.data if n else None), "wgcs_peer_keys_build")
    return table


def peer_keys_find(table, public_key) -> int:
    """The row of public_key in a PEER_KEY_DTYPE table, or -1."""
    t = np.ascontiguousarray(table, dtype=PEER_KEY_DTYPE).reshape(-1)
    return _lib.load().wgcs_peer_keys_find(t.ctypes.data if len(t) else None, len(t),
                                           _fixed(public_key, 32, "a public key"))


def consume_initiation(responder, table, msg) -> tuple[int, np.ndarray]:
    """(verdict, one HS_INIT_DTYPE row) for one message on the host: HS_CONSUMED
    with the whole row, or ERR_LOW_ORDER / ERR_AUTH / ERR_NO_PEER with a row
    that holds the sender and the peer found so far, or ERR_INVALID_ARG (a
    length other than 148 or a wrong type word) with the row untouched (zero)."""
    r = _one(responder, NOISE_RESPONDER_DTYPE, "NOISE_RESPONDER_DTYPE")
    t = np.ascontiguousarray(table, dtype=PEER_KEY_DTYPE).reshape(-1)
    m = bytes(msg)
    out = np.zeros(1, HS_INIT_DTYPE)
    verdict = _lib.load().wgcs_noise_consume_initiation(r.ctypes.data, t.ctypes.data if len(t) else None, len(t), m,
                                                        len(m), out.ctypes.data)
    return verdict, out


def create_initiation(static_private, remote_static, ephemeral_private, timestamp, sender: int
                      ) -> tuple[bytes, bytes, bytes]:
    """(the 148-byte initiation with zero MACs -- cookie.add_macs fills them --,
    the handshake's hash, its chaining key)."""
    msg, h, ck = C.create_string_buffer(148), C.create_string_buffer(32), C.create_string_buffer(32)
    _status(_lib.load().wgcs_noise_create_initiation(_fixed(static_private, 32, "a private key"),
                                                     _fixed(remote_static, 32, "a public key"),
                                                     _fixed(ephemeral_private, 32, "an ephemeral private key"),
                                                     _fixed(timestamp, 12, "a timestamp"), sender & 0xFFFFFFFF, msg, h,
                                                     ck), "wgcs_noise_create_initiation")
    return msg.raw, h.raw, ck.raw


def create_response(init, remote_static, ephemeral_private, local_index: int, preshared_key=None, cookie=None
                    ) -> tuple[int, bytes, bytes, bytes]:
    """(status, the 92-byte response with its MACs, send key, recv key) for one
    HS_INIT_DTYPE row that consume_initiation returned with HS_CONSUMED: status
    0, or ERR_LOW_ORDER with all three zeroed.  preshared_key None is the
    all-zero key; cookie (16 bytes) None leaves MAC2 zero."""
    row = _one(init, HS_INIT_DTYPE, "HS_INIT_DTYPE")
    msg, send, recv = C.create_string_buffer(92), C.create_string_buffer(32), C.create_string_buffer(32)
    rc = _lib.load().wgcs_noise_create_response(
        row.ctypes.data, _fixed(remote_static, 32, "a public key"),
        None if preshared_key is None else _fixed(preshared_key, 32, "a preshared key"),
        _fixed(ephemeral_private, 32, "an ephemeral private key"), local_index & 0xFFFFFFFF,
        None if cookie is None else _fixed(cookie, 16, "a cookie"), msg, send, recv)
    if rc != ERR_LOW_ORDER:
        _status(rc, "wgcs_noise_create_response")
    return rc, msg.raw, send.raw, recv.raw


def consume_response(static_private, hash_, chain_key, ephemeral_private, local_index: int, msg, preshared_key=None
                     ) -> tuple[int, int | None, bytes, bytes]:
    """(status, sender index, send key, recv key) on the initiator's side, under
    what create_initiation returned and the index it was sent with: status 0, or
    ERR_INVALID_ARG (a length other than 92, a wrong type word, another
    receiver), ERR_LOW_ORDER or ERR_AUTH with no sender and zero keys."""
    m = bytes(msg)
    sender, send, recv = C.c_uint32(0), C.create_string_buffer(32), C.create_string_buffer(32)
    rc = _lib.load().wgcs_noise_consume_response(
        _fixed(static_private, 32, "a private key"), _fixed(hash_, 32, "a hash"), _fixed(chain_key, 32, "a chaining key"),
        _fixed(ephemeral_private, 32, "an ephemeral private key"),
        None if preshared_key is None else _fixed(preshared_key, 32, "a preshared key"), local_index & 0xFFFFFFFF, m,
        len(m), C.byref(sender), send, recv)
    return rc, sender.value if rc == 0 else None, send.raw, recv.raw


def x25519_batch(dev, scalars, points, out, status, stream=None, n: int | None = None) -> None:
    """Asynchronous wgcs_x25519_batch over 32-byte rows on the device: out row q
    = X25519(scalars row q, points row q), status[q] (int32) = 0 or ERR_LOW_ORDER."""
    s = getattr(stream, "cuda_stream", stream)
    if n is None:
        n = scalars.numel() * scalars.element_size() // 32
    dev._check(dev.lib.wgcs_x25519_batch(dev.h, _ptr(scalars), _ptr(points), n, _ptr(out), _ptr(status), s))


def consume_batch(dev, arena, pkts, types, gate, responder, table, verdict, out, stream=None, n: int | None = None,
                  n_peers: int | None = None) -> None:
    """Asynchronous wgcs_handshake_consume_batch over classify_batch's pkts and
    types and screen_batch's verdicts as `gate` (None: every row of type 1):
    verdict[q] (int32) = HS_NONE, HS_CONSUMED, ERR_INVALID_ARG, ERR_LOW_ORDER,
    ERR_AUTH or ERR_NO_PEER, and out (HS_INIT_DTYPE rows) as the header says.
    responder is one NOISE_RESPONDER_DTYPE row and table PEER_KEY_DTYPE rows on
    the device."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_peers = (0 if table is None else _rows(table, PEER_KEY_DTYPE)) if n_peers is None else n_peers
    dev._check(dev.lib.wgcs_handshake_consume_batch(dev.h, _ptr(arena), _ptr(pkts), _ptr(types), _ptr(gate), n,
                                                    _ptr(responder), _ptr(table) if n_peers else None, n_peers,
                                                    _ptr(verdict), _ptr(out), s))


def respond_batch(dev, resp, init, gate, table, psk, keys, msgs, status, stream=None, n: int | None = None,
                  n_init: int | None = None, n_peers: int | None = None, n_keys: int | None = None) -> None:
    """Asynchronous wgcs_handshake_respond_batch over HS_RESP_DTYPE descriptors:
    `init` and `gate` are consume_batch's out and verdict (gate None: every
    descriptor is taken), `table` its PEER_KEY_DTYPE rows, `psk` 32 bytes per
    table row or None, `keys` the AEAD_KEY_DTYPE table that seal_batch and
    open_batch read.  status[j] (int32) = HS_RESPONDED, HS_NONE,
    ERR_INVALID_ARG, ERR_NO_PEER or ERR_LOW_ORDER, and msgs (RESPONSE_PITCH
    bytes per descriptor) and keys as the header says.  Everything is on the
    device."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(resp, HS_RESP_DTYPE) if n is None else n
    n_init = (0 if init is None else _rows(init, HS_INIT_DTYPE)) if n_init is None else n_init
    n_peers = (0 if table is None else _rows(table, PEER_KEY_DTYPE)) if n_peers is None else n_peers
    n_keys = (0 if keys is None else _rows(keys, AEAD_KEY_DTYPE)) if n_keys is None else n_keys
    dev._check(dev.lib.wgcs_handshake_respond_batch(dev.h, _ptr(resp), n, _ptr(init) if n_init else None, _ptr(gate),
                                                    n_init, _ptr(table) if n_peers else None, _ptr(psk), n_peers,
                                                    _ptr(keys) if n_keys else None, n_keys, _ptr(msgs), _ptr(status), s))


def initiate_batch(dev, start, static_public, table, states, msgs, status, n_keys: int, stream=None, n: int | None = None,
                   n_peers: int | None = None, n_states: int | None = None) -> None:
    """Asynchronous wgcs_handshake_initiate_batch over HS_START_DTYPE
    descriptors: `static_public` is the device's own public key (32 bytes),
    `table` its PEER_KEY_DTYPE rows (remote static and precomputed secret),
    `states` the HS_STATE_DTYPE table that finish_batch reads, n_keys the rows of
    the AEAD key table the descriptors' key rows are checked against.
    status[j] (int32) = HS_INITIATED, ERR_INVALID_ARG or ERR_LOW_ORDER, and msgs
    (INITIATION_PITCH bytes per descriptor) and states as the header says.
    Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(start, HS_START_DTYPE) if n is None else n
    n_peers = (0 if table is None else _rows(table, PEER_KEY_DTYPE)) if n_peers is None else n_peers
    n_states = (0 if states is None else _rows(states, HS_STATE_DTYPE)) if n_states is None else n_states
    dev._check(dev.lib.wgcs_handshake_initiate_batch(dev.h, _ptr(start), n, _ptr(static_public),
                                                     _ptr(table) if n_peers else None, n_peers, n_keys,
                                                     _ptr(states) if n_states else None, n_states, _ptr(msgs),
                                                     _ptr(status), s))


def finish_batch(dev, arena, pkts, types, gate, responder, slots, states, psk, keys, work, verdict, stream=None,
                 n: int | None = None, n_slots: int | None = None, n_states: int | None = None,
                 n_peers: int | None = None, n_keys: int | None = None) -> None:
    """Asynchronous wgcs_handshake_finish_batch over classify_batch's pkts and
    types and screen_batch's verdicts as `gate` (None: every row of type 2).
    `responder` is the device's own NOISE_RESPONDER_DTYPE row, `slots`
    router.session_table rows that list local_index -> row of `states`, `psk` 32
    bytes per peer row or None (then give n_peers), `keys` the AEAD_KEY_DTYPE
    table, `work` FINISH_WORK_BYTES of scratch per row.  verdict[q] (int32) =
    HS_NONE, HS_FINISHED, ERR_INVALID_ARG, ERR_NO_HANDSHAKE, ERR_LOW_ORDER or
    ERR_AUTH, and keys and states as the header says.  Everything is on the
    device."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_slots = (0 if slots is None else _rows(slots, SESSION_SLOT_DTYPE)) if n_slots is None else n_slots
    n_states = (0 if states is None else _rows(states, HS_STATE_DTYPE)) if n_states is None else n_states
    if n_peers is None:
        if psk is None:
            raise ValueError("n_peers, where there is no psk table to count")
        n_peers = _rows(psk, np.dtype(("u1", (32,))))
    n_keys = (0 if keys is None else _rows(keys, AEAD_KEY_DTYPE)) if n_keys is None else n_keys
    dev._check(dev.lib.wgcs_handshake_finish_batch(dev.h, _ptr(arena), _ptr(pkts), _ptr(types), _ptr(gate), n,
                                                   _ptr(responder), _ptr(slots) if n_slots else None, n_slots,
                                                   _ptr(states) if n_states else None, n_states, _ptr(psk), n_peers,
                                                   _ptr(keys) if n_keys else None, n_keys, _ptr(work), _ptr(verdict), s))


def _host(a, dtype, what: str) -> np.ndarray:
    """A writable C-contiguous array of `dtype` rows over the caller's memory (no copy: the C side writes it)."""
    if not isinstance(a, np.ndarray) or not a.flags.c_contiguous or not a.flags.writeable:
        raise TypeError(f"{what}: a writable C-contiguous numpy array")
    return a.reshape(-1).view(np.uint8).view(dtype)


def initiate_host(start, static_public, table, states, msgs, status, n_keys: int) -> None:
    """wgcs_handshake_initiate_host: initiate_batch on numpy arrays, row by row.
    `states` (HS_STATE_DTYPE), `msgs` (uint8, INITIATION_PITCH bytes per
    descriptor) and `status` (int32) are written in place."""
    d = np.ascontiguousarray(start, dtype=HS_START_DTYPE).reshape(-1)
    t = np.ascontiguousarray(table, dtype=PEER_KEY_DTYPE).reshape(-1)
    st, m, out = _host(states, HS_STATE_DTYPE, "states"), _host(msgs, np.uint8, "msgs"), _host(status, np.int32, "status")
    if len(m) < INITIATION_PITCH * len(d) or len(out) < len(d):
        raise ValueError("msgs and status hold one row per descriptor")
    _status(_lib.load().wgcs_handshake_initiate_host(d.ctypes.data, len(d), _fixed(static_public, 32, "a public key"),
                                                     t.ctypes.data if len(t) else None, len(t), n_keys,
                                                     st.ctypes.data if len(st) else None, len(st), m.ctypes.data,
                                                     out.ctypes.data), "wgcs_handshake_initiate_host")


def finish_host(arena, pkts, types, gate, responder, slots, states, psk, keys, work, verdict, n_peers: int | None = None
                ) -> None:
    """wgcs_handshake_finish_host: finish_batch on numpy arrays, in its two
    passes.  `states` (HS_STATE_DTYPE), `keys` (AEAD_KEY_DTYPE), `work` (uint8)
    and `verdict` (int32) are written in place; gate and psk may be None (then
    give n_peers)."""
    a = np.ascontiguousarray(arena, dtype=np.uint8).reshape(-1)
    p = np.ascontiguousarray(pkts, dtype=AEAD_PKT_DTYPE).reshape(-1)
    ty = np.ascontiguousarray(types, dtype=np.int32).reshape(-1)
    g = None if gate is None else np.ascontiguousarray(gate, dtype=np.int32).reshape(-1)
    r = _one(responder, NOISE_RESPONDER_DTYPE, "NOISE_RESPONDER_DTYPE")
    sl = np.ascontiguousarray(slots, dtype=SESSION_SLOT_DTYPE).reshape(-1)
    k = None if psk is None else np.ascontiguousarray(psk, dtype=np.uint8).reshape(-1, 32)
    st, ks = _host(states, HS_STATE_DTYPE, "states"), _host(keys, AEAD_KEY_DTYPE, "keys")
    w, out = _host(work, np.uint8, "work"), _host(verdict, np.int32, "verdict")
    n = len(p)
    if len(ty) != n or (g is not None and len(g) != n) or len(w) < FINISH_WORK_BYTES * n or len(out) < n:
        raise ValueError("types, gate, work and verdict hold one row per packet")
    if n_peers is None:
        if k is None:
            raise ValueError("n_peers, where there is no psk table to count")
        n_peers = len(k)
    _status(_lib.load().wgcs_handshake_finish_host(a.ctypes.data, p.ctypes.data, ty.ctypes.data,
                                                   None if g is None else g.ctypes.data, n, r.ctypes.data,
                                                   sl.ctypes.data if len(sl) else None, len(sl),
                                                   st.ctypes.data if len(st) else None, len(st),
                                                   None if k is None else k.ctypes.data, n_peers,
                                                   ks.ctypes.data if len(ks) else None, len(ks), w.ctypes.data,
                                                   out.ctypes.data), "wgcs_handshake_finish_host")


def peer_rows_build(table, n_ids: int) -> np.ndarray:
    """wgcs_peer_rows_build: rows[id] (uint32) = the row of the PEER_KEY_DTYPE
    table whose peer is id, PEER_NONE for an id no row has.  An id >= n_ids in
    the table raises."""
    t = np.ascontiguousarray(table, dtype=PEER_KEY_DTYPE).reshape(-1)
    rows = np.zeros(n_ids, np.uint32)
    _status(_lib.load().wgcs_peer_rows_build(t.ctypes.data if len(t) else None, len(t),
                                             rows.ctypes.data if n_ids else None, n_ids), "wgcs_peer_rows_build")
    return rows


def accept_batch(dev, init, gate, now_ns: int, table, peer_rows, peers, tickets, resp, count, verdict, stream=None,
                 n: int | None = None, n_ids: int | None = None, n_peers: int | None = None,
                 n_tickets: int | None = None) -> None:
    """Asynchronous wgcs_handshake_accept_batch between consume_batch and
    respond_batch: `init` and `gate` are consume_batch's out and verdict, `table`
    its PEER_KEY_DTYPE rows, `peer_rows` peer_rows_build's uint32 rows of it,
    `peers` one HS_PEER_DTYPE row per table row, `tickets` HS_TICKET_DTYPE rows.
    verdict[q] (int32) = gate[q] where that is not HS_CONSUMED, else HS_ACCEPTED,
    ERR_NO_PEER, ERR_REPLAY, ERR_FLOOD or ERR_BATCH_FULL; resp (one
    HS_RESP_DTYPE row per ticket), count (one uint32) and peers as the header
    says.  Everything is on the device; now_ns is an int64 of the caller's
    monotonic clock."""
    s = getattr(stream, "cuda_stream", stream)
    n = (0 if init is None else _rows(init, HS_INIT_DTYPE)) if n is None else n
    n_ids = (0 if peer_rows is None else _rows(peer_rows, np.dtype("<u4"))) if n_ids is None else n_ids
    n_peers = (0 if table is None else _rows(table, PEER_KEY_DTYPE)) if n_peers is None else n_peers
    n_tickets = (0 if tickets is None else _rows(tickets, HS_TICKET_DTYPE)) if n_tickets is None else n_tickets
    dev._check(dev.lib.wgcs_handshake_accept_batch(dev.h, _ptr(init), _ptr(gate), n, now_ns, _ptr(table), _ptr(peer_rows),
                                                   n_ids, _ptr(peers), n_peers, _ptr(tickets), n_tickets, _ptr(resp),
                                                   _ptr(count), _ptr(verdict), s))


def accept_host(init, gate, now_ns: int, table, peer_rows, peers, tickets, resp, count, verdict) -> None:
    """wgcs_handshake_accept_host: accept_batch on numpy arrays, in its passes.
    `peers` (HS_PEER_DTYPE), `resp` (HS_RESP_DTYPE, one row per ticket), `count`
    (one uint32) and `verdict` (int32) are written in place."""
    i = np.ascontiguousarray(init, dtype=HS_INIT_DTYPE).reshape(-1)
    g = np.ascontiguousarray(gate, dtype=np.int32).reshape(-1)
    t = np.ascontiguousarray(table, dtype=PEER_KEY_DTYPE).reshape(-1)
    pr = np.ascontiguousarray(peer_rows, dtype=np.uint32).reshape(-1)
    tk = np.ascontiguousarray(tickets, dtype=HS_TICKET_DTYPE).reshape(-1)
    ps, r = _host(peers, HS_PEER_DTYPE, "peers"), _host(resp, HS_RESP_DTYPE, "resp")
    c, out = _host(count, np.uint32, "count"), _host(verdict, np.int32, "verdict")
    n = len(i)
    if len(g) != n or len(out) < n or len(ps) != len(t) or len(r) < len(tk) or len(c) < 1:
        raise ValueError("gate and verdict hold one row per initiation, peers one per table row, resp one per ticket")
    _status(_lib.load().wgcs_handshake_accept_host(i.ctypes.data if n else None, g.ctypes.data if n else None, n, now_ns,
                                                   t.ctypes.data if len(t) else None, pr.ctypes.data if len(pr) else None,
                                                   len(pr), ps.ctypes.data if len(ps) else None, len(t),
                                                   tk.ctypes.data if len(tk) else None, len(tk),
                                                   r.ctypes.data if len(tk) else None, c.ctypes.data,
                                                   out.ctypes.data if n else None), "wgcs_handshake_accept_host")
