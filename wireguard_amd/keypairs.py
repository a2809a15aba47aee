"""Host-side mirror of keypair rotation (package `device`, noise.go:664-754 and
sessions.go) over the C ABI.

Names and argument meaning follow the reference:
  begin_responder_batch / begin_initiator_batch   the tail of BeginSymmetricSession -- sessions.AddKeypair, the
                                                  rotation of previous / current / next with DeleteSession, the
                                                  initiator's new send key -- behind respond_batch / finish_batch,
                                                  noise.go:664-722
  received_batch                                  ReceivedWithNewKeypair per packet behind replay_batch,
                                                  noise.go:725-754, receive.go:418-429
  begin_responder_host / begin_initiator_host /
  received_host                                   those three on host memory (numpy arrays), in row order
One KEYPAIRS_DTYPE row per row of the peer table holds the three entries.  The
two slot tables are router.session_table rows: `slots` (receiver index -> key
row, what classify_batch reads) and `peer_keys` (peer id -> send-key row, what
send_assign_batch reads).  Register every index and every peer id ahead of
time with the key SESSION_NO_KEYPAIR: the calls only overwrite the key of a
slot that exists.  The row functions and the kernels live in libwgcsum.so
(wgcs_keypairs.h, keypairs_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (ERR_INVALID_ARG, ERR_NO_HANDSHAKE, HS_BEGUN, HS_FINISHED, HS_NONE, HS_RESPONDED, KEYPAIR_INITIATOR,
                   KEYPAIR_SET, PEER_NONE, SESSION_NO_KEYPAIR)
from .cookie import _status
from .noise import HS_RESP_DTYPE, HS_STATE_DTYPE, PEER_KEY_DTYPE, _host
from .router import SESSION_SLOT_DTYPE
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE, _rows
from .tun import _ptr

KEYPAIR_REF_DTYPE = np.dtype([("send_key", "<u4"), ("recv_key", "<u4"), ("local_index", "<u4"), ("flags", "<u4"),
                              ("created_ns", "<i8")])  # wgcs_keypair_ref
KEYPAIRS_DTYPE = np.dtype([("previous", KEYPAIR_REF_DTYPE), ("current", KEYPAIR_REF_DTYPE), ("next", KEYPAIR_REF_DTYPE),
                           ("claim", "<u4"), ("pad", "<u4")])  # wgcs_keypairs
KEYPAIRS_CLAIM_NONE = 0xFFFFFFFF  # wgcs_keypairs.claim outside a received call
assert KEYPAIR_REF_DTYPE.itemsize == 24 and KEYPAIRS_DTYPE.itemsize == 80

__all__ = ["KEYPAIR_REF_DTYPE", "KEYPAIRS_DTYPE", "KEYPAIRS_CLAIM_NONE", "SESSION_NO_KEYPAIR", "KEYPAIR_SET",
           "KEYPAIR_INITIATOR", "HS_BEGUN", "HS_NONE", "HS_RESPONDED", "HS_FINISHED", "ERR_INVALID_ARG",
           "ERR_NO_HANDSHAKE", "PEER_NONE", "keypairs_table", "begin_responder_batch", "begin_initiator_batch",
           "received_batch", "begin_responder_host", "begin_initiator_host", "received_host"]

_U4 = np.dtype("<u4")


def keypairs_table(n_peers: int) -> np.ndarray:
    """n_peers KEYPAIRS_DTYPE rows with every entry nil and no claim."""
    kp = np.zeros(n_peers, KEYPAIRS_DTYPE)
    kp["claim"] = KEYPAIRS_CLAIM_NONE
    return kp


def _count(x, dtype, given):
    return (0 if x is None else _rows(x, dtype)) if given is None else given


def begin_responder_batch(dev, resp, gate, now_ns: int, table, kp, slots, peer_keys, keys, key_peer, status, work,
                          stream=None, n: int | None = None, n_peers: int | None = None, n_slots: int | None = None,
                          n_peer_slots: int | None = None, n_keys: int | None = None, work_bytes: int | None = None
                          ) -> None:
    """Asynchronous wgcs_keypairs_begin_responder_batch behind respond_batch:
    `resp` are its HS_RESP_DTYPE descriptors and `gate` its status; `table` the
    PEER_KEY_DTYPE rows, `kp` one KEYPAIRS_DTYPE row per table row, `slots` and
    `peer_keys` the two session_table arrays, `keys` the AEAD_KEY_DTYPE table
    and `key_peer` (uint32) its key -> peer id column, `work`
    keystate.work_bytes(n) of 16-byte-aligned scratch.  status[j] (int32) =
    HS_NONE, HS_BEGUN, ERR_INVALID_ARG or ERR_NO_HANDSHAKE, and the tables as
    the header says.  Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    n = _count(resp, HS_RESP_DTYPE, n)
    dev._check(dev.lib.wgcs_keypairs_begin_responder_batch(
        dev.h, _ptr(resp), _ptr(gate), n, now_ns, _ptr(table), _count(table, PEER_KEY_DTYPE, n_peers), _ptr(kp),
        _ptr(slots), _count(slots, SESSION_SLOT_DTYPE, n_slots), _ptr(peer_keys),
        _count(peer_keys, SESSION_SLOT_DTYPE, n_peer_slots), _ptr(keys), _ptr(key_peer),
        _count(keys, AEAD_KEY_DTYPE, n_keys), _ptr(status), _ptr(work), _count(work, np.dtype("u1"), work_bytes), s))


def begin_initiator_batch(dev, arena, pkts, gate, now_ns: int, hs_slots, states, table, kp, slots, peer_keys, keys,
                          key_peer, status, work, stream=None, n: int | None = None, n_hs_slots: int | None = None,
                          n_states: int | None = None, n_peers: int | None = None, n_slots: int | None = None,
                          n_peer_slots: int | None = None, n_keys: int | None = None, work_bytes: int | None = None
                          ) -> None:
    """Asynchronous wgcs_keypairs_begin_initiator_batch behind finish_batch:
    `arena` and `pkts` are the receive batch, `gate` finish_batch's verdict,
    `hs_slots` and `states` its slots and its HS_STATE_DTYPE table (only read);
    the rest as begin_responder_batch."""
    s = getattr(stream, "cuda_stream", stream)
    n = _count(pkts, AEAD_PKT_DTYPE, n)
    dev._check(dev.lib.wgcs_keypairs_begin_initiator_batch(
        dev.h, _ptr(arena), _ptr(pkts), _ptr(gate), n, now_ns, _ptr(hs_slots),
        _count(hs_slots, SESSION_SLOT_DTYPE, n_hs_slots), _ptr(states), _count(states, HS_STATE_DTYPE, n_states),
        _ptr(table), _count(table, PEER_KEY_DTYPE, n_peers), _ptr(kp), _ptr(slots),
        _count(slots, SESSION_SLOT_DTYPE, n_slots), _ptr(peer_keys), _count(peer_keys, SESSION_SLOT_DTYPE, n_peer_slots),
        _ptr(keys), _ptr(key_peer), _count(keys, AEAD_KEY_DTYPE, n_keys), _ptr(status), _ptr(work),
        _count(work, np.dtype("u1"), work_bytes), s))


def received_batch(dev, pkts, verdict, key_peer, peer_rows, kp, slots, peer_keys, keys, rotated, stream=None,
                   n: int | None = None, n_keys: int | None = None, n_ids: int | None = None,
                   n_peers: int | None = None, n_slots: int | None = None, n_peer_slots: int | None = None) -> None:
    """Asynchronous wgcs_keypairs_received_batch behind replay_batch: `pkts`
    are the receive batch's AEAD_PKT_DTYPE rows and `verdict` replay_batch's;
    `key_peer` (uint32 per key row), `peer_rows` (noise.peer_rows_build), `kp`,
    `slots`, `peer_keys` and `keys` as above.  rotated[i] (uint32) = 1 for the
    row that promoted its peer's next keypair, else 0.  Everything is on the
    device."""
    s = getattr(stream, "cuda_stream", stream)
    n = _count(pkts, AEAD_PKT_DTYPE, n)
    dev._check(dev.lib.wgcs_keypairs_received_batch(
        dev.h, _ptr(pkts), _ptr(verdict), n, _ptr(key_peer), _count(key_peer, _U4, n_keys), _ptr(peer_rows),
        _count(peer_rows, _U4, n_ids), _ptr(kp), _count(kp, KEYPAIRS_DTYPE, n_peers), _ptr(slots),
        _count(slots, SESSION_SLOT_DTYPE, n_slots), _ptr(peer_keys), _count(peer_keys, SESSION_SLOT_DTYPE, n_peer_slots),
        _ptr(keys), _ptr(rotated), s))


def _in(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a: np.ndarray):
    return a.ctypes.data if len(a) else None


def _tail(table, kp, slots, peer_keys, keys, key_peer):
    t = _in(table, PEER_KEY_DTYPE)
    k, sl, pk = _host(kp, KEYPAIRS_DTYPE, "kp"), _host(slots, SESSION_SLOT_DTYPE, "slots"), _host(
        peer_keys, SESSION_SLOT_DTYPE, "peer_keys")
    ks, kpr = _host(keys, AEAD_KEY_DTYPE, "keys"), _host(key_peer, np.uint32, "key_peer")
    if len(k) != len(t) or len(kpr) != len(ks):
        raise ValueError("kp holds one row per table row, key_peer one word per key row")
    return t, k, sl, pk, ks, kpr


def begin_responder_host(resp, gate, now_ns: int, table, kp, slots, peer_keys, keys, key_peer, status) -> None:
    """wgcs_keypairs_begin_responder_host: begin_responder_batch on numpy
    arrays, in descriptor order.  `kp`, `slots`, `peer_keys`, `keys`, `key_peer`
    and `status` are written in place."""
    r, g = _in(resp, HS_RESP_DTYPE), _in(gate, np.int32)
    t, k, sl, pk, ks, kpr = _tail(table, kp, slots, peer_keys, keys, key_peer)
    out = _host(status, np.int32, "status")
    if len(g) != len(r) or len(out) < len(r):
        raise ValueError("gate and status hold one row per descriptor")
    _status(_lib.load().wgcs_keypairs_begin_responder_host(_p(r), _p(g), len(r), now_ns, _p(t), len(t), _p(k), _p(sl),
                                                           len(sl), _p(pk), len(pk), _p(ks), _p(kpr), len(ks), _p(out)),
            "wgcs_keypairs_begin_responder_host")


def begin_initiator_host(arena, pkts, gate, now_ns: int, hs_slots, states, table, kp, slots, peer_keys, keys, key_peer,
                         status) -> None:
    """wgcs_keypairs_begin_initiator_host: begin_initiator_batch on numpy
    arrays, in row order."""
    a, p, g = _in(arena, np.uint8), _in(pkts, AEAD_PKT_DTYPE), _in(gate, np.int32)
    hs, st = _in(hs_slots, SESSION_SLOT_DTYPE), _in(states, HS_STATE_DTYPE)
    t, k, sl, pk, ks, kpr = _tail(table, kp, slots, peer_keys, keys, key_peer)
    out = _host(status, np.int32, "status")
    if len(g) != len(p) or len(out) < len(p):
        raise ValueError("gate and status hold one row per packet")
    _status(_lib.load().wgcs_keypairs_begin_initiator_host(_p(a), _p(p), _p(g), len(p), now_ns, _p(hs), len(hs), _p(st),
                                                           len(st), _p(t), len(t), _p(k), _p(sl), len(sl), _p(pk),
                                                           len(pk), _p(ks), _p(kpr), len(ks), _p(out)),
            "wgcs_keypairs_begin_initiator_host")


def received_host(pkts, verdict, key_peer, peer_rows, kp, slots, peer_keys, keys, rotated) -> None:
    """wgcs_keypairs_received_host: received_batch on numpy arrays, in its two
    passes.  `key_peer`, `kp`, `slots`, `peer_keys`, `keys` and `rotated`
    (uint32) are written in place."""
    p, v, pr = _in(pkts, AEAD_PKT_DTYPE), _in(verdict, np.int32), _in(peer_rows, np.uint32)
    k, sl, pk = _host(kp, KEYPAIRS_DTYPE, "kp"), _host(slots, SESSION_SLOT_DTYPE, "slots"), _host(
        peer_keys, SESSION_SLOT_DTYPE, "peer_keys")
    ks, kpr = _host(keys, AEAD_KEY_DTYPE, "keys"), _host(key_peer, np.uint32, "key_peer")
    out = _host(rotated, np.uint32, "rotated")
    if len(v) != len(p) or len(out) < len(p) or len(kpr) != len(ks):
        raise ValueError("verdict and rotated hold one row per packet, key_peer one word per key row")
    _status(_lib.load().wgcs_keypairs_received_host(_p(p), _p(v), len(p), _p(kpr), len(ks), _p(pr), len(pr), _p(k),
                                                    len(k), _p(sl), len(sl), _p(pk), len(pk), _p(ks), _p(out)),
            "wgcs_keypairs_received_host")
