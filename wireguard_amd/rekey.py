"""Host-side mirror of keypair expiry, the rekey rules and the start of a
handshake (package `device`: receive.go:80-91 and :162-170, send.go:84-100,
:131-133, :213-227 and :368-374) over the C ABI.

Names and argument meaning follow the reference:
  recv_gate_batch    a packet under a keypair past RejectAfterTime gets the key SESSION_EXPIRED, between
                     classify_batch and open_batch                                   receive.go:162-170
  send_gate_batch    a job whose peer has no usable current keypair gets ERR_KEY_EXPIRED and stays staged,
                     between route_dst_batch and send_assign_batch                   send.go:368-374
  sent_batch         keepKeyFreshSending behind send_assign_batch                    send.go:213-227
  received_batch     keepKeyFreshReceiving behind write_build_batch                  receive.go:80-91
  responded_batch    SendHandshakeResponse's lastSentHandshake behind respond_batch  send.go:131-133
  start_batch        SendHandshakeInitiation: the wishes of the table into HS_START_DTYPE descriptors that
                     initiate_batch takes as they are                                send.go:84-100
  *_host             those six on host memory (numpy arrays), in row order
One REKEY_DTYPE row sits beside every KEYPAIRS_DTYPE row; a peer id finds its
row through noise.peer_rows_build.  The clock is the caller's: one int64 of
nanoseconds per call.  The row functions and the kernels live in libwgcsum.so
(wgcs_rekey.h, rekey_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ERR_BATCH_FULL, ERR_INVALID_ARG, ERR_KEY_EXPIRED, ERR_REKEY_TIMEOUT, HS_NONE, HS_STARTED,
                   KEEPALIVE_TIMEOUT_NS, PEER_NONE, REJECT_AFTER_TIME_NS, REKEY_AFTER_TIME_NS,
                   REKEY_LAST_MINUTE, REKEY_TIMEOUT_NS, REKEY_WANT_HOST, REKEY_WANT_LAST_MINUTE, REKEY_WANT_NO_KEYPAIR,
                   REKEY_WANT_REJECT_MESSAGES, REKEY_WANT_REJECT_TIME, REKEY_WANT_REKEY_MESSAGES,
                   REKEY_WANT_REKEY_TIME, SESSION_EXPIRED)
from .cookie import _status
from .keypairs import KEYPAIRS_DTYPE
from .noise import HS_PEER_DTYPE, HS_RESP_DTYPE, HS_START_DTYPE, _host
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import _ptr
from .writeplan import WRITE_GROUP_DTYPE

REKEY_DTYPE = np.dtype([("last_sent_ns", "<i8"), ("want", "<u4"), ("flags", "<u4")])  # wgcs_rekey
REKEY_AFTER_MESSAGES = 1 << 60  # WGCS_REKEY_AFTER_MESSAGES, constants.go:12
assert REKEY_DTYPE.itemsize == 16

__all__ = ["REKEY_DTYPE", "REJECT_AFTER_TIME_NS", "REKEY_AFTER_TIME_NS", "REKEY_TIMEOUT_NS", "KEEPALIVE_TIMEOUT_NS",
           "REKEY_AFTER_MESSAGES", "SESSION_EXPIRED", "ERR_KEY_EXPIRED", "ERR_REKEY_TIMEOUT", "ERR_BATCH_FULL",
           "ERR_INVALID_ARG", "HS_STARTED", "HS_NONE", "PEER_NONE", "REKEY_LAST_MINUTE", "REKEY_WANT_NO_KEYPAIR",
           "REKEY_WANT_REJECT_MESSAGES", "REKEY_WANT_REJECT_TIME", "REKEY_WANT_REKEY_MESSAGES", "REKEY_WANT_REKEY_TIME",
           "REKEY_WANT_LAST_MINUTE", "REKEY_WANT_HOST", "rekey_table", "recv_gate_batch", "send_gate_batch",
           "sent_batch", "received_batch", "responded_batch", "start_batch", "recv_gate_host", "send_gate_host",
           "sent_host", "received_host", "responded_host", "start_host"]

_U4, _I4, _U8, _U1 = np.dtype("<u4"), np.dtype("<i4"), np.dtype("<u8"), np.dtype("u1")


def rekey_table(n_peers: int, now_ns: int) -> np.ndarray:
    """n_peers REKEY_DTYPE rows as NewPeer leaves them (peer.go:180): nothing
    wanted, no flag, lastSentHandshake = now - (RekeyTimeout + 1 s)."""
    t = np.zeros(n_peers, REKEY_DTYPE)
    t["last_sent_ns"] = now_ns - (REKEY_TIMEOUT_NS + 1_000_000_000)
    return t


def _count(x, dtype, given):
    return (0 if x is None else _rows(x, dtype)) if given is None else given


def recv_gate_batch(dev, pkts, now_ns: int, key_peer, peer_rows, kp, stream=None, n: int | None = None,
                    n_keys: int | None = None, n_ids: int | None = None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_rekey_recv_gate_batch between classify_batch and
    open_batch: `pkts` are the receive batch's AEAD_PKT_DTYPE rows, of which
    only `key` is read and, for a keypair past RejectAfterTime, overwritten
    with SESSION_EXPIRED; `key_peer` (uint32 per key row), `peer_rows`
    (noise.peer_rows_build) and `kp` (KEYPAIRS_DTYPE) are only read.
    Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_rekey_recv_gate_batch(
        dev.h, _ptr(pkts), _count(pkts, AEAD_PKT_DTYPE, n), now_ns, _ptr(key_peer), _count(key_peer, _U4, n_keys),
        _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(kp), _count(kp, KEYPAIRS_DTYPE, n_peers), s))


def send_gate_batch(dev, peer, count, status_in, max_segs: int, now_ns: int, peer_rows, kp, send_nonce, limit: int,
                    rekey, status_out, stream=None, n_jobs: int | None = None, n_ids: int | None = None,
                    n_peers: int | None = None, n_keys: int | None = None) -> None:
    """Asynchronous wgcs_rekey_send_gate_batch between route_dst_batch and
    send_assign_batch: `peer` (uint32 per slot), `count` and `status_in`
    (int32 per job) are send_assign_batch's own inputs, `send_nonce` its
    uint64 per key row, `rekey` the REKEY_DTYPE table.  status_out[j] =
    ERR_KEY_EXPIRED for a job whose peer has no current keypair or one past
    its limits (want gets the reasons), else status_in[j]; it may be
    `status_in` and is what send_assign_batch then reads."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_rekey_send_gate_batch(
        dev.h, _ptr(peer), _ptr(count), _ptr(status_in), _count(count, _I4, n_jobs), max_segs, now_ns, _ptr(peer_rows),
        _count(peer_rows, _U4, n_ids), _ptr(kp), _count(kp, KEYPAIRS_DTYPE, n_peers), _ptr(send_nonce),
        _count(send_nonce, _U8, n_keys), limit, _ptr(rekey), _ptr(status_out), s))


def sent_batch(dev, peer, count, status, job_key, max_segs: int, now_ns: int, peer_rows, kp, send_nonce, limit: int,
               rekey, stream=None, n_jobs: int | None = None, n_ids: int | None = None, n_peers: int | None = None,
               n_keys: int | None = None) -> None:
    """Asynchronous wgcs_rekey_sent_batch behind send_assign_batch: `status`
    is send_gate_batch's status_out, `job_key` send_assign_batch's, and
    `send_nonce` as it left it.  Only `rekey`'s want is written."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_rekey_sent_batch(
        dev.h, _ptr(peer), _ptr(count), _ptr(status), _ptr(job_key), _count(count, _I4, n_jobs), max_segs, now_ns,
        _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(kp), _count(kp, KEYPAIRS_DTYPE, n_peers), _ptr(send_nonce),
        _count(send_nonce, _U8, n_keys), limit, _ptr(rekey), s))


def received_batch(dev, groups, calls_per_batch: int, now_ns: int, peer_rows, kp, rekey, stream=None,
                   n_batches: int | None = None, n_ids: int | None = None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_rekey_received_batch behind write_build_batch over
    its WRITE_GROUP_DTYPE rows (n_batches * calls_per_batch of them).  Only
    `rekey`'s want and flags are written."""
    s = getattr(stream, "cuda_stream", stream)
    if n_batches is None:
        n_batches = _count(groups, WRITE_GROUP_DTYPE, None) // max(calls_per_batch, 1)
    dev._check(dev.lib.wgcs_rekey_received_batch(
        dev.h, _ptr(groups), n_batches, calls_per_batch, now_ns, _ptr(peer_rows), _count(peer_rows, _U4, n_ids),
        _ptr(kp), _count(kp, KEYPAIRS_DTYPE, n_peers), _ptr(rekey), s))


def responded_batch(dev, resp, gate, now_ns: int, rekey, stream=None, n: int | None = None,
                    n_peers: int | None = None) -> None:
    """Asynchronous wgcs_rekey_responded_batch behind respond_batch: `resp`
    are its HS_RESP_DTYPE descriptors and `gate` its status.  last_sent_ns of
    every peer row it responded for becomes now_ns."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_rekey_responded_batch(dev.h, _ptr(resp), _ptr(gate), _count(resp, HS_RESP_DTYPE, n), now_ns,
                                                  _ptr(rekey), _count(rekey, REKEY_DTYPE, n_peers), s))


def start_batch(dev, now_ns: int, rekey, hs_peers, tickets, start, start_peer, count, status, reasons, work,
                stream=None, n_peers: int | None = None, n_tickets: int | None = None,
                work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_rekey_start_batch: `rekey` the REKEY_DTYPE table,
    `hs_peers` the HS_PEER_DTYPE rows (only flags and cookie are read),
    `tickets` prefilled HS_START_DTYPE rows.  Writes `start` (n_tickets
    HS_START_DTYPE rows, the tail with state_row 0xFFFFFFFF), `start_peer`
    (uint32 per ticket), `count` (one uint32), `status` (int32 per peer row:
    HS_NONE, HS_STARTED, ERR_REKEY_TIMEOUT or ERR_BATCH_FULL) and `reasons`
    (uint32 per peer row: want as it stood).  `work` is
    keystate.work_bytes(n_peers) of 16-byte-aligned scratch."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_rekey_start_batch(
        dev.h, now_ns, _ptr(rekey), _ptr(hs_peers), _count(rekey, REKEY_DTYPE, n_peers), _ptr(tickets),
        _count(tickets, HS_START_DTYPE, n_tickets), _ptr(start), _ptr(start_peer), _ptr(count), _ptr(status),
        _ptr(reasons), _ptr(work), _count(work, _U1, work_bytes), s))


def _in(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a: np.ndarray):
    return a.ctypes.data if len(a) else None


def _tables(peer_rows, kp, rekey=None):
    pr, k = _in(peer_rows, np.uint32), _in(kp, KEYPAIRS_DTYPE)
    if rekey is None:
        return pr, k
    r = _host(rekey, REKEY_DTYPE, "rekey")
    if len(r) != len(k):
        raise ValueError("rekey holds one row per kp row")
    return pr, k, r


def recv_gate_host(pkts, now_ns: int, key_peer, peer_rows, kp) -> None:
    """wgcs_rekey_recv_gate_host: recv_gate_batch on numpy arrays.  `pkts`
    (AEAD_PKT_DTYPE) is written in place."""
    p, kpr = _host(pkts, AEAD_PKT_DTYPE, "pkts"), _in(key_peer, np.uint32)
    pr, k = _tables(peer_rows, kp)
    _status(_lib.load().wgcs_rekey_recv_gate_host(_p(p), len(p), now_ns, _p(kpr), len(kpr), _p(pr), len(pr), _p(k),
                                                  len(k)), "wgcs_rekey_recv_gate_host")


def _jobs(peer, count, status, max_segs):
    pe, c, st = _in(peer, np.uint32), _in(count, np.int32), _in(status, np.int32)
    if len(st) != len(c) or len(pe) != len(c) * max_segs:
        raise ValueError("count and status hold one row per job, peer max_segs words per job")
    return pe, c, st


def send_gate_host(peer, count, status_in, max_segs: int, now_ns: int, peer_rows, kp, send_nonce, limit: int, rekey,
                   status_out) -> None:
    """wgcs_rekey_send_gate_host: send_gate_batch on numpy arrays.  `rekey`
    and `status_out` (int32) are written in place."""
    out = _host(status_out, np.int32, "status_out")
    # in place: the same memory goes in and out
    pe, c, st = _jobs(peer, count, out[:np.size(count)] if status_in is status_out else status_in, max_segs)
    pr, k, r = _tables(peer_rows, kp, rekey)
    sn = _in(send_nonce, np.uint64)
    if len(out) < len(c):
        raise ValueError("status_out holds one row per job")
    _status(_lib.load().wgcs_rekey_send_gate_host(_p(pe), _p(c), _p(st), len(c), max_segs, now_ns, _p(pr), len(pr), _p(k),
                                                  len(k), _p(sn), len(sn), C.c_uint64(limit), _p(r), _p(out)),
            "wgcs_rekey_send_gate_host")


def sent_host(peer, count, status, job_key, max_segs: int, now_ns: int, peer_rows, kp, send_nonce, limit: int,
              rekey) -> None:
    """wgcs_rekey_sent_host: sent_batch on numpy arrays.  `rekey` is written in place."""
    pe, c, st = _jobs(peer, count, status, max_segs)
    jk = _in(job_key, np.uint32)
    pr, k, r = _tables(peer_rows, kp, rekey)
    sn = _in(send_nonce, np.uint64)
    if len(jk) != len(c):
        raise ValueError("job_key holds one word per job")
    _status(_lib.load().wgcs_rekey_sent_host(_p(pe), _p(c), _p(st), _p(jk), len(c), max_segs, now_ns, _p(pr), len(pr),
                                             _p(k), len(k), _p(sn), len(sn), C.c_uint64(limit), _p(r)),
            "wgcs_rekey_sent_host")


def received_host(groups, calls_per_batch: int, now_ns: int, peer_rows, kp, rekey) -> None:
    """wgcs_rekey_received_host: received_batch on numpy arrays.  `rekey` is written in place."""
    g = _in(groups, WRITE_GROUP_DTYPE)
    pr, k, r = _tables(peer_rows, kp, rekey)
    if calls_per_batch < 1 or len(g) % calls_per_batch:
        raise ValueError("groups holds calls_per_batch rows per batch")
    _status(_lib.load().wgcs_rekey_received_host(_p(g), len(g) // calls_per_batch, calls_per_batch, now_ns, _p(pr),
                                                 len(pr), _p(k), len(k), _p(r)), "wgcs_rekey_received_host")


def responded_host(resp, gate, now_ns: int, rekey) -> None:
    """wgcs_rekey_responded_host: responded_batch on numpy arrays.  `rekey` is written in place."""
    d, g, r = _in(resp, HS_RESP_DTYPE), _in(gate, np.int32), _host(rekey, REKEY_DTYPE, "rekey")
    if len(g) != len(d):
        raise ValueError("gate holds one row per descriptor")
    _status(_lib.load().wgcs_rekey_responded_host(_p(d), _p(g), len(d), now_ns, _p(r), len(r)),
            "wgcs_rekey_responded_host")


def start_host(now_ns: int, rekey, hs_peers, tickets, start, start_peer, count, status, reasons) -> None:
    """wgcs_rekey_start_host: start_batch on numpy arrays, in its passes.
    `rekey`, `start` (HS_START_DTYPE), `start_peer` (uint32), `count` (one
    uint32), `status` (int32) and `reasons` (uint32) are written in place."""
    r, hp, t = _host(rekey, REKEY_DTYPE, "rekey"), _in(hs_peers, HS_PEER_DTYPE), _in(tickets, HS_START_DTYPE)
    d, sp = _host(start, HS_START_DTYPE, "start"), _host(start_peer, np.uint32, "start_peer")
    n, st, why = _host(count, np.uint32, "count"), _host(status, np.int32, "status"), _host(reasons, np.uint32, "reasons")
    if len(hp) != len(r) or len(st) < len(r) or len(why) < len(r) or len(d) < len(t) or len(sp) < len(t) or len(n) < 1:
        raise ValueError("hs_peers, status and reasons hold one row per rekey row, start and start_peer one per ticket")
    _status(_lib.load().wgcs_rekey_start_host(now_ns, _p(r), _p(hp), len(r), _p(t), len(t), _p(d), _p(sp), _p(n), _p(st),
                                              _p(why)), "wgcs_rekey_start_host")
