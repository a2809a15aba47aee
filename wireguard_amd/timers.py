"""Host-side mirror of the peer timers (package `device`: timers.go, with
send.go:85-87, :117-126, :158-160, :193-209 and :498-510, receive.go:311-312,
:339-348, :422-427 and :486-494, peer.go:241-252) over the C ABI.

Names and argument meaning follow the reference:
  sent_batch         traversal, packet sent and data sent behind send_assign_batch          send.go:498-510
  received_batch     traversal, packet received and data received behind write_build_batch  receive.go:486-494
  initiated_batch    !isRetry and timersHandshakeInitiated behind rekey.start_batch and
                     noise.initiate_batch                                                   send.go:85-87, :117-126
  responded_batch    the responder's hooks behind respond_batch               receive.go:311-312, send.go:158-160
  finished_batch     the initiator's hooks behind begin_initiator_batch                     receive.go:339-348
  rotated_batch      timersHandshakeComplete behind keypairs.received_batch                 receive.go:422-427
  expire_batch       the five expiry bodies over the peer rows: want bits for rekey.start_batch, keepalive
                     jobs for send_assign_batch, ZeroAndFlushAll's keypair part             timers.go:73-144
  *_host             those seven on host memory (numpy arrays), in row order
One TIMERS_DTYPE row sits beside every KEYPAIRS_DTYPE and REKEY_DTYPE row.  The
clock is the caller's: one int64 of nanoseconds per call; the jitter of
timers.go:204 and :271 is jitter_ms(seed, row) of a seed the caller passes.  The
row functions and the kernels live in libwgcsum.so (wgcs_timers.h,
timers_kernels.hip); nothing here computes but jitter_ms, which restates the
library's mix for callers that predict a deadline.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (REKEY_WANT_NEW_HANDSHAKE, REKEY_WANT_RETRY, TIMER_KEEPALIVE, TIMER_NEW_HANDSHAKE,
                   TIMER_RESEND_HANDSHAKE, TIMER_SEND_KEEPALIVE, TIMER_ZERO_OUT_KEYS, TIMERS_ACT_DEFERRED,
                   TIMERS_ACT_FLUSH_STAGED, TIMERS_ACT_GAVE_UP, TIMERS_ACT_KEEPALIVE, TIMERS_ACT_ZEROED, TIMERS_ACTIVE,
                   TIMERS_CLEAR_SRC, TIMERS_JITTER_MAX_MS, TIMERS_KEEPALIVE_NOW, TIMERS_MAX_ATTEMPTS,
                   TIMERS_NEED_ANOTHER, TIMERS_ZERO_KEYS_NS)
from .cookie import _status
from .keypairs import KEYPAIRS_DTYPE
from .noise import HS_RESP_DTYPE, HS_STATE_DTYPE, PEER_KEY_DTYPE, _host
from .rekey import REKEY_DTYPE
from .router import SESSION_SLOT_DTYPE
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE, _rows
from .tun import _ptr
from .writeplan import WRITE_GROUP_DTYPE

TIMERS_DTYPE = np.dtype([("deadline_ns", "<i8", (5,)), ("last_handshake_ns", "<i8"), ("pending", "<u4"),
                         ("attempts", "<u4"), ("flags", "<u4"), ("keepalive_interval_s", "<u4")])  # wgcs_timers
assert TIMERS_DTYPE.itemsize == 64

__all__ = ["TIMERS_DTYPE", "TIMER_NEW_HANDSHAKE", "TIMER_RESEND_HANDSHAKE", "TIMER_SEND_KEEPALIVE", "TIMER_KEEPALIVE",
           "TIMER_ZERO_OUT_KEYS", "TIMERS_ACTIVE", "TIMERS_NEED_ANOTHER", "TIMERS_CLEAR_SRC", "TIMERS_KEEPALIVE_NOW",
           "TIMERS_JITTER_MAX_MS", "TIMERS_MAX_ATTEMPTS", "TIMERS_ZERO_KEYS_NS", "TIMERS_ACT_KEEPALIVE",
           "TIMERS_ACT_DEFERRED", "TIMERS_ACT_FLUSH_STAGED", "TIMERS_ACT_ZEROED", "TIMERS_ACT_GAVE_UP",
           "REKEY_WANT_NEW_HANDSHAKE", "REKEY_WANT_RETRY", "timers_table", "jitter_ms", "sent_batch", "received_batch",
           "initiated_batch", "responded_batch", "finished_batch", "rotated_batch", "expire_batch", "sent_host",
           "received_host", "initiated_host", "responded_host", "finished_host", "rotated_host", "expire_host"]

_U4, _I4, _U1 = np.dtype("<u4"), np.dtype("<i4"), np.dtype("u1")


def timers_table(n_peers: int, keepalive_interval_s=0, active: bool = True) -> np.ndarray:
    """n_peers TIMERS_DTYPE rows as timersInit and timersStart leave them
    (timers.go:146-158): nothing pending, no attempts, no flag but
    TIMERS_ACTIVE when `active`; `keepalive_interval_s` is a number or one per
    row."""
    t = np.zeros(n_peers, TIMERS_DTYPE)
    t["flags"] = TIMERS_ACTIVE if active else 0
    t["keepalive_interval_s"] = keepalive_interval_s
    return t


def jitter_ms(seed: int, row: int) -> int:
    """wgcs_timers_jitter_ms restated: the milliseconds, in [0, 334), that peer
    row `row` adds under `seed` where timers.go draws rand.Int64N(334)."""
    m = 0xFFFFFFFF
    x = (seed ^ (row * 0x9E3779B9)) & m
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return (x * TIMERS_JITTER_MAX_MS) >> 32


def _count(x, dtype, given):
    return (0 if x is None else _rows(x, dtype)) if given is None else given


def sent_batch(dev, sizes, peer, count, status, job_key, max_segs: int, now_ns: int, jitter_seed: int, peer_rows,
               timers, stream=None, n_jobs: int | None = None, n_ids: int | None = None,
               n_peers: int | None = None) -> None:
    """Asynchronous wgcs_timers_sent_batch behind send_assign_batch: `sizes`
    (int32 per slot), `peer`, `count` and `status` are its inputs, `job_key` its
    output; a kept job runs traversal and packet sent on its peer's TIMERS_DTYPE
    row, and data sent if one of its sizes is not zero.  Only `timers` is
    written.  Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_timers_sent_batch(
        dev.h, _ptr(sizes), _ptr(peer), _ptr(count), _ptr(status), _ptr(job_key), _count(count, _I4, n_jobs), max_segs,
        now_ns, jitter_seed, _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(timers),
        _count(timers, TIMERS_DTYPE, n_peers), s))


def received_batch(dev, groups, calls_per_batch: int, now_ns: int, peer_rows, timers, stream=None,
                   n_batches: int | None = None, n_ids: int | None = None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_timers_received_batch behind write_build_batch over
    its WRITE_GROUP_DTYPE rows (n_batches * calls_per_batch of them).  Only
    `timers` is written."""
    s = getattr(stream, "cuda_stream", stream)
    if n_batches is None:
        n_batches = _count(groups, WRITE_GROUP_DTYPE, None) // max(calls_per_batch, 1)
    dev._check(dev.lib.wgcs_timers_received_batch(
        dev.h, _ptr(groups), n_batches, calls_per_batch, now_ns, _ptr(peer_rows), _count(peer_rows, _U4, n_ids),
        _ptr(timers), _count(timers, TIMERS_DTYPE, n_peers), s))


def initiated_batch(dev, reasons, start_peer, init_status, now_ns: int, jitter_seed: int, timers, stream=None,
                    n_tickets: int | None = None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_timers_initiated_batch behind rekey.start_batch and
    noise.initiate_batch: `reasons` (uint32 per peer row) and `start_peer`
    (uint32 per ticket) are start's outputs, `init_status` (int32 per ticket)
    initiate's.  Only `timers` is written."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_timers_initiated_batch(
        dev.h, _ptr(reasons), _ptr(start_peer), _ptr(init_status), _count(start_peer, _U4, n_tickets), now_ns,
        jitter_seed, _ptr(timers), _count(timers, TIMERS_DTYPE, n_peers), s))


def responded_batch(dev, resp, gate, now_ns: int, timers, stream=None, n: int | None = None,
                    n_peers: int | None = None) -> None:
    """Asynchronous wgcs_timers_responded_batch behind respond_batch: `resp`
    are its HS_RESP_DTYPE descriptors and `gate` its status.  Only `timers` is
    written."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_timers_responded_batch(dev.h, _ptr(resp), _ptr(gate), _count(resp, HS_RESP_DTYPE, n), now_ns,
                                                   _ptr(timers), _count(timers, TIMERS_DTYPE, n_peers), s))


def finished_batch(dev, arena, pkts, gate, begun, now_ns: int, hs_slots, states, timers, rekey, stream=None,
                   n: int | None = None, n_hs_slots: int | None = None, n_states: int | None = None,
                   n_peers: int | None = None) -> None:
    """Asynchronous wgcs_timers_finished_batch behind begin_initiator_batch
    over the same rows: `gate` is finish_batch's verdict, `begun`
    begin_initiator_batch's status, `hs_slots` and `states` as it read them.
    `timers` and the flags of `rekey` are written."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_timers_finished_batch(
        dev.h, _ptr(arena), _ptr(pkts), _ptr(gate), _ptr(begun), _count(pkts, AEAD_PKT_DTYPE, n), now_ns, _ptr(hs_slots),
        _count(hs_slots, SESSION_SLOT_DTYPE, n_hs_slots), _ptr(states), _count(states, HS_STATE_DTYPE, n_states),
        _ptr(timers), _ptr(rekey), _count(timers, TIMERS_DTYPE, n_peers), s))


def rotated_batch(dev, pkts, rotated, now_ns: int, key_peer, peer_rows, timers, rekey, stream=None,
                  n: int | None = None, n_keys: int | None = None, n_ids: int | None = None,
                  n_peers: int | None = None) -> None:
    """Asynchronous wgcs_timers_rotated_batch behind keypairs.received_batch:
    `pkts` are the receive batch's rows and `rotated` (uint32) its output.
    `timers` and the flags of `rekey` are written."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_timers_rotated_batch(
        dev.h, _ptr(pkts), _ptr(rotated), _count(pkts, AEAD_PKT_DTYPE, n), now_ns, _ptr(key_peer),
        _count(key_peer, _U4, n_keys), _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(timers), _ptr(rekey),
        _count(timers, TIMERS_DTYPE, n_peers), s))


def expire_batch(dev, now_ns: int, timers, rekey, table, staged, kp, slots, peer_keys, keys, key_peer, ka_peer, ka_count,
                 ka_sizes, ka_status, n_ka, actions, work, stream=None, n_peers: int | None = None,
                 n_slots: int | None = None, n_peer_slots: int | None = None, n_keys: int | None = None,
                 n_ka_max: int | None = None, work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_timers_expire_batch over the peer rows: `timers`,
    `rekey`, `table` (PEER_KEY_DTYPE, only read) and `kp` hold one row per
    peer, `staged` (uint32 per peer row, or None) is non-zero where the host
    has staged packets; `slots`, `peer_keys`, `keys` and `key_peer` are what
    zeroOutKeys deletes from, as keypairs.received_batch takes them.  Writes
    the keepalive jobs `ka_peer` (uint32), `ka_count`, `ka_sizes`, `ka_status`
    (int32; n_ka_max rows each, the tail {PEER_NONE, 0, 0, 0}) for
    send_assign_batch with max_segs == 1, `n_ka` (one uint32) and `actions`
    (uint32 per peer row: TIMERS_ACT_*, bits 0..4 the timers that fired).
    `work` is keystate.work_bytes(n_peers) of 16-byte-aligned scratch."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_timers_expire_batch(
        dev.h, now_ns, _ptr(timers), _ptr(rekey), _ptr(table), _count(timers, TIMERS_DTYPE, n_peers), _ptr(staged),
        _ptr(kp), _ptr(slots), _count(slots, SESSION_SLOT_DTYPE, n_slots), _ptr(peer_keys),
        _count(peer_keys, SESSION_SLOT_DTYPE, n_peer_slots), _ptr(keys), _ptr(key_peer),
        _count(keys, AEAD_KEY_DTYPE, n_keys), _count(ka_peer, _U4, n_ka_max), _ptr(ka_peer), _ptr(ka_count),
        _ptr(ka_sizes), _ptr(ka_status), _ptr(n_ka), _ptr(actions), _ptr(work), _count(work, _U1, work_bytes), s))


def _in(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a: np.ndarray):
    return a.ctypes.data if len(a) else None


def _pair(timers, rekey):
    t, r = _host(timers, TIMERS_DTYPE, "timers"), _host(rekey, REKEY_DTYPE, "rekey")
    if len(r) != len(t):
        raise ValueError("rekey holds one row per timers row")
    return t, r


def sent_host(sizes, peer, count, status, job_key, max_segs: int, now_ns: int, jitter_seed: int, peer_rows,
              timers) -> None:
    """wgcs_timers_sent_host: sent_batch on numpy arrays.  `timers` is written in place."""
    sz, pe, c, st = _in(sizes, np.int32), _in(peer, np.uint32), _in(count, np.int32), _in(status, np.int32)
    jk, pr, t = _in(job_key, np.uint32), _in(peer_rows, np.uint32), _host(timers, TIMERS_DTYPE, "timers")
    if len(st) != len(c) or len(jk) != len(c) or len(pe) != len(c) * max_segs or len(sz) != len(pe):
        raise ValueError("count, status and job_key hold one row per job, sizes and peer max_segs words per job")
    _status(_lib.load().wgcs_timers_sent_host(_p(sz), _p(pe), _p(c), _p(st), _p(jk), len(c), max_segs, now_ns,
                                              jitter_seed, _p(pr), len(pr), _p(t), len(t)), "wgcs_timers_sent_host")


def received_host(groups, calls_per_batch: int, now_ns: int, peer_rows, timers) -> None:
    """wgcs_timers_received_host: received_batch on numpy arrays.  `timers` is written in place."""
    g, pr, t = _in(groups, WRITE_GROUP_DTYPE), _in(peer_rows, np.uint32), _host(timers, TIMERS_DTYPE, "timers")
    if calls_per_batch < 1 or len(g) % calls_per_batch:
        raise ValueError("groups holds calls_per_batch rows per batch")
    _status(_lib.load().wgcs_timers_received_host(_p(g), len(g) // calls_per_batch, calls_per_batch, now_ns, _p(pr),
                                                  len(pr), _p(t), len(t)), "wgcs_timers_received_host")


def initiated_host(reasons, start_peer, init_status, now_ns: int, jitter_seed: int, timers) -> None:
    """wgcs_timers_initiated_host: initiated_batch on numpy arrays, in its two
    passes.  `timers` is written in place."""
    why, sp, st = _in(reasons, np.uint32), _in(start_peer, np.uint32), _in(init_status, np.int32)
    t = _host(timers, TIMERS_DTYPE, "timers")
    if len(why) < len(t) or len(st) != len(sp):
        raise ValueError("reasons holds one word per timers row, init_status one per ticket")
    _status(_lib.load().wgcs_timers_initiated_host(_p(why), _p(sp), _p(st), len(sp), now_ns, jitter_seed, _p(t), len(t)),
            "wgcs_timers_initiated_host")


def responded_host(resp, gate, now_ns: int, timers) -> None:
    """wgcs_timers_responded_host: responded_batch on numpy arrays.  `timers` is written in place."""
    d, g, t = _in(resp, HS_RESP_DTYPE), _in(gate, np.int32), _host(timers, TIMERS_DTYPE, "timers")
    if len(g) != len(d):
        raise ValueError("gate holds one row per descriptor")
    _status(_lib.load().wgcs_timers_responded_host(_p(d), _p(g), len(d), now_ns, _p(t), len(t)),
            "wgcs_timers_responded_host")


def finished_host(arena, pkts, gate, begun, now_ns: int, hs_slots, states, timers, rekey) -> None:
    """wgcs_timers_finished_host: finished_batch on numpy arrays.  `timers` and `rekey` are written in place."""
    a, p, g, b = _in(arena, np.uint8), _in(pkts, AEAD_PKT_DTYPE), _in(gate, np.int32), _in(begun, np.int32)
    hs, st = _in(hs_slots, SESSION_SLOT_DTYPE), _in(states, HS_STATE_DTYPE)
    t, r = _pair(timers, rekey)
    if len(g) != len(p) or len(b) != len(p):
        raise ValueError("gate and begun hold one row per packet")
    _status(_lib.load().wgcs_timers_finished_host(_p(a), _p(p), _p(g), _p(b), len(p), now_ns, _p(hs), len(hs), _p(st),
                                                  len(st), _p(t), _p(r), len(t)), "wgcs_timers_finished_host")


def rotated_host(pkts, rotated, now_ns: int, key_peer, peer_rows, timers, rekey) -> None:
    """wgcs_timers_rotated_host: rotated_batch on numpy arrays.  `timers` and `rekey` are written in place."""
    p, ro, kpr, pr = _in(pkts, AEAD_PKT_DTYPE), _in(rotated, np.uint32), _in(key_peer, np.uint32), _in(peer_rows, np.uint32)
    t, r = _pair(timers, rekey)
    if len(ro) != len(p):
        raise ValueError("rotated holds one word per packet")
    _status(_lib.load().wgcs_timers_rotated_host(_p(p), _p(ro), len(p), now_ns, _p(kpr), len(kpr), _p(pr), len(pr), _p(t),
                                                 _p(r), len(t)), "wgcs_timers_rotated_host")


def expire_host(now_ns: int, timers, rekey, table, staged, kp, slots, peer_keys, keys, key_peer, ka_peer, ka_count,
                ka_sizes, ka_status, n_ka, actions, n_ka_max: int | None = None) -> None:
    """wgcs_timers_expire_host: expire_batch on numpy arrays, in its passes.
    `timers`, `rekey`, `kp`, `slots`, `peer_keys`, `keys`, `key_peer`, the four
    job arrays, `n_ka` and `actions` are written in place; `n_ka_max` defaults
    to the length of `ka_peer`."""
    t, r = _pair(timers, rekey)
    tb, k = _in(table, PEER_KEY_DTYPE), _host(kp, KEYPAIRS_DTYPE, "kp")
    stg = None if staged is None else _in(staged, np.uint32)
    sl, pk = _host(slots, SESSION_SLOT_DTYPE, "slots"), _host(peer_keys, SESSION_SLOT_DTYPE, "peer_keys")
    ks, kpr = _host(keys, AEAD_KEY_DTYPE, "keys"), _host(key_peer, np.uint32, "key_peer")
    kap, kac = _host(ka_peer, np.uint32, "ka_peer"), _host(ka_count, np.int32, "ka_count")
    kas, kat = _host(ka_sizes, np.int32, "ka_sizes"), _host(ka_status, np.int32, "ka_status")
    n, act = _host(n_ka, np.uint32, "n_ka"), _host(actions, np.uint32, "actions")
    room = len(kap) if n_ka_max is None else n_ka_max
    if (len(tb) != len(t) or len(k) != len(t) or len(act) < len(t) or len(kpr) != len(ks) or len(n) < 1 or
            (stg is not None and len(stg) != len(t)) or min(len(kap), len(kac), len(kas), len(kat)) < room):
        raise ValueError("table, kp, staged and actions hold one row per timers row, the job arrays n_ka_max rows")
    _status(_lib.load().wgcs_timers_expire_host(
        now_ns, _p(t), _p(r), _p(tb), len(t), None if stg is None else _p(stg), _p(k), _p(sl), len(sl), _p(pk), len(pk),
        _p(ks), _p(kpr), len(ks), room, _p(kap), _p(kac), _p(kas), _p(kat), _p(n), _p(act)), "wgcs_timers_expire_host")
