"""Host-side mirror of the cookie generator (package `device`, cookie.go:247-339
and receive.go:246-269 where RoutineHandshake hands it a cookie reply) over
the C ABI.

Names and argument meaning follow the reference:
  gen_build         CookieGenerator.Init per peer row                         cookie.go:269-282
  initiated_batch   AddMACs' lastMAC1 behind noise.initiate_batch             cookie.go:301-302
  responded_batch   the same behind noise.respond_batch
  consume_batch     the cookie-reply case of RoutineHandshake + ConsumeReply  receive.go:246-269, cookie.go:319-339
  age_batch         the CookieRefreshTime rule of AddMACs                     cookie.go:306
  *_host            those four on host memory (numpy arrays), rows in order
A table is one COOKIE_GEN_DTYPE row per row of the peer table; the cookie and
its valid bit live in the HS_PEER_DTYPE rows that noise.accept_batch and
rekey.start_batch read.  The clock is the caller's: one int64 of nanoseconds
per call.  peer.isRunning, index allocation and -- should the host ever write
a cookie into the HS_PEER_DTYPE rows itself -- cookie_set_at_ns stay with the
caller.  The row functions and the kernels live in libwgcsum.so
(wgcs_cookiegen.h, cookiegen_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import COOKIE_GEN_HAS_MAC1, COOKIE_REFRESH_NS, HS_COOKIE_KEPT
from .cookie import _status
from .noise import (HS_PEER_DTYPE, HS_RESP_DTYPE, HS_START_DTYPE, HS_STATE_DTYPE, INITIATION_PITCH, PEER_KEY_DTYPE,
                    RESPONSE_PITCH, _host)
from .router import SESSION_SLOT_DTYPE
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import _ptr

COOKIE_GEN_DTYPE = np.dtype([("cookie_key", "u1", (32,)), ("last_mac1", "u1", (16,)), ("cookie_set_at_ns", "<i8"),
                             ("flags", "<u4"), ("claim", "<u4")])  # wgcs_cookie_gen
CONSUME_WORK_BYTES = 16  # consume_batch's scratch per row
assert COOKIE_GEN_DTYPE.itemsize == 64

__all__ = ["COOKIE_GEN_DTYPE", "COOKIE_GEN_HAS_MAC1", "COOKIE_REFRESH_NS", "CONSUME_WORK_BYTES", "HS_COOKIE_KEPT",
           "gen_build", "initiated_batch", "responded_batch", "consume_batch", "age_batch", "initiated_host",
           "responded_host", "consume_host", "age_host"]

_U4, _I4 = np.dtype("<u4"), np.dtype("<i4")


def _count(x, dtype, given):
    return (0 if x is None else _rows(x, dtype)) if given is None else given


def _in(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a: np.ndarray):
    return a.ctypes.data if len(a) else None


def gen_build(table) -> np.ndarray:
    """wgcs_cookie_gen_build: one COOKIE_GEN_DTYPE row per PEER_KEY_DTYPE row of
    `table`, cookie_key from its public key and everything else zero."""
    t = _in(table, PEER_KEY_DTYPE)
    rows = np.zeros(len(t), COOKIE_GEN_DTYPE)
    _status(_lib.load().wgcs_cookie_gen_build(_p(t), len(t), _p(rows)), "wgcs_cookie_gen_build")
    return rows


def initiated_batch(dev, start, status, msgs, gen, stream=None, n: int | None = None,
                    n_peers: int | None = None) -> None:
    """Asynchronous wgcs_cookie_initiated_batch behind noise.initiate_batch:
    `start` (HS_START_DTYPE), `status` and `msgs` are that call's; the MAC1 of
    every HS_INITIATED descriptor goes into its peer's COOKIE_GEN_DTYPE row of
    `gen`, the highest descriptor's where several name one peer.  Only `gen` is
    written.  Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_cookie_initiated_batch(dev.h, _ptr(start), _ptr(status), _ptr(msgs),
                                                   _count(start, HS_START_DTYPE, n), _ptr(gen),
                                                   _count(gen, COOKIE_GEN_DTYPE, n_peers), s))


def responded_batch(dev, resp, status, msgs, gen, stream=None, n: int | None = None,
                    n_peers: int | None = None) -> None:
    """Asynchronous wgcs_cookie_responded_batch behind noise.respond_batch:
    initiated_batch for HS_RESP_DTYPE descriptors and HS_RESPONDED."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_cookie_responded_batch(dev.h, _ptr(resp), _ptr(status), _ptr(msgs),
                                                   _count(resp, HS_RESP_DTYPE, n), _ptr(gen),
                                                   _count(gen, COOKIE_GEN_DTYPE, n_peers), s))


def consume_batch(dev, arena, pkts, types, now_ns: int, hs_slots, states, slots, key_peer, peer_rows, gen, peers, work,
                  verdict, stream=None, n: int | None = None, n_hs_slots: int | None = None,
                  n_states: int | None = None, n_slots: int | None = None, n_keys: int | None = None,
                  n_ids: int | None = None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_cookie_consume_batch over classify_batch's pkts
    (AEAD_PKT_DTYPE rows) and types (int32).  `hs_slots` and `states` are the
    initiator's slots and HS_STATE_DTYPE table, `slots`, `key_peer` and
    `peer_rows` the session table, the key -> peer id column and
    noise.peer_rows_build's rows; `gen` (COOKIE_GEN_DTYPE) and `peers`
    (HS_PEER_DTYPE) hold one row per peer-table row and are written; `work` is
    CONSUME_WORK_BYTES of scratch per row, all zero afterwards.  verdict[q]
    (int32) = HS_NONE, HS_COOKIE_KEPT, ERR_INVALID_ARG, ERR_NO_PEER,
    ERR_NO_HANDSHAKE or ERR_AUTH.  Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_cookie_consume_batch(
        dev.h, _ptr(arena), _ptr(pkts), _ptr(types), _count(pkts, AEAD_PKT_DTYPE, n), now_ns, _ptr(hs_slots),
        _count(hs_slots, SESSION_SLOT_DTYPE, n_hs_slots), _ptr(states), _count(states, HS_STATE_DTYPE, n_states),
        _ptr(slots), _count(slots, SESSION_SLOT_DTYPE, n_slots), _ptr(key_peer), _count(key_peer, _U4, n_keys),
        _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(gen), _ptr(peers), _count(gen, COOKIE_GEN_DTYPE, n_peers),
        _ptr(work), _ptr(verdict), s))


def age_batch(dev, now_ns: int, gen, peers, stream=None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_cookie_age_batch in front of noise.accept_batch and
    rekey.start_batch: HS_PEER_COOKIE is cleared in every HS_PEER_DTYPE row
    whose cookie was set more than COOKIE_REFRESH_NS before now_ns."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_cookie_age_batch(dev.h, now_ns, _ptr(gen), _ptr(peers),
                                             _count(gen, COOKIE_GEN_DTYPE, n_peers), s))


def initiated_host(start, status, msgs, gen) -> None:
    """wgcs_cookie_initiated_host: initiated_batch on numpy arrays, in its two passes.  `gen` is written in place."""
    d, st, m = _in(start, HS_START_DTYPE), _in(status, np.int32), _in(msgs, np.uint8)
    g = _host(gen, COOKIE_GEN_DTYPE, "gen")
    if len(st) != len(d) or len(m) < INITIATION_PITCH * len(d):
        raise ValueError("status and msgs hold one row per descriptor")
    _status(_lib.load().wgcs_cookie_initiated_host(_p(d), _p(st), _p(m), len(d), _p(g), len(g)),
            "wgcs_cookie_initiated_host")


def responded_host(resp, status, msgs, gen) -> None:
    """wgcs_cookie_responded_host: responded_batch on numpy arrays, in its two passes.  `gen` is written in place."""
    d, st, m = _in(resp, HS_RESP_DTYPE), _in(status, np.int32), _in(msgs, np.uint8)
    g = _host(gen, COOKIE_GEN_DTYPE, "gen")
    if len(st) != len(d) or len(m) < RESPONSE_PITCH * len(d):
        raise ValueError("status and msgs hold one row per descriptor")
    _status(_lib.load().wgcs_cookie_responded_host(_p(d), _p(st), _p(m), len(d), _p(g), len(g)),
            "wgcs_cookie_responded_host")


def consume_host(arena, pkts, types, now_ns: int, hs_slots, states, slots, key_peer, peer_rows, gen, peers,
                 work=None, verdict=None) -> np.ndarray:
    """wgcs_cookie_consume_host: consume_batch on numpy arrays, in its two
    passes.  `gen`, `peers` and, when given, `work` (uint8) and `verdict`
    (int32) are written in place; returns the verdicts."""
    a, p, ty = _in(arena, np.uint8), _in(pkts, AEAD_PKT_DTYPE), _in(types, np.int32)
    hs, st, sl = _in(hs_slots, SESSION_SLOT_DTYPE), _in(states, HS_STATE_DTYPE), _in(slots, SESSION_SLOT_DTYPE)
    kpr, pr = _in(key_peer, np.uint32), _in(peer_rows, np.uint32)
    g, ps = _host(gen, COOKIE_GEN_DTYPE, "gen"), _host(peers, HS_PEER_DTYPE, "peers")
    n = len(p)
    w = np.zeros(CONSUME_WORK_BYTES * n, np.uint8) if work is None else _host(work, np.uint8, "work")
    v = np.empty(n, np.int32) if verdict is None else _host(verdict, np.int32, "verdict")
    if len(ty) != n or len(w) < CONSUME_WORK_BYTES * n or len(v) < n or len(ps) != len(g):
        raise ValueError("types, work and verdict hold one row per packet, peers one row per gen row")
    _status(_lib.load().wgcs_cookie_consume_host(_p(a), _p(p), _p(ty), n, now_ns, _p(hs), len(hs), _p(st), len(st),
                                                 _p(sl), len(sl), _p(kpr), len(kpr), _p(pr), len(pr), _p(g), _p(ps),
                                                 len(g), _p(w), _p(v)), "wgcs_cookie_consume_host")
    return v


def age_host(now_ns: int, gen, peers) -> None:
    """wgcs_cookie_age_host: age_batch on numpy arrays.  `peers` is written in place."""
    g, ps = _in(gen, COOKIE_GEN_DTYPE), _host(peers, HS_PEER_DTYPE, "peers")
    if len(ps) != len(g):
        raise ValueError("peers holds one row per gen row")
    _status(_lib.load().wgcs_cookie_age_host(now_ns, _p(g), _p(ps), len(g)), "wgcs_cookie_age_host")
