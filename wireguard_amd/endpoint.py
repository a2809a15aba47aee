"""Host-side mirror of the peer endpoints (package `conn`, bind.go:308-319 and
sticky.go:46-94; package `device`, peer.go:195-221, :281-297 and the three live
call sites of SetEndpointFromPacket, receive.go:314, :335, :487) over the C ABI.

Names and argument meaning follow the reference:
  table, row           a peer table of ENDPOINT_DTYPE rows; one NetEndpoint as a row
  recv_batch           the endpoints ReceiveIPvX hands back, behind conn's split   bind.go:308-319
  set_received_batch   SetEndpointFromPacket behind writeplan.build_batch          receive.go:487
  set_accepted_batch   ... behind noise.accept_batch                               :314
  set_finished_batch   ... behind noise.finish_batch                               :335
  dst_jobs_batch       Peer.Send up to bind.Send for the jobs of a send batch      peer.go:201-211
  dst_initiated_batch  ... for the initiations of noise.initiate_batch
  dst_responded_batch  ... for the responses of noise.respond_batch
  coalesce_dst_batch   coalesceMessages with the address family per batch          bind.go:599-662
  *_host               the seven endpoint calls on host memory (numpy arrays), rows in order
A table is one ENDPOINT_DTYPE row and one uint32 claim word (0 outside a call)
per row of the peer table; clearSrcOnTx is TIMERS_CLEAR_SRC of the peer's
TIMERS_DTYPE row.  The recvmmsg Addr of each landed message, the UAPI's
endpoint write, the route listener's flag, txBytes and sending stay with the
caller.  The row functions and the kernels live in libwgcsum.so
(wgcs_endpoint.h, endpoint_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ERR_NO_ENDPOINT, TIMERS_CLEAR_SRC
from .cookie import SRC_ADDR_DTYPE, _status, src_addr
from .noise import HS_RESP_DTYPE, HS_START_DTYPE, HS_STATE_DTYPE, _host
from .router import SESSION_SLOT_DTYPE
from .timers import TIMERS_DTYPE
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import _ptr
from .writeplan import WRITE_GROUP_DTYPE

ENDPOINT_DTYPE = np.dtype([("dst", SRC_ADDR_DTYPE), ("src_len", "u1"), ("pad", "u1", (3,)),
                           ("src", "u1", (40,))])  # wgcs_endpoint
assert ENDPOINT_DTYPE.itemsize == 64

__all__ = ["ENDPOINT_DTYPE", "ERR_NO_ENDPOINT", "TIMERS_CLEAR_SRC", "table", "row", "recv_batch", "set_received_batch",
           "set_accepted_batch", "set_finished_batch", "dst_jobs_batch", "dst_initiated_batch", "dst_responded_batch",
           "coalesce_dst_batch", "recv_host", "set_received_host", "set_accepted_host", "set_finished_host",
           "dst_jobs_host", "dst_initiated_host", "dst_responded_host"]

_U4, _I4 = np.dtype("<u4"), np.dtype("<i4")


def table(n_peers: int) -> tuple[np.ndarray, np.ndarray]:
    """A peer table without endpoints and its claim words: (ENDPOINT_DTYPE rows, uint32 words), all zero."""
    return np.zeros(n_peers, ENDPOINT_DTYPE), np.zeros(n_peers, np.uint32)


def row(ip, port: int, src: bytes = b"") -> np.ndarray:
    """One canonical ENDPOINT_DTYPE row: NetEndpoint{AddrPort: ip:port, src: src}."""
    if len(src) not in (0, 32, 40):
        raise ValueError("a sticky source of 0, 32 or 40 bytes")
    r = np.zeros(1, ENDPOINT_DTYPE)
    r["dst"] = src_addr(ip, port)
    r["src_len"] = len(src)
    r["src"][0, :len(src)] = np.frombuffer(bytes(src), np.uint8)
    return r


def _count(x, dtype, given):
    return (0 if x is None else _rows(x, dtype)) if given is None else given


def _in(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a):
    return a.ctypes.data if a is not None and len(a) else None


# ---------------------------------------------------------------- device calls
def recv_batch(dev, addr, src_from, size, oob, oob_stride: int, nn, n_msgs: int, n_batches: int, ep, addr_out=None,
               stream=None) -> None:
    """Asynchronous wgcs_endpoint_recv_batch behind wgcs_split_messages_batch
    (src_from = its d_src, size = its d_n_out; src_from None: no split ran).
    `addr` holds one SRC_ADDR_DTYPE row per slot, `oob` the control buffers at
    oob_stride bytes per slot with lengths `nn`; `ep` (ENDPOINT_DTYPE) and,
    when given, `addr_out` (SRC_ADDR_DTYPE: the screen's and the rate
    limiter's src) get one row per slot.  Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_endpoint_recv_batch(dev.h, _ptr(addr), _ptr(src_from), _ptr(size), _ptr(oob), oob_stride,
                                                _ptr(nn), n_msgs, n_batches, _ptr(ep), _ptr(addr_out), s))


def set_received_batch(dev, groups, calls_per_batch: int, ep, peer_rows, tab, claim, timers, stream=None,
                       n_batches: int | None = None, n_rows: int | None = None, n_ids: int | None = None,
                       n_peers: int | None = None) -> None:
    """Asynchronous wgcs_endpoint_set_received_batch behind
    writeplan.build_batch: the peer of every group with a tail takes
    ep[tail]; TIMERS_CLEAR_SRC is cleared in its `timers` row."""
    s = getattr(stream, "cuda_stream", stream)
    nb = _rows(groups, WRITE_GROUP_DTYPE) // calls_per_batch if n_batches is None else n_batches
    dev._check(dev.lib.wgcs_endpoint_set_received_batch(
        dev.h, _ptr(groups), nb, calls_per_batch, _ptr(ep), _count(ep, ENDPOINT_DTYPE, n_rows), _ptr(peer_rows),
        _count(peer_rows, _U4, n_ids), _ptr(tab), _ptr(claim), _ptr(timers), _count(tab, ENDPOINT_DTYPE, n_peers), s))


def set_accepted_batch(dev, resp, ep, tab, claim, timers, stream=None, n_tickets: int | None = None,
                       n_rows: int | None = None, n_peers: int | None = None) -> None:
    """Asynchronous wgcs_endpoint_set_accepted_batch behind noise.accept_batch
    over its descriptors: the peer of every one takes ep[init_row]."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_endpoint_set_accepted_batch(
        dev.h, _ptr(resp), _count(resp, HS_RESP_DTYPE, n_tickets), _ptr(ep), _count(ep, ENDPOINT_DTYPE, n_rows),
        _ptr(tab), _ptr(claim), _ptr(timers), _count(tab, ENDPOINT_DTYPE, n_peers), s))


def set_finished_batch(dev, arena, pkts, gate, hs_slots, states, ep, tab, claim, timers, stream=None,
                       n: int | None = None, n_hs_slots: int | None = None, n_states: int | None = None,
                       n_peers: int | None = None) -> None:
    """Asynchronous wgcs_endpoint_set_finished_batch behind noise.finish_batch
    (gate = its verdicts): the peer of every HS_FINISHED row q takes ep[q]."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_endpoint_set_finished_batch(
        dev.h, _ptr(arena), _ptr(pkts), _ptr(gate), _count(pkts, AEAD_PKT_DTYPE, n), _ptr(hs_slots),
        _count(hs_slots, SESSION_SLOT_DTYPE, n_hs_slots), _ptr(states), _count(states, HS_STATE_DTYPE, n_states),
        _ptr(ep), _ptr(tab), _ptr(claim), _ptr(timers), _count(tab, ENDPOINT_DTYPE, n_peers), s))


def dst_jobs_batch(dev, peer, count, status, job_key, max_segs: int, lens, nbufs, peer_rows, tab, timers, dst, dst_v6,
                   dst_status, tx_bytes, stream=None, n_jobs: int | None = None, n_ids: int | None = None,
                   n_peers: int | None = None) -> None:
    """Asynchronous wgcs_endpoint_dst_jobs_batch behind transport.seal_batch
    (lens = its out_len) and in front of coalesce_dst_batch: per job its
    ENDPOINT_DTYPE destination, 1 for a 16-byte address, 0 or ERR_NO_ENDPOINT
    (then nbufs[j] = 0) and the bytes to add to txBytes (uint64)."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_endpoint_dst_jobs_batch(
        dev.h, _ptr(peer), _ptr(count), _ptr(status), _ptr(job_key), _count(job_key, _U4, n_jobs), max_segs, _ptr(lens),
        _ptr(nbufs), _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(tab), _ptr(timers),
        _count(tab, ENDPOINT_DTYPE, n_peers), _ptr(dst), _ptr(dst_v6), _ptr(dst_status), _ptr(tx_bytes), s))


def dst_initiated_batch(dev, start, status, tab, timers, dst, dst_v6, dst_status, stream=None, n: int | None = None,
                        n_peers: int | None = None) -> None:
    """Asynchronous wgcs_endpoint_dst_initiated_batch behind
    noise.initiate_batch over its descriptors and status."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_endpoint_dst_initiated_batch(
        dev.h, _ptr(start), _ptr(status), _count(start, HS_START_DTYPE, n), _ptr(tab), _ptr(timers),
        _count(tab, ENDPOINT_DTYPE, n_peers), _ptr(dst), _ptr(dst_v6), _ptr(dst_status), s))


def dst_responded_batch(dev, resp, status, tab, timers, dst, dst_v6, dst_status, stream=None, n: int | None = None,
                        n_peers: int | None = None) -> None:
    """Asynchronous wgcs_endpoint_dst_responded_batch behind
    noise.respond_batch over its descriptors and status."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_endpoint_dst_responded_batch(
        dev.h, _ptr(resp), _ptr(status), _count(resp, HS_RESP_DTYPE, n), _ptr(tab), _ptr(timers),
        _count(tab, ENDPOINT_DTYPE, n_peers), _ptr(dst), _ptr(dst_v6), _ptr(dst_status), s))


def coalesce_dst_batch(dev, bufs, buf_stride: int, buf_cap: int, caps, lens, nbufs, max_bufs: int, n_batches: int,
                       dst_v6, n_msgs, msg_first, msg_len, msg_gso, stream=None) -> None:
    """Asynchronous wgcs_coalesce_messages_dst_batch: wgcs_coalesce_messages_batch
    with dst_v6[b] (int32, dst_jobs_batch's) as the family of batch b."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_coalesce_messages_dst_batch(dev.h, _ptr(bufs), buf_stride, buf_cap, _ptr(caps), _ptr(lens),
                                                        _ptr(nbufs), max_bufs, n_batches, _ptr(dst_v6), _ptr(n_msgs),
                                                        _ptr(msg_first), _ptr(msg_len), _ptr(msg_gso), s))


# ---------------------------------------------------------------- host forms
def recv_host(addr, src_from, size, oob, oob_stride: int, nn, n_msgs: int, n_batches: int, ep=None,
              addr_out=None) -> tuple[np.ndarray, np.ndarray]:
    """wgcs_endpoint_recv_host: recv_batch on numpy arrays.  Returns (ep,
    addr_out); arrays given for them are written in place."""
    n = n_msgs * n_batches
    a, sz, c = _in(addr, SRC_ADDR_DTYPE), _in(size, np.int32), _in(nn, np.int32)
    f = None if src_from is None else _in(src_from, np.int32)
    o = _in(oob, np.uint8)
    e = np.zeros(n, ENDPOINT_DTYPE) if ep is None else _host(ep, ENDPOINT_DTYPE, "ep")
    ao = np.zeros(n, SRC_ADDR_DTYPE) if addr_out is None else _host(addr_out, SRC_ADDR_DTYPE, "addr_out")
    if min(len(a), len(sz), len(c), len(e), len(ao)) < n or (f is not None and len(f) < n) or len(o) < n * oob_stride:
        raise ValueError("one row per slot and oob_stride bytes of control per slot")
    _status(_lib.load().wgcs_endpoint_recv_host(_p(a), _p(f), _p(sz), _p(o), oob_stride, _p(c), n_msgs, n_batches, _p(e),
                                                _p(ao)), "wgcs_endpoint_recv_host")
    return e, ao


def _tables(tab, claim, timers):
    t, c, tm = _host(tab, ENDPOINT_DTYPE, "table"), _host(claim, np.uint32, "claim"), _host(timers, TIMERS_DTYPE, "timers")
    if len(c) != len(t) or len(tm) != len(t):
        raise ValueError("claim and timers hold one row per table row")
    return t, c, tm


def set_received_host(groups, calls_per_batch: int, ep, peer_rows, tab, claim, timers) -> None:
    """wgcs_endpoint_set_received_host: `tab`, `claim` and `timers` are written in place."""
    g, e, pr = _in(groups, WRITE_GROUP_DTYPE), _in(ep, ENDPOINT_DTYPE), _in(peer_rows, np.uint32)
    t, c, tm = _tables(tab, claim, timers)
    if calls_per_batch < 1 or len(g) % calls_per_batch:
        raise ValueError("groups holds calls_per_batch rows per batch")
    _status(_lib.load().wgcs_endpoint_set_received_host(_p(g), len(g) // calls_per_batch, calls_per_batch, _p(e), len(e),
                                                        _p(pr), len(pr), _p(t), _p(c), _p(tm), len(t)),
            "wgcs_endpoint_set_received_host")


def set_accepted_host(resp, ep, tab, claim, timers) -> None:
    """wgcs_endpoint_set_accepted_host: `tab`, `claim` and `timers` are written in place."""
    d, e = _in(resp, HS_RESP_DTYPE), _in(ep, ENDPOINT_DTYPE)
    t, c, tm = _tables(tab, claim, timers)
    _status(_lib.load().wgcs_endpoint_set_accepted_host(_p(d), len(d), _p(e), len(e), _p(t), _p(c), _p(tm), len(t)),
            "wgcs_endpoint_set_accepted_host")


def set_finished_host(arena, pkts, gate, hs_slots, states, ep, tab, claim, timers) -> None:
    """wgcs_endpoint_set_finished_host: `tab`, `claim` and `timers` are written in place."""
    a, p, g = _in(arena, np.uint8), _in(pkts, AEAD_PKT_DTYPE), _in(gate, np.int32)
    hs, st, e = _in(hs_slots, SESSION_SLOT_DTYPE), _in(states, HS_STATE_DTYPE), _in(ep, ENDPOINT_DTYPE)
    t, c, tm = _tables(tab, claim, timers)
    if len(g) != len(p) or len(e) != len(p):
        raise ValueError("gate and ep hold one row per packet")
    _status(_lib.load().wgcs_endpoint_set_finished_host(_p(a), _p(p), _p(g), len(p), _p(hs), len(hs), _p(st), len(st),
                                                        _p(e), _p(t), _p(c), _p(tm), len(t)),
            "wgcs_endpoint_set_finished_host")


def _dst_out(n: int):
    return np.zeros(n, ENDPOINT_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.int32)


def _pair(tab, timers):
    t, tm = _host(tab, ENDPOINT_DTYPE, "table"), _host(timers, TIMERS_DTYPE, "timers")
    if len(tm) != len(t):
        raise ValueError("timers holds one row per table row")
    return t, tm


def dst_jobs_host(peer, count, status, job_key, max_segs: int, lens, nbufs, peer_rows, tab, timers):
    """wgcs_endpoint_dst_jobs_host: `nbufs` (int32), `tab` and `timers` are
    written in place; returns (dst, dst_v6, dst_status, tx_bytes)."""
    pe, co, st, jk = _in(peer, np.uint32), _in(count, np.int32), _in(status, np.int32), _in(job_key, np.uint32)
    ln, nb, pr = _in(lens, np.int32), _host(nbufs, np.int32, "nbufs"), _in(peer_rows, np.uint32)
    t, tm = _pair(tab, timers)
    n = len(jk)
    if len(co) != n or len(st) != n or len(nb) != n or len(pe) < n * max_segs or len(ln) < n * max_segs:
        raise ValueError("count, status and nbufs hold one row per job, peer and lens max_segs per job")
    dst, v6, ds = _dst_out(n)
    tx = np.zeros(n, np.uint64)
    _status(_lib.load().wgcs_endpoint_dst_jobs_host(_p(pe), _p(co), _p(st), _p(jk), n, max_segs, _p(ln), _p(nb), _p(pr),
                                                    len(pr), _p(t), _p(tm), len(t), _p(dst), _p(v6), _p(ds), _p(tx)),
            "wgcs_endpoint_dst_jobs_host")
    return dst, v6, ds, tx


def dst_initiated_host(start, status, tab, timers):
    """wgcs_endpoint_dst_initiated_host: `tab` and `timers` are written in place; returns (dst, dst_v6, dst_status)."""
    d, st = _in(start, HS_START_DTYPE), _in(status, np.int32)
    t, tm = _pair(tab, timers)
    if len(st) != len(d):
        raise ValueError("status holds one row per descriptor")
    dst, v6, ds = _dst_out(len(d))
    _status(_lib.load().wgcs_endpoint_dst_initiated_host(_p(d), _p(st), len(d), _p(t), _p(tm), len(t), _p(dst), _p(v6),
                                                         _p(ds)), "wgcs_endpoint_dst_initiated_host")
    return dst, v6, ds


def dst_responded_host(resp, status, tab, timers):
    """wgcs_endpoint_dst_responded_host: `tab` and `timers` are written in place; returns (dst, dst_v6, dst_status)."""
    d, st = _in(resp, HS_RESP_DTYPE), _in(status, np.int32)
    t, tm = _pair(tab, timers)
    if len(st) != len(d):
        raise ValueError("status holds one row per descriptor")
    dst, v6, ds = _dst_out(len(d))
    _status(_lib.load().wgcs_endpoint_dst_responded_host(_p(d), _p(st), len(d), _p(t), _p(tm), len(t), _p(dst), _p(v6),
                                                         _p(ds)), "wgcs_endpoint_dst_responded_host")
    return dst, v6, ds
