"""Host-side mirror of the staged queue (package `device`: peer.qus.staged,
send.go:331-426) over the C ABI.

Names and argument meaning follow the reference:
  stage_batch      StagePackets: the jobs the send gate refused or send_assign_batch dropped join their
                   peer's ring, behind send_assign_batch over the same job table    send.go:331-350, :402-407
  release_batch    SendStagedPackets: the rings of the peers whose current keypair can send become a job
                   table for send_assign_batch (max_segs == 1)                      send.go:363-426
  flush_batch      FlushStagedPackets over expire_batch's actions, or every row     send.go:352-361
  *_host           those three on host memory (numpy arrays), in row order
  state / entries  an empty queue; a peer's queue in order, for tests
  work_bytes(n)    the device scratch stage_batch (n jobs) and release_batch (n peer rows) need
The state is five arrays beside the other per-peer tables; `len` is what
timers.expire_batch takes as `staged`.  The row functions and the kernels live
in libwgcsum.so (wgcs_staged.h, staged_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import (ERR_BATCH_FULL, ERR_INVALID_ARG, ERR_KEY_EXPIRED, HS_NONE, PEER_NONE, STAGED_EVICTED, STAGED_NONE,
                   STAGED_RELEASED, TIMERS_ACT_FLUSH_STAGED)
from .cookie import _status
from .keypairs import KEYPAIRS_DTYPE
from .keystate import work_bytes
from .noise import PEER_KEY_DTYPE, _host
from .rekey import REKEY_DTYPE
from .transport import _rows
from .tun import _ptr

HEAD_ROOM, ROOM = 16, 48  # a packet sits at slot * stride + 16 and needs 16 + size + 32 <= stride
MAX_CAP = 1024

__all__ = ["State", "state", "entries", "work_bytes", "stage_batch", "release_batch", "flush_batch", "stage_host",
           "release_host", "flush_host", "STAGED_RELEASED", "STAGED_NONE", "STAGED_EVICTED", "ERR_BATCH_FULL",
           "ERR_KEY_EXPIRED", "ERR_INVALID_ARG", "HS_NONE", "PEER_NONE", "TIMERS_ACT_FLUSH_STAGED", "HEAD_ROOM", "ROOM",
           "MAX_CAP"]

_U4, _I4, _U8, _U1 = np.dtype("<u4"), np.dtype("<i4"), np.dtype("<u8"), np.dtype("u1")


@dataclass
class State:
    """The five arrays of one queue table (numpy arrays, or tensors on the device) and its shape."""
    len: object        # uint32 per peer row: packets staged; expire_batch's `staged`
    head: object       # uint32 per peer row: ring position of the oldest packet
    lost: object       # uint32 per peer row: packets evicted or flushed so far
    slot_size: object  # int32 per slot
    ring: object       # uint8, n_peers * cap * stride: slot s holds its packet at s * stride + 16
    n_peers: int
    cap: int
    stride: int

    def arrays(self):
        return self.len, self.head, self.lost, self.slot_size, self.ring


def state(n_peers: int, cap: int, stride: int, fill: int = 0) -> State:
    """The empty queue of n_peers rings of `cap` slots of `stride` bytes on the
    host: every word zero; the ring bytes `fill` (no call reads a byte it did
    not write)."""
    if not (1 <= cap <= MAX_CAP and cap & (cap - 1) == 0 and n_peers * cap <= 1 << 28 and stride >= 16 and stride % 16 == 0):
        raise ValueError("cap a power of two in [1, 1024], n_peers * cap <= 2^28, stride a multiple of 16")
    return State(np.zeros(n_peers, np.uint32), np.zeros(n_peers, np.uint32), np.zeros(n_peers, np.uint32),
                 np.zeros(n_peers * cap, np.int32), np.full(n_peers * cap * stride, fill, np.uint8), n_peers, cap, stride)


def _np(x) -> np.ndarray:
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def entries(st: State, row: int) -> list[bytes]:
    """The packets staged for peer row `row`, oldest first."""
    n, head = int(_np(st.len).view(np.uint32)[row]), int(_np(st.head).view(np.uint32)[row])
    sizes, ring = _np(st.slot_size).view(np.int32), _np(st.ring).view(np.uint8)
    out = []
    for i in range(n):
        s = row * st.cap + ((head + i) & (st.cap - 1))
        o = s * st.stride + HEAD_ROOM
        out.append(ring[o:o + int(sizes[s])].tobytes())
    return out


def _count(x, dtype, given):
    return (0 if x is None else _rows(x, dtype)) if given is None else given


def stage_batch(dev, arena, sizes, peer, count, status_in, status_out, job_key, max_segs: int, peer_rows, st: State,
                where, work, stream=None, n_jobs: int | None = None, n_ids: int | None = None,
                work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_staged_stage_batch behind send_assign_batch over its
    job table: `arena` with st.stride bytes a slot, `sizes` (int32 per slot),
    `peer` (uint32 per slot), `count` (int32 per job), `status_in` and
    `status_out` of send_gate_batch (two arrays), `job_key` of
    send_assign_batch.  Writes the state and `where` (uint32 per slot: the
    ring slot, STAGED_NONE or STAGED_EVICTED).  `work` is work_bytes(n_jobs) of
    16-byte-aligned scratch."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_staged_stage_batch(
        dev.h, _ptr(arena), st.stride, _ptr(sizes), _ptr(peer), _ptr(count), _ptr(status_in), _ptr(status_out),
        _ptr(job_key), _count(count, _I4, n_jobs), max_segs, _ptr(peer_rows), _count(peer_rows, _U4, n_ids), _ptr(st.len),
        _ptr(st.head), _ptr(st.lost), _ptr(st.slot_size), _ptr(st.ring), st.n_peers, st.cap, _ptr(where), _ptr(work),
        _count(work, _U1, work_bytes), s))


def release_batch(dev, now_ns: int, table, kp, send_nonce, limit: int, rekey, st: State, n_out_max: int, out, out_peer,
                  out_count, out_sizes, out_status, n_out, status, work, stream=None, n_keys: int | None = None,
                  work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_staged_release_batch: `table` the PEER_KEY_DTYPE rows,
    `kp`, `send_nonce` and `rekey` as send_gate_batch takes them.  Writes
    `status` (int32 per peer row: HS_NONE, STAGED_RELEASED, ERR_KEY_EXPIRED or
    ERR_BATCH_FULL), the job table `out` (st.stride bytes a job), `out_peer`,
    `out_count`, `out_sizes`, `out_status` (n_out_max rows each) and `n_out`
    (one uint32); the rings it released are empty afterwards.  `work` is
    work_bytes(st.n_peers) of 16-byte-aligned scratch."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_staged_release_batch(
        dev.h, now_ns, _ptr(table), _ptr(kp), _ptr(send_nonce), _count(send_nonce, _U8, n_keys), limit, _ptr(rekey),
        _ptr(st.len), _ptr(st.head), _ptr(st.slot_size), _ptr(st.ring), st.n_peers, st.cap, st.stride, n_out_max,
        _ptr(out), _ptr(out_peer), _ptr(out_count), _ptr(out_sizes), _ptr(out_status), _ptr(n_out), _ptr(status),
        _ptr(work), _count(work, _U1, work_bytes), s))


def flush_batch(dev, actions, st: State, stream=None) -> None:
    """Asynchronous wgcs_staged_flush_batch: `actions` is expire_batch's
    uint32 per peer row, or None to flush every row."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_staged_flush_batch(dev.h, _ptr(actions), _ptr(st.len), _ptr(st.head), _ptr(st.lost),
                                               st.n_peers, s))


def _in(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _p(a: np.ndarray):
    return a.ctypes.data if len(a) else None


def _state(st: State):
    a = (_host(st.len, np.uint32, "len"), _host(st.head, np.uint32, "head"), _host(st.lost, np.uint32, "lost"),
         _host(st.slot_size, np.int32, "slot_size"), _host(st.ring, np.uint8, "ring"))
    if not (len(a[0]) == len(a[1]) == len(a[2]) == st.n_peers and len(a[3]) == st.n_peers * st.cap and
            len(a[4]) == st.n_peers * st.cap * st.stride):
        raise ValueError("the state's arrays do not have its shape")
    return a


def stage_host(arena, sizes, peer, count, status_in, status_out, job_key, max_segs: int, peer_rows, st: State, where,
               work=None) -> None:
    """wgcs_staged_stage_host: stage_batch on numpy arrays.  The state and
    `where` (uint32) are written in place; `work` defaults to a fresh array."""
    c, si, so, jk = _in(count, np.int32), _in(status_in, np.int32), _in(status_out, np.int32), _in(job_key, np.uint32)
    z, pe, ar, pr = _in(sizes, np.int32), _in(peer, np.uint32), _in(arena, np.uint8), _in(peer_rows, np.uint32)
    w = _host(where, np.uint32, "where")
    n = len(c)
    if not (len(si) == len(so) == len(jk) == n and len(z) == len(pe) == n * max_segs and len(w) >= n * max_segs and
            len(ar) >= n * max_segs * st.stride):
        raise ValueError("count, status and job_key hold one row per job; sizes, peer, where and the arena max_segs slots")
    ln, hd, lo, ss, rg = _state(st)
    if work is None:
        work = np.zeros(2 * max(n, 1), np.uint64)
    wk = _host(work, np.uint8, "work")
    _status(_lib.load().wgcs_staged_stage_host(_p(ar), st.stride, _p(z), _p(pe), _p(c), _p(si), _p(so), _p(jk), n, max_segs,
                                               _p(pr), len(pr), _p(ln), _p(hd), _p(lo), _p(ss), _p(rg), st.n_peers, st.cap,
                                               _p(w), _p(wk), len(wk)), "wgcs_staged_stage_host")


def release_host(now_ns: int, table, kp, send_nonce, limit: int, rekey, st: State, n_out_max: int, out, out_peer,
                 out_count, out_sizes, out_status, n_out, status) -> None:
    """wgcs_staged_release_host: release_batch on numpy arrays.  `rekey`, the
    state and every output are written in place."""
    t, k, sn = _in(table, PEER_KEY_DTYPE), _in(kp, KEYPAIRS_DTYPE), _in(send_nonce, np.uint64)
    r = _host(rekey, REKEY_DTYPE, "rekey")
    o, op, oc = _host(out, np.uint8, "out"), _host(out_peer, np.uint32, "out_peer"), _host(out_count, np.int32, "out_count")
    oz, os_ = _host(out_sizes, np.int32, "out_sizes"), _host(out_status, np.int32, "out_status")
    no, stt = _host(n_out, np.uint32, "n_out"), _host(status, np.int32, "status")
    ln, hd, _, ss, rg = _state(st)
    if not (len(t) == len(k) == len(r) == st.n_peers and len(stt) >= st.n_peers and len(no) >= 1 and
            len(o) >= n_out_max * st.stride and min(len(op), len(oc), len(oz), len(os_)) >= n_out_max):
        raise ValueError("table, kp, rekey and status hold one row per peer row, the job table n_out_max rows")
    _status(_lib.load().wgcs_staged_release_host(now_ns, _p(t), _p(k), _p(sn), len(sn), C.c_uint64(limit), _p(r), _p(ln),
                                                 _p(hd), _p(ss), _p(rg), st.n_peers, st.cap, st.stride, n_out_max, _p(o),
                                                 _p(op), _p(oc), _p(oz), _p(os_), _p(no), _p(stt)),
            "wgcs_staged_release_host")


def flush_host(actions, st: State) -> None:
    """wgcs_staged_flush_host: flush_batch on numpy arrays."""
    a = None if actions is None else _in(actions, np.uint32)
    if a is not None and len(a) != st.n_peers:
        raise ValueError("actions holds one word per peer row")
    ln, hd, lo, _, _ = _state(st)
    _status(_lib.load().wgcs_staged_flush_host(None if a is None else _p(a), _p(ln), _p(hd), _p(lo), st.n_peers),
            "wgcs_staged_flush_host")
