"""Host-side mirror of the rate limiter (package `ratelimiter`, and
device/receive.go:283-286 where RoutineHandshake consults it) over the C ABI.

Names and argument meaning follow the reference:
  allow            RateLimiter.Allow on a table in host memory          ratelimiter.go:91-126
  allow_batch      Allow over the screened rows of a receive batch, between
                   cookie.screen_batch (under load) and noise.consume_batch   receive.go:283-286
  cleanup_batch    cleanup() as a rebuild into a second table           ratelimiter.go:77-89
  allow_host, cleanup_host   those two on host memory (numpy arrays), rows and slots in order
A table is n_slots RL_ENTRY_DTYPE rows, n_slots a power of two, all zero when
new: open addressing from home_slot(src, n_slots).  Where an entry lands among
the slots of its probe depends, on the device, on which row claimed first, so
tables are compared through entries().  The clock is the caller's: one int64 of
nanoseconds per call.  When to call cleanup (once a second while the last live
count or entries_created was not zero) and IsUnderLoad stay with the caller.
The row functions and the kernels live in libwgcsum.so (wgcs_ratelimit.h,
ratelimit_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import (ERR_RATE_LIMITED, ERR_RATE_TABLE_FULL, HS_PASS, RL_CLEANUP_NS, RL_MAX_TOKENS_NS,
                   RL_PACKET_COST_NS)
from .cookie import SRC_ADDR_DTYPE, _status
from .keystate import work_bytes
from .noise import _host
from .transport import _rows
from .tun import _ptr

RL_ENTRY_DTYPE = np.dtype([("ip", "u1", (16,)), ("state", "<u4"), ("family", "<u4"), ("tokens", "<i8"),
                           ("last_ns", "<i8")])  # wgcs_rl_entry
assert RL_ENTRY_DTYPE.itemsize == 40

__all__ = ["RL_ENTRY_DTYPE", "RL_PACKET_COST_NS", "RL_MAX_TOKENS_NS", "RL_CLEANUP_NS", "ERR_RATE_LIMITED",
           "ERR_RATE_TABLE_FULL", "HS_PASS", "table", "home_slot", "allow", "allow_batch", "cleanup_batch",
           "allow_host", "cleanup_host", "work_bytes", "entries"]

_I4, _U1 = np.dtype("<i4"), np.dtype("u1")


def table(n_slots: int) -> np.ndarray:
    """An empty table: n_slots (a power of two, at most 2^24) zeroed RL_ENTRY_DTYPE rows."""
    if n_slots < 1 or n_slots & (n_slots - 1) or n_slots > 1 << 24:
        raise ValueError("n_slots is a power of two in [1, 2^24]")
    return np.zeros(n_slots, RL_ENTRY_DTYPE)


def _src(src) -> np.ndarray:
    return np.ascontiguousarray(src, dtype=SRC_ADDR_DTYPE).reshape(-1)


def home_slot(src, n_slots: int) -> int:
    """wgcs_ratelimit_home_slot: the slot the probe of one SRC_ADDR_DTYPE row's address starts at."""
    s = _src(src)
    if len(s) != 1 or s["len"][0] not in (6, 18):
        raise ValueError("one SRC_ADDR_DTYPE row of len 6 or 18")
    table(n_slots)
    return _lib.load().wgcs_ratelimit_home_slot(s.ctypes.data, n_slots)


def allow(tab, src, now_ns: int) -> bool:
    """wgcs_ratelimit_allow: one Allow of one SRC_ADDR_DTYPE row on the table
    `tab` (numpy, written in place).  Raises WgcsError(ERR_RATE_TABLE_FULL) for
    a new address when no slot is free."""
    t, s = _host(tab, RL_ENTRY_DTYPE, "tab"), _src(src)
    if len(s) != 1:
        raise ValueError("one SRC_ADDR_DTYPE row")
    return bool(_status(_lib.load().wgcs_ratelimit_allow(t.ctypes.data, len(t), s.ctypes.data, now_ns),
                        "wgcs_ratelimit_allow"))


def allow_batch(dev, gate, src, tab, now_ns: int, verdict, work, stats=None, stream=None, n: int | None = None,
                n_slots: int | None = None, work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_ratelimit_batch: `gate` (int32 per row, the screen's
    verdict) and `src` (SRC_ADDR_DTYPE rows) are read, `tab` (RL_ENTRY_DTYPE
    rows) is updated and `verdict` (int32 per row; may be `gate`) receives the
    gate of a row that is not HS_PASS, else HS_PASS, ERR_RATE_LIMITED,
    ERR_RATE_TABLE_FULL or ERR_INVALID_ARG.  `stats` (4 uint32, optional) gets
    {passed, limited, table_full, entries_created}; `work` is work_bytes(n) of
    16-byte-aligned scratch.  Everything is on the device."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_ratelimit_batch(
        dev.h, _ptr(gate), _ptr(src), _rows(gate, _I4) if n is None else n, _ptr(tab),
        _rows(tab, RL_ENTRY_DTYPE) if n_slots is None else n_slots, now_ns, _ptr(verdict), _ptr(stats), _ptr(work),
        _rows(work, _U1) if work_bytes is None else work_bytes, s))


def cleanup_batch(dev, old, new, now_ns: int, live, stream=None, n_slots: int | None = None) -> None:
    """Asynchronous wgcs_ratelimit_cleanup_batch: `new` (as large as `old`, not
    overlapping it) is zeroed and receives every live entry of `old` that was
    used within the last second; `live` (one uint32) the number kept.  The
    caller then uses `new` as the table."""
    s = getattr(stream, "cuda_stream", stream)
    dev._check(dev.lib.wgcs_ratelimit_cleanup_batch(
        dev.h, _ptr(old), _ptr(new), _rows(old, RL_ENTRY_DTYPE) if n_slots is None else n_slots, now_ns, _ptr(live), s))


def allow_host(gate, src, tab, now_ns: int, verdict=None, stats=None) -> np.ndarray:
    """wgcs_ratelimit_batch_host: allow_batch on numpy arrays, rows in order.
    `tab` is written in place, and `verdict` (default: a new int32 array) and
    `stats` (4 uint32, optional) when given; returns the verdicts."""
    g, s, t = np.ascontiguousarray(gate, dtype=np.int32).reshape(-1), _src(src), _host(tab, RL_ENTRY_DTYPE, "tab")
    v = np.empty(len(g), np.int32) if verdict is None else _host(verdict, np.int32, "verdict")
    st = None if stats is None else _host(stats, np.uint32, "stats")
    if len(s) != len(g) or len(v) != len(g) or (st is not None and len(st) != 4):
        raise ValueError("gate, src and verdict hold one row per message, stats four words")
    _status(_lib.load().wgcs_ratelimit_batch_host(g.ctypes.data if len(g) else None, s.ctypes.data if len(g) else None,
                                                  len(g), t.ctypes.data, len(t), now_ns,
                                                  v.ctypes.data if len(g) else None,
                                                  None if st is None else st.ctypes.data), "wgcs_ratelimit_batch_host")
    return v


def cleanup_host(old, now_ns: int) -> tuple[np.ndarray, int]:
    """wgcs_ratelimit_cleanup_host: (the rebuilt table, the entries kept)."""
    o = np.ascontiguousarray(old, dtype=RL_ENTRY_DTYPE).reshape(-1)
    new, live = np.zeros(len(o), RL_ENTRY_DTYPE), np.zeros(1, np.uint32)
    _status(_lib.load().wgcs_ratelimit_cleanup_host(o.ctypes.data, new.ctypes.data, len(o), now_ns, live.ctypes.data),
            "wgcs_ratelimit_cleanup_host")
    return new, int(live[0])


def entries(tab) -> dict:
    """{(family, the 16 key bytes): (tokens, last_ns)} of the live rows of a
    table given as RL_ENTRY_DTYPE rows (numpy) or their bytes (a uint8 tensor
    or array).  Raises if a key is held twice."""
    if hasattr(tab, "cpu"):
        tab = tab.cpu().numpy()
    t = np.ascontiguousarray(tab).reshape(-1).view(np.uint8).view(RL_ENTRY_DTYPE)
    out = {}
    for e in t[t["state"] == 1]:
        key = (int(e["family"]), e["ip"].tobytes())
        if key in out:
            raise ValueError(f"address {key} is in the table twice")
        out[key] = (int(e["tokens"]), int(e["last_ns"]))
    return out
