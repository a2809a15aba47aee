"""Host-side mirror of the Write-call builder over the C ABI.

Names and argument meaning follow the reference:
  write_build_batch   the per-peer containers of RoutineReceiveIncoming and each
                      peer's Tun.Write and bookkeeping in RoutineSendToInternet,
                      device/receive.go:178-228, :398-504, on device arrays
  write_build_host    the same rule on numpy arrays (no device)
Per receive batch and peer the builder writes one GRO_CALL_DTYPE row, its
GRO_BUF_DTYPE rows and one WRITE_GROUP_DTYPE accounting row, in a fixed layout
of calls_per_batch rows per batch that handle_gro_batch consumes as it is.
The grouping lives in libwgcsum.so (write_kernels.hip, wgcs_write_plan.h);
nothing here computes.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ERR_BATCH_FULL, ERR_OUT_OF_RANGE, GROUP_DATA, PEER_NONE, WgcsError
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE, GRO_CAN_UDP, _ptr

# wgcs_write_group, 24 B
WRITE_GROUP_DTYPE = np.dtype([("peer", "<u4"), ("tail", "<i4"), ("flags", "<u4"), ("n_valid", "<u4"),
                              ("rx_bytes", "<u8")])

__all__ = ["WRITE_GROUP_DTYPE", "GROUP_DATA", "PEER_NONE", "ERR_BATCH_FULL", "ERR_OUT_OF_RANGE", "write_build_batch",
           "write_build_host"]


def write_build_batch(dev, pkts, verdict, n_msgs: int, key_peer, offset: int, cap: int, calls_per_batch: int, bufs,
                      calls, groups, n_groups, status, gro_flags: int = GRO_CAN_UDP, stream=None,
                      n_batches: int | None = None, n_keys: int | None = None) -> None:
    """Asynchronous wgcs_write_build_batch on what source_batch left: pkts
    (AEAD_PKT_DTYPE rows) and verdict (int32) of n_batches * n_msgs rows,
    key_peer (uint32 per key row).  Fills bufs (GRO_BUF_DTYPE, n_batches *
    n_msgs rows), calls (GRO_CALL_DTYPE) and groups (WRITE_GROUP_DTYPE) of
    n_batches * calls_per_batch rows each, and n_groups / status (int32 per
    batch).  pkts, bufs and calls are 16-byte aligned (a fresh torch tensor is)."""
    s = getattr(stream, "cuda_stream", stream)
    n_batches = _rows(pkts, AEAD_PKT_DTYPE) // n_msgs if n_batches is None else n_batches
    n_keys = _rows(key_peer, np.dtype("<u4")) if n_keys is None else n_keys
    dev._check(dev.lib.wgcs_write_build_batch(dev.h, _ptr(pkts), _ptr(verdict), n_msgs, n_batches, _ptr(key_peer), n_keys,
                                              offset, cap, gro_flags, calls_per_batch, _ptr(bufs), _ptr(calls),
                                              _ptr(groups), _ptr(n_groups), _ptr(status), s))


def write_build_host(pkts: np.ndarray, verdict: np.ndarray, n_msgs: int, key_peer: np.ndarray, offset: int, cap: int,
                     calls_per_batch: int, bufs: np.ndarray, calls: np.ndarray, groups: np.ndarray,
                     n_groups: np.ndarray, status: np.ndarray, gro_flags: int = GRO_CAN_UDP,
                     n_batches: int | None = None, n_keys: int | None = None) -> None:
    """wgcs_write_build_host: the same rule, array for array, on numpy arrays
    of the dtypes above (alignment as for the device form)."""
    for a, dt in ((pkts, AEAD_PKT_DTYPE), (verdict, np.dtype("<i4")), (key_peer, np.dtype("<u4")),
                  (bufs, GRO_BUF_DTYPE), (calls, GRO_CALL_DTYPE), (groups, WRITE_GROUP_DTYPE),
                  (n_groups, np.dtype("<i4")), (status, np.dtype("<i4"))):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
            raise TypeError(f"a contiguous numpy array of {dt}")
    n_batches = len(pkts) // n_msgs if n_batches is None else n_batches
    n_keys = len(key_peer) if n_keys is None else n_keys
    rc = _lib.load().wgcs_write_build_host(_ptr(pkts), _ptr(verdict), n_msgs, n_batches, _ptr(key_peer), n_keys, offset,
                                           cap, gro_flags, calls_per_batch, _ptr(bufs), _ptr(calls), _ptr(groups),
                                           _ptr(n_groups), _ptr(status))
    if rc != 0:
        raise WgcsError(rc, "wgcs_write_build_host")
