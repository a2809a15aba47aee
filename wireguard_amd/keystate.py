"""Host-side mirror of the per-keypair state (replay filter, send nonce) over
the C ABI.

Names and argument meaning follow the reference:
  replay_validate / replay_reset   replay.Filter.Validate / Reset, replay/replay.go:32-76
  replay_batch                     keypair.replayFilter.Validate per message, device/receive.go:414-420
  send_assign_batch                keypair.sendNonce and its limit per packet, device/send.go:383-390
  work_bytes(n)                    the device workspace either batch needs for n rows (jobs)
The filters (REPLAY_FILTER_DTYPE rows) and the send nonces (uint64) sit in
device memory beside the AEAD key table and are indexed by its rows.  The key
order, the wave form of the filter and the nonce assignment live in
libwgcsum.so (keyorder.hip, replay_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import ERR_REPLAY, REJECT_AFTER_MESSAGES, WgcsError
from .router import SESSION_SLOT_DTYPE
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import _ptr

REPLAY_FILTER_DTYPE = np.dtype([("last", "<u8"), ("ring", "<u8", (128,))])  # wgcs_replay_filter, 1,032 B
NO_KEY = 0xFFFFFFFF

__all__ = ["REPLAY_FILTER_DTYPE", "REJECT_AFTER_MESSAGES", "ERR_REPLAY", "NO_KEY", "work_bytes", "replay_validate",
           "replay_reset", "replay_batch", "send_assign_batch"]


def work_bytes(n: int) -> int:
    """wgcs_keyorder_work_bytes: an upper bound for n rows, n <= 2^24."""
    if not 0 <= n <= 1 << 24:
        raise WgcsError(_lib.ERR_INVALID_ARG, f"n {n}")
    return _lib.load().wgcs_keyorder_work_bytes(n)


def _filter(f: np.ndarray) -> int:
    if not (isinstance(f, np.ndarray) and f.dtype == REPLAY_FILTER_DTYPE and f.size == 1 and f.flags.c_contiguous and
            f.flags.writeable):
        raise TypeError("one writable REPLAY_FILTER_DTYPE row")
    return f.ctypes.data


def replay_validate(f: np.ndarray, value: int, limit: int = REJECT_AFTER_MESSAGES) -> bool:
    """Filter.Validate on one REPLAY_FILTER_DTYPE row in host memory."""
    rc = _lib.load().wgcs_replay_validate(_filter(f), value, limit)
    if rc < 0:
        raise WgcsError(rc, "wgcs_replay_validate")
    return rc == 1


def replay_reset(f: np.ndarray) -> None:
    _lib.load().wgcs_replay_reset(_filter(f))


def replay_batch(dev, pkts, pkt_len, counter, filters, verdict, work, limit: int = REJECT_AFTER_MESSAGES, stream=None,
                 n: int | None = None, n_keys: int | None = None, work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_replay_batch on what open_batch left: verdict[i]
    (int32, may be pkt_len itself) = pkt_len[i], or ERR_REPLAY for a message
    open decrypted whose counter (uint64) filters[pkts[i].key] rejects; the
    filters are updated in place.  work is 16-byte-aligned device memory of at
    least work_bytes(n) bytes (a fresh torch tensor is aligned)."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_keys = _rows(filters, REPLAY_FILTER_DTYPE) if n_keys is None else n_keys
    work_bytes = _rows(work, np.dtype("u1")) if work_bytes is None else work_bytes
    dev._check(dev.lib.wgcs_replay_batch(dev.h, _ptr(pkts), _ptr(pkt_len), _ptr(counter), n, _ptr(filters), n_keys,
                                         limit, _ptr(verdict), _ptr(work), work_bytes, s))


def send_assign_batch(dev, sizes, peer, count, status, max_segs: int, stride: int, peer_keys, send_nonce, pkts, nbufs,
                      job_key, work, limit: int = REJECT_AFTER_MESSAGES, stream=None, n_jobs: int | None = None,
                      n_slots: int | None = None, n_keys: int | None = None, work_bytes: int | None = None) -> None:
    """Asynchronous wgcs_send_assign_batch between route_dst_batch and
    seal_batch: from gso_split_batch's sizes / count / status and the slots'
    peer ids, the seal descriptors of every slot (pkts, AEAD_PKT_DTYPE rows,
    n_jobs * max_segs of them), nbufs (int32) and job_key (uint32) per job;
    send_nonce (uint64 per key row) advances.  peer_keys are session_table
    rows that map a peer id to its key row."""
    s = getattr(stream, "cuda_stream", stream)
    n_jobs = _rows(count, np.dtype("<i4")) if n_jobs is None else n_jobs
    n_slots = _rows(peer_keys, SESSION_SLOT_DTYPE) if n_slots is None else n_slots
    n_keys = _rows(send_nonce, np.dtype("<u8")) if n_keys is None else n_keys
    work_bytes = _rows(work, np.dtype("u1")) if work_bytes is None else work_bytes
    dev._check(dev.lib.wgcs_send_assign_batch(dev.h, _ptr(sizes), _ptr(peer), _ptr(count), _ptr(status), n_jobs,
                                              max_segs, stride, _ptr(peer_keys), n_slots, _ptr(send_nonce), n_keys,
                                              limit, _ptr(pkts), _ptr(nbufs), _ptr(job_key), _ptr(work), work_bytes, s))
