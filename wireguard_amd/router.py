"""Host-side mirror of the reference's peer lookup (package `device`) over the
C ABI -- SURVEY.md §8 row f5.

Names and argument meaning follow the reference's device/:
  Router.insert / remove / remove_by_peer / find / peer_prefixes
                                                  Router, device/router.go:405-495
  Router.image()                                  the flat image of both tries the kernels walk
  session_table(indices, keys, n_slots)           SessionMap.Get as an array, sessions.go:26-30
  classify_batch                                  RoutineReceiveFromPeers' loop body, receive.go:145-207
  source_batch                                    the allowed-source check, receive.go:438-482
  route_dst_batch                                 RoutineReadFromTUN's routing step, send.go:264-293
Peers are caller-chosen uint32 ids; PEER_NONE is Find's nil.  The trie, the
image walk and the three kernels live in libwgcsum.so (router.cpp,
wgcs_route_walk.h, route_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import ctypes as C
import ipaddress

import numpy as np

from . import _lib
from ._lib import ERR_SOURCE, PEER_NONE, WgcsError
from .transport import AEAD_PKT_DTYPE, _rows
from .tun import _ptr

SESSION_SLOT_DTYPE = np.dtype([("index", "<u4"), ("key", "<u4")])  # wgcs_session_slot
PREFIX_DTYPE = np.dtype([("addr", "u1", (16,)), ("addr_len", "u1"), ("cidr", "u1"), ("pad", "u1", (2,))])  # wgcs_prefix

__all__ = ["Router", "image_find", "session_table", "classify_batch", "source_batch", "route_dst_batch",
           "SESSION_SLOT_DTYPE", "PREFIX_DTYPE", "PEER_NONE", "ERR_SOURCE"]


def _addr(addr) -> bytes:
    """4 or 16 address bytes of bytes, an ipaddress object or a string."""
    if isinstance(addr, str):
        addr = ipaddress.ip_address(addr)
    if isinstance(addr, (ipaddress.IPv4Address, ipaddress.IPv6Address)):
        return addr.packed
    return bytes(addr)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise WgcsError(rc, f"{what}: {_lib.load().wgcs_strerror(rc).decode()}")


class Router:
    """device.Router with uint32 peer ids.  A prefix is (addr, cidr): addr as 4
    or 16 bytes, an ipaddress address or a string."""

    def __init__(self):
        self.lib = _lib.load()
        self.h = self.lib.wgcs_router_create()
        if not self.h:
            raise MemoryError("wgcs_router_create")

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.wgcs_router_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def insert(self, addr, cidr: int, peer: int) -> None:
        a = _addr(addr)
        if not 0 <= cidr <= 255:
            raise WgcsError(_lib.ERR_INVALID_ARG, f"cidr {cidr}")
        _check(self.lib.wgcs_router_insert(self.h, a, len(a), cidr, peer), "wgcs_router_insert")

    def remove(self, addr, cidr: int, peer: int) -> None:
        a = _addr(addr)
        if not 0 <= cidr <= 255:
            raise WgcsError(_lib.ERR_INVALID_ARG, f"cidr {cidr}")
        _check(self.lib.wgcs_router_remove(self.h, a, len(a), cidr, peer), "wgcs_router_remove")

    def remove_by_peer(self, peer: int) -> None:
        _check(self.lib.wgcs_router_remove_by_peer(self.h, peer), "wgcs_router_remove_by_peer")

    def find(self, addr) -> int:
        """The peer id, or PEER_NONE."""
        a = _addr(addr)
        if len(a) not in (4, 16):
            raise WgcsError(_lib.ERR_INVALID_ARG, "unknown address type")
        return self.lib.wgcs_router_find(self.h, a, len(a))

    def peer_prefixes(self, peer: int) -> list[tuple[bytes, int]]:
        """[(masked address bytes, cidr)] in the order of the reference's peer.nodes."""
        n = C.c_size_t(0)
        _check(self.lib.wgcs_router_peer_prefixes(self.h, peer, None, 0, C.byref(n)), "wgcs_router_peer_prefixes")
        out = np.zeros(n.value, PREFIX_DTYPE)
        _check(self.lib.wgcs_router_peer_prefixes(self.h, peer, out.ctypes.data, len(out), C.byref(n)),
               "wgcs_router_peer_prefixes")
        return [(p["addr"][:int(p["addr_len"])].tobytes(), int(p["cidr"])) for p in out[:n.value]]

    def image(self) -> np.ndarray:
        """The image as a uint8 array: copy it to 16-byte-aligned device memory
        (a fresh torch tensor is) for source_batch / route_dst_batch."""
        buf = np.zeros(self.lib.wgcs_router_image_size(self.h), dtype=np.uint8)
        n = C.c_size_t(0)
        _check(self.lib.wgcs_router_write_image(self.h, buf.ctypes.data, len(buf), C.byref(n)), "wgcs_router_write_image")
        return buf[:n.value]


def image_find(image, addr) -> int:
    """Router.find on an image in host memory (the walk the kernels run)."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    a = _addr(addr)
    peer = C.c_uint32(0)
    _check(_lib.load().wgcs_router_image_find(img.ctypes.data, len(img), a, len(a), C.byref(peer)),
           "wgcs_router_image_find")
    return peer.value


def session_table(indices, keys, n_slots: int | None = None) -> np.ndarray:
    """SESSION_SLOT_DTYPE rows for the sessions (receiver index -> key table
    row); n_slots defaults to the smallest power of two >= 2 * len(indices)."""
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    key = np.ascontiguousarray(keys, dtype=np.uint32)
    if idx.shape != key.shape or idx.ndim != 1:
        raise ValueError("indices and keys are 1-D and of one length")
    if n_slots is None:
        n_slots = 1
        while n_slots < 2 * len(idx):
            n_slots *= 2
    if not 0 <= n_slots < 2**32:
        raise WgcsError(_lib.ERR_INVALID_ARG, f"n_slots {n_slots}")
    slots = np.zeros(max(n_slots, 1), SESSION_SLOT_DTYPE)
    _check(_lib.load().wgcs_session_table_build(idx.ctypes.data, key.ctypes.data, len(idx), slots.ctypes.data, n_slots),
           "wgcs_session_table_build")
    return slots[:n_slots]


def classify_batch(dev, arena, sizes, slots, pkts, types, off=None, stride: int = 0, stream=None,
                   n: int | None = None, n_slots: int | None = None) -> None:
    """Asynchronous wgcs_recv_classify_batch: message q of sizes[q] (int32)
    bytes at off[q] (uint64), or at q * stride when off is None; slots are
    session_table rows on the device; pkts (AEAD_PKT_DTYPE rows) and types
    (int32) are written."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_slots = _rows(slots, SESSION_SLOT_DTYPE) if n_slots is None else n_slots
    dev._check(dev.lib.wgcs_recv_classify_batch(dev.h, _ptr(arena), _ptr(off), stride, _ptr(sizes), n, _ptr(slots),
                                                n_slots, _ptr(pkts), _ptr(types), s))


def source_batch(dev, arena, pkts, pkt_len, key_peer, image, verdict, peer=None, stream=None, n: int | None = None,
                 n_keys: int | None = None, image_bytes: int | None = None) -> None:
    """Asynchronous wgcs_recv_source_batch on what open_batch left: verdict[i]
    (int32, may be pkt_len itself) = the length, a passed-through pkt_len <= 0,
    ERR_SOURCE, ERR_PACKET_TOO_SHORT or ERR_INVALID_ARG; key_peer (uint32) maps
    a key table row to its peer id."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_keys = _rows(key_peer, np.dtype("<u4")) if n_keys is None else n_keys
    image_bytes = _rows(image, np.dtype("u1")) if image_bytes is None else image_bytes
    dev._check(dev.lib.wgcs_recv_source_batch(dev.h, _ptr(arena), _ptr(pkts), _ptr(pkt_len), _ptr(key_peer), n_keys, n,
                                              _ptr(image), image_bytes, _ptr(verdict), _ptr(peer), s))


def route_dst_batch(dev, arena, sizes, image, peer, off=None, stride: int = 0, offset: int = 0, stream=None,
                    n: int | None = None, image_bytes: int | None = None) -> None:
    """Asynchronous wgcs_route_dst_batch: peer[q] (uint32) = find(dst) of the
    packet of sizes[q] bytes at (off[q] or q * stride) + offset, or PEER_NONE."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(sizes, np.dtype("<i4")) if n is None else n
    image_bytes = _rows(image, np.dtype("u1")) if image_bytes is None else image_bytes
    dev._check(dev.lib.wgcs_route_dst_batch(dev.h, _ptr(arena), _ptr(off), stride, offset, _ptr(sizes), n, _ptr(image),
                                            image_bytes, _ptr(peer), s))
