"""Host-side mirror of the reference's transport-message AEAD (package
`device`) over the C ABI -- SURVEY.md §8 row f4.

Names, argument meaning and error behaviour follow the reference's device/:
  padding(packet_size, mtu)                       device/send.go:529-560
  seal(dev, key, remote_index, counter, packet, mtu)
                                                  RoutineEncryption, send.go:438-463
  open_(dev, key, msg)                            RoutineDecryption, receive.go:363-383,
                                                  and the length trim of :432-482
  seal_batch / open_batch                         the same for device-resident batches
A transport message is LE32 type 4 | LE32 receiver index | LE64 counter |
ciphertext | 16-byte tag; the nonce is 4 zero bytes | LE64 counter and there is
no additional data.  Every byte is sealed or opened by the gfx950 kernel of
libwgcsum.so (aead_kernels.hip); nothing here computes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ERR_AUTH, ERR_PACKET_TOO_SHORT, WgcsError
from .tun import _ptr

MESSAGE_TRANSPORT_TYPE = 4  # device/noise-protocol.go
MESSAGE_TRANSPORT_HEADER_SIZE = 16  # device/noise-protocol.go: type | receiver | counter
POLY1305_TAG_SIZE = 16  # chacha20poly1305.Overhead
MIN_MESSAGE_SIZE = MESSAGE_TRANSPORT_HEADER_SIZE + POLY1305_TAG_SIZE  # a keepalive
PADDING_MULTIPLE = 16  # device/send.go

AEAD_KEY_DTYPE = np.dtype([("key", "u1", (32,)), ("remote_index", "<u4"), ("pad", "<u4", (3,))])  # wgcs_aead_key
AEAD_PKT_DTYPE = np.dtype([("off", "<u8"), ("counter", "<u8"), ("len", "<u4"), ("key", "<u4")])  # wgcs_aead_pkt

__all__ = ["padding", "seal", "open_", "seal_batch", "open_batch", "AEAD_KEY_DTYPE", "AEAD_PKT_DTYPE",
           "MESSAGE_TRANSPORT_HEADER_SIZE", "POLY1305_TAG_SIZE", "MIN_MESSAGE_SIZE", "PADDING_MULTIPLE",
           "ERR_AUTH", "ERR_PACKET_TOO_SHORT"]


def padding(packet_size: int, mtu: int) -> int:
    """padding(packetSize, mtu int) int."""
    return _lib.load().wgcs_padding(packet_size, mtu)


def _key(key) -> np.ndarray:
    k = np.frombuffer(bytes(key), dtype=np.uint8)
    if len(k) != 32:
        raise ValueError("a ChaCha20-Poly1305 key has 32 bytes")
    return k


def seal(dev, key, remote_index: int, counter: int, packet, mtu: int) -> bytes:
    """The transport message RoutineEncryption makes of `packet`: header,
    padding(len(packet), mtu) zero bytes appended, sealed under (key, counter)."""
    n = len(packet)
    buf = np.zeros(MIN_MESSAGE_SIZE + n + PADDING_MULTIPLE, dtype=np.uint8)
    buf[MESSAGE_TRANSPORT_HEADER_SIZE:MESSAGE_TRANSPORT_HEADER_SIZE + n] = np.frombuffer(bytes(packet), dtype=np.uint8)
    k = _key(key)
    out_len = C.c_size_t(0)
    dev._check(dev.lib.wgcs_aead_seal(dev.h, k.ctypes.data, remote_index, counter, buf.ctypes.data, n, len(buf), mtu,
                                      C.byref(out_len)))
    return buf[:out_len.value].tobytes()


def open_(dev, key, msg) -> tuple[int, bytes | None, WgcsError | None]:
    """(counter, packet, err) of one transport message.  err is None and packet
    the decrypted packet cut to its IP length (b"" for a keepalive); or err is
    ERR_AUTH and packet None (chacha20poly1305.Open failed: the reference drops
    the element); or err is ERR_PACKET_TOO_SHORT and packet the whole decrypted
    content (RoutineSendToInternet skips it)."""
    m = np.frombuffer(bytes(msg), dtype=np.uint8).copy()
    k = _key(key)
    counter = C.c_uint64(0)
    pkt_len = C.c_int(0)
    rc = dev.lib.wgcs_aead_open(dev.h, k.ctypes.data, m.ctypes.data, len(m), C.byref(counter), C.byref(pkt_len))
    if rc == ERR_AUTH:
        return counter.value, None, dev._err(rc)
    content = m[MESSAGE_TRANSPORT_HEADER_SIZE:len(m) - POLY1305_TAG_SIZE]
    if rc == ERR_PACKET_TOO_SHORT:
        return counter.value, content.tobytes(), dev._err(rc)
    dev._check(rc)
    return counter.value, content[:pkt_len.value].tobytes(), None


def seal_batch(dev, arena, pkts, keys, mtu: int, out_len, stream=None, n: int | None = None,
               n_keys: int | None = None) -> None:
    """Asynchronous device-resident batch (wgcs_aead_seal_batch): `pkts`
    (AEAD_PKT_DTYPE rows), `keys` (AEAD_KEY_DTYPE rows) and `out_len` (int32)
    are device tensors / pointers; n and n_keys default to their lengths."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_keys = _rows(keys, AEAD_KEY_DTYPE) if n_keys is None else n_keys
    dev._check(dev.lib.wgcs_aead_seal_batch(dev.h, _ptr(arena), _ptr(pkts), _ptr(keys), n_keys, n, mtu, _ptr(out_len),
                                            s))


def open_batch(dev, arena, pkts, keys, pkt_len, counter, stream=None, n: int | None = None,
               n_keys: int | None = None) -> None:
    """Asynchronous device-resident batch (wgcs_aead_open_batch): per message
    pkt_len[i] (int32: trimmed length, 0 keepalive, or ERR_*) and counter[i]
    (uint64, for the caller's replay filter)."""
    s = getattr(stream, "cuda_stream", stream)
    n = _rows(pkts, AEAD_PKT_DTYPE) if n is None else n
    n_keys = _rows(keys, AEAD_KEY_DTYPE) if n_keys is None else n_keys
    dev._check(dev.lib.wgcs_aead_open_batch(dev.h, _ptr(arena), _ptr(pkts), _ptr(keys), n_keys, n, _ptr(pkt_len),
                                            _ptr(counter), s))


def _rows(x, dtype: np.dtype) -> int:
    """Rows of a descriptor table given as a uint8 tensor / array of its bytes
    or as a structured numpy array."""
    if isinstance(x, np.ndarray) and x.dtype == dtype:
        return len(x)
    if hasattr(x, "numel"):
        nbytes = x.numel() * x.element_size()
    elif isinstance(x, np.ndarray):
        nbytes = x.nbytes
    else:
        raise TypeError("give n / n_keys explicitly for a raw pointer")
    if nbytes % dtype.itemsize:
        raise ValueError(f"{nbytes} bytes is not a whole number of {dtype.itemsize}-byte rows")
    return nbytes // dtype.itemsize
