"""Literal Python restatement of the reference's endpoint code, message by
message (test oracle, CPU only):

  parse_one_socket_control_message   unix.ParseOneSocketControlMessage (sockcmsg_unix.go)
  get_src_from_control               conn/sticky.go:46-94
  receive_endpoints                  the tail of ReceiveIPvX, conn/bind.go:308-319
  Peer                               peer.endpoint with SetEndpointFromPacket, markEndpointSrcForClearing
                                     and the part of Send in front of bind.Send (device/peer.go:195-221, :281-297)

An endpoint is (dst bytes, src bytes): dst is AddrPort.MarshalBinary() -- the
4 or 16 address bytes, then the port as LE16 -- and src NetEndpoint.src."""
import struct

SIZEOF_CMSGHDR = 16
IPPROTO_IP, IP_PKTINFO = 0, 8
IPPROTO_IPV6, IPV6_PKTINFO = 41, 50
SOL_UDP, UDP_GRO = 17, 104
ERR_NO_ENDPOINT = -30


def cmsg_align(n: int) -> int:
    return (n + 7) & ~7


def cmsg_space(datalen: int) -> int:
    return cmsg_align(SIZEOF_CMSGHDR) + cmsg_align(datalen)


def cmsg(level: int, typ: int, data: bytes, length: int | None = None) -> bytes:
    """One control message as the kernel writes it: header, data, padding to 8; `length` overrides Cmsghdr.Len."""
    ln = SIZEOF_CMSGHDR + len(data) if length is None else length
    body = struct.pack("<Qii", ln, level, typ) + data
    return body + bytes(cmsg_align(len(body)) - len(body))


def parse_one_socket_control_message(b: bytes):
    """(hdr bytes, (len, level, type), data, remainder) or None for EINVAL."""
    ln, level, typ = struct.unpack("<Qii", b[:SIZEOF_CMSGHDR].ljust(SIZEOF_CMSGHDR, b"\0"))
    if ln < SIZEOF_CMSGHDR or ln > len(b):
        return None
    i = cmsg_align(ln)
    return b[:SIZEOF_CMSGHDR], (ln, level, typ), b[SIZEOF_CMSGHDR:ln], (b[i:] if i < len(b) else b"")


def get_src_from_control(control: bytes) -> bytes:
    src = b""  # endpoint.ClearSrc()
    remaining = control
    while len(remaining) > SIZEOF_CMSGHDR:
        parsed = parse_one_socket_control_message(remaining)
        if parsed is None:
            return src
        hdr, (_, level, typ), data, remaining = parsed
        for lv, ty, payload in ((IPPROTO_IP, IP_PKTINFO, 12), (IPPROTO_IPV6, IPV6_PKTINFO, 20)):
            if level == lv and typ == ty:
                out = bytearray(cmsg_space(payload))  # a fresh zeroed buffer
                out[:SIZEOF_CMSGHDR] = hdr            # copy(endpoint.src, hdrSlice)
                room = len(out) - SIZEOF_CMSGHDR      # copy(endpoint.src[unix.CmsgLen(0):], data)
                out[SIZEOF_CMSGHDR:SIZEOF_CMSGHDR + min(room, len(data))] = data[:room]
                return bytes(out)
    return src


def receive_endpoints(addrs, sizes, controls):
    """bind.go:308-319 over one batch after splitMessages: addrs[i] is msgs[i].Addr
    (dst bytes), sizes[i] msgs[i].N, controls[i] msgs[i].OOB[:msgs[i].NN].  None
    for a slot of size 0."""
    return [None if sizes[i] == 0 else (addrs[i], get_src_from_control(controls[i])) for i in range(len(sizes))]


class Peer:
    """peer.endpoint: val is None or (dst, src)."""

    def __init__(self):
        self.val, self.clear_src_on_tx = None, False
        self.tx_bytes = 0

    def set_endpoint_from_packet(self, endpoint):  # peer.go:281-286
        self.val = endpoint
        self.clear_src_on_tx = False

    def mark_endpoint_src_for_clearing(self):  # :290-297
        if self.val is None:
            return
        self.clear_src_on_tx = True

    def send(self, bufs):
        """Peer.Send up to bind.Send: the endpoint bind.Send gets, or ERR_NO_ENDPOINT; the caller
        adds tx_bytes once its send succeeded (:212-219)."""
        if self.val is None:
            return ERR_NO_ENDPOINT
        if self.clear_src_on_tx:
            self.val = (self.val[0], b"")  # ClearSrc
            self.clear_src_on_tx = False
        return self.val

    def sent(self, bufs):
        self.tx_bytes += sum(len(b) for b in bufs)


def is6(dst: bytes) -> bool:
    """endpoint.DstIP().Is6(): every 16-byte address, v4-mapped included (conn/bind.go:405)."""
    return len(dst) == 18
