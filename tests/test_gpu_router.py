"""The device-resident peer lookup on the GPU (wgcs_recv_classify_batch,
wgcs_recv_source_batch, wgcs_route_dst_batch; route_kernels.hip) against the
references of tests/router_ref.py and, for the AEAD in between, aead_ref.py.

All comparisons are exact.  The kernels write nothing to the arena: every arena
is filled with a sentinel around its packets and compared whole afterwards.
Packets sit at odd byte offsets (the strided forms, with an odd stride, at
odd and even ones).  Only valid images go to the device."""
import ipaddress
import struct

import numpy as np
import pytest
import torch

import aead_ref
import router_ref
from router_ref import ERR_INVALID_ARG, ERR_OUT_OF_RANGE, ERR_PACKET_TOO_SHORT, ERR_SOURCE, NO_KEY
from wireguard_amd import _lib, router, transport
from wireguard_amd.router import PEER_NONE, SESSION_SLOT_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
HDR = 16  # MessageTransportHeaderSize: the offset of wgcs_gso_split_batch's packets and of a message's content


def V4(s):
    return ipaddress.IPv4Address(s).packed


def V6(s):
    return ipaddress.IPv6Address(s).packed


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def i32(n, fill=12345):
    return torch.full((max(n, 1),), fill, dtype=torch.int32, device="cuda")


def u32_out(n):
    return torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")


def as_u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n]


def none_to(peer):
    return PEER_NONE if peer is None else peer


class Table:
    """A C router, the restatement fed the same prefixes, and the image on the device."""

    def __init__(self, prefixes):
        self.c, self.ref = router.Router(), router_ref.RefRouter()
        self.prefixes = prefixes
        for addr, cidr, peer in prefixes:
            self.c.insert(addr, cidr, peer)
            self.ref.insert(addr, cidr, peer)
        self.image = self.c.image()
        self.d_image = up(self.image)
        assert self.d_image.data_ptr() % 16 == 0


def big_prefixes():
    """About 40 assorted prefixes, /0, /32 and /128 among them, plus a v4 chain
    /1../32 (a walk 32 deep) and a v6 chain /1../128 under the v6 /0: 129 nodes
    on one path, which reaches the walk's visit bound from the valid side.
    IPv4 has no /0 here, so that there are unrouted addresses."""
    rng = np.random.default_rng(405)
    p = [(V6("::"), 0, 1), (V4("10.0.0.1"), 32, 2), (V4("255.255.255.255"), 32, 3), (V6("2001:db8::1"), 128, 4),
         (V6("fd00::"), 8, 5), (V6("fd00:1::"), 32, 6), (V6("fd00:1:0:0:8000::"), 65, 7), (V6("fd00:1::ffff"), 128, 8)]
    for k in range(16):
        p.append((bytes([172, 16 + k, int(rng.integers(256)), 0]), int(rng.choice([12, 16, 20, 24, 30])), 10 + k))
    for k in range(16):
        p.append((V6("2001:db8::")[:6] + rng.bytes(10), int(rng.choice([48, 56, 64, 80, 112, 127])), 30 + k))
    chain4, chain6 = V4("203.0.113.77"), V6("2a00:1450:4001:82b:dead:beef:0:200e")
    p += [(chain4, c, 100 + c) for c in range(1, 33)]
    p += [(chain6, c, 200 + c) for c in range(1, 129)]
    return p


SMALL = [(V4("10.0.0.0"), 8, 1), (V4("10.1.0.0"), 16, 2), (V4("192.168.7.0"), 24, 3), (V6("fd00::"), 16, 4),
         (V6("fd00:0:0:1::"), 64, 5), (V6("2001:db8::"), 32, 1)]


@pytest.fixture(scope="module")
def big():
    return Table(big_prefixes())


@pytest.fixture(scope="module")
def small():
    """No /0 on either side: unrouted addresses in both families."""
    return Table(SMALL)


def edge_addresses(table):
    out = set()
    for addr, cidr, _ in table.prefixes:
        bits = 8 * len(addr)
        first = int.from_bytes(router_ref.mask_addr(addr, cidr), "big")
        last = first | ((1 << (bits - cidr)) - 1)
        for x in (first, last):
            for d in (-1, 0, 1):
                out.add(((x + d) % (1 << bits)).to_bytes(len(addr), "big"))
    out.update((bytes(4), b"\xff" * 4, bytes(16), b"\xff" * 16, V4("8.8.8.8"), V4("10.0.0.0"), V4("172.15.0.1"),
                V4("172.32.0.1"), V4("192.0.2.1"), V4("1.1.1.1"), V4("100.64.0.1"), V4("127.0.0.1"), V4("64.0.0.0"),
                V4("9.255.255.255"), V4("11.0.0.0"), V6("::1"), V6("8000::"), V6("fe80::1")))
    return sorted(out)


def ip_packet(version_byte, size, src=None, dst=None):
    """`size` bytes that start like an IP header; addresses where they fit."""
    b = bytearray((0x11 + 3 * i) & 0xFF for i in range(size))
    if size:
        b[0] = version_byte
    v6 = (version_byte >> 4) == 6
    for a, at in ((src, 8 if v6 else 12), (dst, 24 if v6 else 16)):
        if a is not None and at + len(a) <= size:
            b[at:at + len(a)] = a
    return bytes(b)


def lay_out(packets, gap=HDR, pitch=None):
    """Slot q at an odd offset; its packet `gap` bytes in.  Returns (arena, offsets)."""
    offs, cur = [], 3
    for p in packets:
        offs.append(cur)
        cur += pitch if pitch else (gap + len(p) + 3) & ~1  # even steps keep every offset odd
        assert pitch is None or gap + len(p) <= pitch
    arena = np.full(cur + 64, SENTINEL, np.uint8)
    for o, p in zip(offs, packets):
        arena[o + gap:o + gap + len(p)] = np.frombuffer(p, np.uint8)
    return arena, offs


def test_find_parity_dst_and_source(dev, big):
    addrs = edge_addresses(big)
    assert 500 <= len(addrs) <= 900
    want = [none_to(big.ref.find(a)) for a in addrs]
    assert PEER_NONE in want and 100 + 32 in want and 200 + 128 in want  # unrouted, and both chain ends
    assert all(router.image_find(big.image, a) == w for a, w in zip(addrs, want))
    n = len(addrs)
    # the address is the destination and the source of its packet
    packets = [ip_packet(0x45 if len(a) == 4 else 0x60, 20 if len(a) == 4 else 40, src=a, dst=a) for a in addrs]
    arena, offs = lay_out(packets)
    d_arena = up(arena)
    sizes = np.array([len(p) for p in packets], np.int32)
    d_peer = u32_out(n)
    router.route_dst_batch(dev, d_arena, up(sizes), big.d_image, d_peer, off=up(np.array(offs, np.uint64)), offset=HDR, n=n)
    dev.sync()
    assert as_u32(d_peer, n).tolist() == want
    # source: the key of row i belongs to the found peer on even rows, to another peer on odd ones
    peers = sorted(set(want) - {PEER_NONE})
    key_peer = np.array(peers + [0x7FFFFFFF], np.uint32)
    pk = np.zeros(n, AEAD_PKT_DTYPE)
    pk["off"], pk["len"] = offs, sizes + 32
    for i, w in enumerate(want):
        pk["key"][i] = peers.index(w) if (w != PEER_NONE and i % 2 == 0) else len(peers)
    d_verdict, d_found = i32(n), u32_out(n)
    router.source_batch(dev, d_arena, up(pk), up(sizes), up(key_peer), big.d_image, d_verdict, peer=d_found, n=n)
    dev.sync()
    assert as_u32(d_found, n).tolist() == want
    ref = [router_ref.source_verdict(big.ref, p, len(p), int(k), key_peer.tolist())[0] for p, k in zip(packets, pk["key"])]
    assert d_verdict.cpu().numpy()[:n].tolist() == ref
    assert ERR_SOURCE in ref and 20 in ref and 40 in ref
    assert np.array_equal(d_arena.cpu().numpy(), arena)


@pytest.mark.parametrize("strided", [False, True])
def test_dst_sizes_and_versions(dev, small, strided):
    packets, sizes = [], []
    for nibble in (0, 4, 5, 6, 15):
        for size in (0, 1, 19, 20, 39, 40):
            # 40 bytes are laid down whatever `size` says, with a routed destination where each version keeps it
            dst = V6("fd00:0:0:1::9") if nibble == 6 else V4("10.1.2.3")
            packets.append(ip_packet((nibble << 4) | 5, 40, dst=dst))
            sizes.append(size)
    n = len(packets)
    arena, offs = lay_out(packets, pitch=57)
    want = [none_to(router_ref.route_dst(small.ref, p, s)) for p, s in zip(packets, sizes)]
    assert sorted(set(want)) == [2, 5, PEER_NONE] and want.count(2) == 3 and want.count(5) == 1
    d_arena, d_peer = up(arena), u32_out(n)
    if strided:
        assert offs == [3 + 57 * q for q in range(n)]
        router.route_dst_batch(dev, d_arena[3:], up(np.array(sizes, np.int32)), small.d_image, d_peer, stride=57,
                               offset=HDR, n=n)
    else:
        router.route_dst_batch(dev, d_arena, up(np.array(sizes, np.int32)), small.d_image, d_peer,
                               off=up(np.array(offs, np.uint64)), offset=HDR, n=n)
    dev.sync()
    assert as_u32(d_peer, n).tolist() == want
    assert np.array_equal(d_arena.cpu().numpy(), arena)
    router.route_dst_batch(dev, d_arena, up(np.array(sizes, np.int32)), small.d_image, d_peer, n=0)  # a no-op


def test_dst_unrouted_and_argument_checks(dev, small):
    addrs = [V4("10.1.0.1"), V4("10.2.0.1"), V4("11.0.0.1"), V4("192.168.8.1"), V6("fd00:0:0:1::1"), V6("fd00:0:0:2::1"),
             V6("fd01::1"), V6("2001:db8:ffff::1"), V6("2001:db9::1")]
    packets = [ip_packet(0x45 if len(a) == 4 else 0x6F, 61, dst=a) for a in addrs]
    arena, offs = lay_out(packets, gap=0)
    d_arena, d_peer = up(arena), u32_out(len(addrs))
    d_sizes, d_off = up(np.full(len(addrs), 61, np.int32)), up(np.array(offs, np.uint64))
    router.route_dst_batch(dev, d_arena, d_sizes, small.d_image, d_peer, off=d_off, n=len(addrs))
    dev.sync()
    assert as_u32(d_peer, len(addrs)).tolist() == [2, 1, PEER_NONE, PEER_NONE, 5, 4, PEER_NONE, 1, PEER_NONE]
    L, img = dev.lib, small.d_image
    bad = [
        L.wgcs_route_dst_batch(dev.h, None, d_off.data_ptr(), 0, 0, d_sizes.data_ptr(), 1, img.data_ptr(), len(small.image),
                               d_peer.data_ptr(), None),
        L.wgcs_route_dst_batch(dev.h, d_arena.data_ptr(), d_off.data_ptr(), 0, 0, d_sizes.data_ptr(), 1,
                               img.data_ptr() + 8, len(small.image) - 8, d_peer.data_ptr(), None),  # image alignment
        L.wgcs_route_dst_batch(dev.h, d_arena.data_ptr(), d_off.data_ptr(), 0, 0, d_sizes.data_ptr(), 1, img.data_ptr(), 31,
                               d_peer.data_ptr(), None),  # shorter than a header
        L.wgcs_route_dst_batch(dev.h, d_arena.data_ptr(), d_off.data_ptr(), 0, 0, d_sizes.data_ptr(), (1 << 28) + 1,
                               img.data_ptr(), len(small.image), d_peer.data_ptr(), None),
        L.wgcs_route_dst_batch(dev.h, d_arena.data_ptr(), d_off.data_ptr() + 4, 0, 0, d_sizes.data_ptr(), 1, img.data_ptr(),
                               len(small.image), d_peer.data_ptr(), None),
        L.wgcs_recv_source_batch(dev.h, d_arena.data_ptr(), None, d_sizes.data_ptr(), None, 0, 1, img.data_ptr(),
                                 len(small.image), d_sizes.data_ptr(), None, None),
        L.wgcs_recv_classify_batch(dev.h, d_arena.data_ptr(), None, 64, d_sizes.data_ptr(), 1, d_off.data_ptr(), 3,
                                   d_off.data_ptr(), d_peer.data_ptr(), None),  # n_slots not a power of two
        L.wgcs_recv_classify_batch(None, None, None, 0, None, 1, None, 1, None, None, None),
    ]
    assert bad == [_lib.ERR_INVALID_ARG] * len(bad)


# ---------------------------------------------------------------- classify

def make_sessions(rng, with_edges):
    idx = set([0, 0xFFFFFFFF] if with_edges else [])
    while len(idx) < 64:
        v = int(rng.integers(1, 2**32 - 1))
        if v not in (0x01010101, 0xFFFFFFFE):
            idx.add(v)
    idx = sorted(idx)
    keys = [int(k) for k in rng.permutation(64)]
    return dict(zip(idx, keys))


def make_keys(rng, n):
    keys = np.zeros(n, AEAD_KEY_DTYPE)
    keys["key"] = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32)
    keys["remote_index"] = np.arange(n) + 0x1000
    return keys


def classify_cases(rng, sessions, keys):
    """[(message bytes as laid down, size)].  149 bytes are laid down for every
    message whatever its size, so a kernel that read past `size` would show."""
    present = [i for i in sessions if i not in (0, 0xFFFFFFFF)][:2] + [0, 0xFFFFFFFF]
    cases = []
    k = 0
    for size in (-1, 0, 31, 32, 63, 64, 65, 91, 92, 93, 147, 148, 149):
        for t, receiver in ((1, None), (2, None), (3, None), (4, "present"), (4, 0x01010101), (4, 0), (4, 0xFFFFFFFF),
                            (4, 0xFFFFFFFE), (0, None), (5, None), (0x00000104, None)):
            if receiver == "present":
                receiver = present[k % 2]
                k += 1
            body = bytearray(rng.bytes(149))
            body[0:4] = struct.pack("<I", t)
            if receiver is not None:
                body[4:8] = struct.pack("<I", receiver)
            cases.append((bytes(body), size))
    # two messages that open: sealed for the sessions of receiver 0 / 0xFFFFFFFF when those are listed
    for receiver, pt_len in ((present[2], 28), (present[3], 0), (present[0], 48)):
        key = sessions.get(receiver, 0)
        pkt = ip_packet(0x45, pt_len)
        if pt_len:
            pkt = pkt[:2] + struct.pack(">H", pt_len) + pkt[4:]
        msg = aead_ref.wg_seal(keys[key]["key"].tobytes(), receiver, 7 + pt_len, pkt, 0)
        cases.append((msg + bytes(rng.bytes(149 - len(msg))), len(msg)))
    return cases


@pytest.mark.parametrize("with_edges", [True, False])
def test_classify_then_open(dev, with_edges):
    """Receiver indices 0 and 0xFFFFFFFF are listed in one table and missing
    from the other; d_pkts goes straight into open_batch and must give what
    host-built descriptors give."""
    rng = np.random.default_rng(145207 + with_edges)
    sessions = make_sessions(rng, with_edges)
    keys = make_keys(rng, 64)
    slots = router.session_table(list(sessions), list(sessions.values()), 128)
    cases = classify_cases(rng, sessions, keys)
    n = len(cases)
    d_slots, d_keys = up(slots), up(keys)

    def run(n, arena, sizes, ref, **where):
        d_arena, d_pkts, d_type = up(arena), up(np.zeros(n, AEAD_PKT_DTYPE)), i32(n)
        router.classify_batch(dev, d_arena, up(np.array(sizes, np.int32)), d_slots, d_pkts, d_type, n=n, **where)
        dev.sync()
        pk = d_pkts.cpu().numpy().view(AEAD_PKT_DTYPE)
        assert d_type.cpu().numpy()[:n].tolist() == [r[0] for r in ref]
        assert pk["len"].tolist() == [r[1] for r in ref] and pk["key"].tolist() == [r[2] for r in ref]
        assert not pk["counter"].any()
        assert np.array_equal(d_arena.cpu().numpy(), arena)
        return d_arena, d_pkts, pk

    # d_off form, plus two rows that only it can carry: a size past 65535 (nothing read) and 152 bytes
    bodies = [c[0] for c in cases]
    long152 = bytes(struct.pack("<II", 4, next(iter(sessions)))) + bytes(rng.bytes(144))
    arena2, offs2 = lay_out(bodies + [long152], gap=0, pitch=163)
    big_off = len(arena2)  # a 65536-byte message would start here: OUT_OF_RANGE, so the arena need not hold it
    sizes2 = [c[1] for c in cases] + [152]
    n0, n = n, n + 2
    ref2 = [router_ref.classify(b, s, sessions) for b, s in zip(bodies + [long152], sizes2)]
    ref2.append((ERR_OUT_OF_RANGE, 0, NO_KEY))
    assert ref2[-2][0] == 4
    d_off = up(np.array(offs2 + [big_off], np.uint64))
    d_arena, d_pkts, pk = run(n, arena2, sizes2 + [65536], ref2, off=d_off)
    assert pk["off"].tolist() == offs2 + [big_off]
    types = [r[0] for r in ref2]
    assert {0, 1, 2, 3, 4, ERR_OUT_OF_RANGE} == set(types) and types.count(1) == types.count(2) == types.count(3) == 1

    # open on the kernel's descriptors == open on descriptors built here from the reference's decisions
    host = np.zeros(n, AEAD_PKT_DTYPE)
    host["off"], host["len"], host["key"] = offs2 + [big_off], [r[1] for r in ref2], [r[2] for r in ref2]
    outs = []
    for d in (d_pkts, up(host)):
        a, d_len, d_ctr = up(arena2), i32(n), torch.full((n,), -7, dtype=torch.int64, device="cuda")
        transport.open_batch(dev, a, d, d_keys, d_len, d_ctr, n=n, n_keys=64)
        dev.sync()
        outs.append((a.cpu().numpy(), d_len.cpu().numpy(), d_ctr.cpu().numpy()))
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x, y)
    lens = outs[0][1].tolist()
    assert lens[n0 - 3:n0] == [28, 0, 48] if with_edges else lens[n0 - 1] == 48  # the sealed ones open
    for r, got in zip(ref2, lens):
        if r[2] == NO_KEY:  # not a listed transport message: open refuses the row untouched
            assert got in (ERR_INVALID_ARG, ERR_OUT_OF_RANGE)

    # strided form over the same messages: 152 > stride 151 is OUT_OF_RANGE there
    n = n0 + 1
    arena3, offs3 = lay_out(bodies + [long152[:148]], gap=0, pitch=151)
    assert offs3 == [3 + 151 * q for q in range(n)]
    ref3 = [router_ref.classify(b, s, sessions, stride=151) for b, s in zip(bodies + [long152], sizes2)]
    assert ref3[-1] == (ERR_OUT_OF_RANGE, 0, NO_KEY) and ref3[:-1] == ref2[:n0]
    d_arena, d_pkts, pk = run(n, arena3[3:], sizes2, ref3, stride=151)
    assert pk["off"].tolist() == [151 * q for q in range(n)]


# ---------------------------------------------------------------- source, and the chain

PEER_A, PEER_B = 1, 2  # small: 10/8 and 2001:db8::/32 are peer 1's, 10.1/16 peer 2's


def v4_packet(src, size=28):
    p = bytearray(ip_packet(0x45, size, src=src, dst=V4("10.9.9.9")))
    p[2:4] = struct.pack(">H", size)
    return bytes(p)


def v6_packet(src, size=48):
    p = bytearray(ip_packet(0x60, size, src=src, dst=V6("2001:db8::9")))
    p[4:6] = struct.pack(">H", size - 40)
    return bytes(p)


def seal_on_device(dev, plains, key_of, keys, counters):
    """Seal plains[i] under keys[key_of[i]] with seal_batch; returns (arena, offsets, message lengths)."""
    room = [b"\0" * HDR + p + b"\0" * (32 + 16) for p in plains]
    arena, offs = lay_out(room, gap=0)
    pk = np.zeros(len(plains), AEAD_PKT_DTYPE)
    pk["off"], pk["counter"], pk["len"], pk["key"] = offs, counters, [len(p) for p in plains], key_of
    d_arena, d_len = up(arena), i32(len(plains))
    transport.seal_batch(dev, d_arena, up(pk), up(keys), 0, d_len, n=len(plains), n_keys=len(keys))
    dev.sync()
    lens = d_len.cpu().numpy()[:len(plains)].tolist()
    assert lens == [32 + len(p) + aead_ref.padding(len(p), 0) for p in plains]
    return d_arena.cpu().numpy(), offs, lens


def test_source_after_seal_and_open(dev, small):
    rng = np.random.default_rng(438482)
    keys = make_keys(rng, 6)
    key_peer = [PEER_A, PEER_B, 4, 5, 3]  # five rows: key 5 opens, but the source check has no peer for it
    rows = [  # (packet, key)
        (v4_packet(V4("10.2.3.4")), 0),  # allowed: 10/8 is peer 1's
        (v4_packet(V4("10.1.3.4")), 0),  # routed to peer 2
        (v4_packet(V4("10.1.3.4")), 1),  # ... which is allowed for key 1
        (v4_packet(V4("11.0.0.1")), 0),  # no route
        (b"", 0),  # keepalive
        (v4_packet(V4("10.2.3.4"), 44), 0),  # its tag is damaged below
        (v6_packet(V6("2001:db8::77")), 0),  # v6, allowed
        (v6_packet(V6("fd00:0:0:1::5")), 0),  # v6, peer 5's
        (v6_packet(V6("fd00:0:0:1::5")), 3),  # ... allowed for key 3
        (v4_packet(V4("10.2.3.4")), 5),  # key >= n_keys of the source check
        (ip_packet(0x55, 32), 0),  # version 5: open reports PACKET_TOO_SHORT, which passes through
    ]
    plains, key_of = [r[0] for r in rows], [r[1] for r in rows]
    n = len(rows)
    sealed, offs, lens = seal_on_device(dev, plains, key_of, keys, np.arange(n) + 1)
    sealed[offs[5] + lens[5] - 1] ^= 0x80
    opk = np.zeros(n, AEAD_PKT_DTYPE)
    opk["off"], opk["len"], opk["key"] = offs, lens, key_of
    d_arena, d_opk, d_len, d_ctr = up(sealed), up(opk), i32(n), torch.zeros(n, dtype=torch.int64, device="cuda")
    transport.open_batch(dev, d_arena, d_opk, up(keys), d_len, d_ctr, n=n, n_keys=6)
    dev.sync()
    opened, pkt_len = d_arena.cpu().numpy(), d_len.cpu().numpy()[:n].tolist()
    assert pkt_len == [28, 28, 28, 28, 0, _lib.ERR_AUTH, 48, 48, 48, 28, ERR_PACKET_TOO_SHORT]
    want = [28, ERR_SOURCE, 28, ERR_SOURCE, 0, _lib.ERR_AUTH, 48, ERR_SOURCE, 48, ERR_INVALID_ARG, ERR_PACKET_TOO_SHORT]
    ref = [router_ref.source_verdict(small.ref, p, l, k, key_peer) for p, l, k in zip(plains, pkt_len, key_of)]
    assert [r[0] for r in ref] == want
    d_key_peer = up(np.array(key_peer, np.uint32))
    d_verdict, d_found = i32(n), u32_out(n)
    router.source_batch(dev, d_arena, d_opk, d_len, d_key_peer, small.d_image, d_verdict, peer=d_found, n=n)
    dev.sync()
    assert d_verdict.cpu().numpy()[:n].tolist() == want
    assert as_u32(d_found, n).tolist() == [none_to(r[1]) for r in ref]
    assert d_len.cpu().numpy()[:n].tolist() == pkt_len
    # the verdict written over pkt_len, and no d_peer
    router.source_batch(dev, d_arena, d_opk, d_len, d_key_peer, small.d_image, d_len, n=n)
    dev.sync()
    assert d_len.cpu().numpy()[:n].tolist() == want
    assert np.array_equal(d_arena.cpu().numpy(), opened)


def test_receive_chain_on_one_stream(dev, small):
    """classify -> open -> source, enqueued back to back on one stream with one
    synchronisation at the end, against the same decisions made in Python."""
    rng = np.random.default_rng(32)
    keys = make_keys(rng, 4)
    key_peer = [PEER_A, PEER_B, 5, 3]
    receivers = [0x11111111, 0, 0xFFFFFFFF, 0x80000001]  # receiver index of key k
    sessions = {r: k for k, r in enumerate(receivers)}
    srcs = [V4("10.2.0.1"), V4("10.1.0.1"), V4("172.16.0.1"), V6("2001:db8::5"), V6("fd00:0:0:1::1"), V6("fe80::1")]
    plains, key_of = [], []
    for i in range(24):
        s = srcs[i % len(srcs)]
        plains.append(v4_packet(s, 28 + i) if len(s) == 4 else v6_packet(s, 48 + i))
        key_of.append(i % 4)
    plains += [b"", b""]  # keepalives
    key_of += [0, 3]
    m = len(plains)
    # sealed on the device first (set-up, with its own sync); the header's receiver index is keys[k].remote_index
    keys["remote_index"] = receivers
    sealed, offs, lens = seal_on_device(dev, plains, key_of, keys, np.arange(m) + 100)
    msgs = [bytes(sealed[o:o + l]) for o, l in zip(offs, lens)]
    msgs[3] = msgs[3][:-1] + bytes([msgs[3][-1] ^ 1])  # a damaged tag
    msgs[5] = msgs[5][:4] + struct.pack("<I", 0x22222222) + msgs[5][8:]  # an unknown receiver
    msgs += [struct.pack("<I", 1) + bytes(rng.bytes(144)), struct.pack("<I", 2) + bytes(rng.bytes(88)),
             struct.pack("<I", 3) + bytes(rng.bytes(61)), struct.pack("<I", 4) + bytes(rng.bytes(20)),
             struct.pack("<I", 7) + bytes(rng.bytes(60)), bytes(rng.bytes(5))]
    n = len(msgs)
    assert n == 32
    arena, offs = lay_out(msgs, gap=0)
    sizes = [len(x) for x in msgs]

    # the decisions in Python
    want_type, want_verdict, want_plain = [], [], arena.copy()
    for q, (msg, off) in enumerate(zip(msgs, offs)):
        t, length, key = router_ref.classify(msg, len(msg), sessions)
        want_type.append(t)
        if key == NO_KEY:
            want_verdict.append(ERR_OUT_OF_RANGE if length < 32 else ERR_INVALID_ARG)  # open's own refusals
            continue
        _, plain = aead_ref.wg_open(keys[key]["key"].tobytes(), msg)
        if plain is None:
            want_verdict.append(_lib.ERR_AUTH)
            want_plain[off + 16:off + len(msg) - 16] = 0
            continue
        want_plain[off + 16:off + len(msg) - 16] = np.frombuffer(plain, np.uint8)
        want_verdict.append(router_ref.source_verdict(small.ref, plain, aead_ref.trim(plain), key, key_peer)[0])
    assert want_type.count(4) == 25 and sorted(set(want_type)) == [0, 1, 2, 4]
    assert {ERR_SOURCE, _lib.ERR_AUTH, ERR_INVALID_ARG, ERR_OUT_OF_RANGE, 0} <= set(want_verdict)
    assert sum(v > 0 for v in want_verdict) >= 6

    d_arena, d_off, d_sizes = up(arena), up(np.array(offs, np.uint64)), up(np.array(sizes, np.int32))
    d_slots, d_keys = up(router.session_table(receivers, [0, 1, 2, 3], 8)), up(keys)
    d_key_peer = up(np.array(key_peer, np.uint32))
    d_pkts, d_type, d_len = up(np.zeros(n, AEAD_PKT_DTYPE)), i32(n), i32(n)
    d_ctr = torch.zeros(n, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    router.classify_batch(dev, d_arena, d_sizes, d_slots, d_pkts, d_type, off=d_off, stream=stream, n=n)
    transport.open_batch(dev, d_arena, d_pkts, d_keys, d_len, d_ctr, stream=stream, n=n, n_keys=4)
    router.source_batch(dev, d_arena, d_pkts, d_len, d_key_peer, small.d_image, d_len, stream=stream, n=n)
    stream.synchronize()
    assert d_type.cpu().numpy()[:n].tolist() == want_type
    assert d_len.cpu().numpy()[:n].tolist() == want_verdict
    assert np.array_equal(d_arena.cpu().numpy(), want_plain)
