"""The host router and session table of libwgcsum.so (router.cpp) through
ctypes, against the two references of router_ref.py (CPU only).

After every operation the trie (wgcs_router_find), a fresh image walked by the
kernels' own code (wgcs_router_image_find), the line-by-line restatement and
the brute-force longest-prefix match must agree on the first and last address
of every prefix present and on their neighbours; the image must have as many
nodes as the restatement's tries (so empty nodes stay and leave as the
reference's do), and every peer's prefix list must come in the reference's
order.

node.remove's last branch has a half that cannot be reached through Router: an
empty node (peer == nil) always has two children -- it is made with two
(commonNode, or a removed node that had two), a child that leaves with one
child of its own is replaced by that child, a child that leaves as a leaf
takes the empty node with it, and an insert below it only ever replaces what a
child slot holds.  So "a leaf under an empty parent without a sibling" never
runs; the random test asserts that and covers the half with a sibling."""
import ctypes as C
import ipaddress
import random

import numpy as np
import pytest

import router_ref
from wireguard_amd import _lib, router
from wireguard_amd.router import PEER_NONE, Router

V4 = lambda s: ipaddress.IPv4Address(s).packed  # noqa: E731
V6 = lambda s: ipaddress.IPv6Address(s).packed  # noqa: E731


class Trio:
    """The C router and both references, driven together."""

    def __init__(self):
        self.c, self.ref, self.brute = Router(), router_ref.RefRouter(), router_ref.BruteRouter()
        self.peers = set()

    def insert(self, addr, cidr, peer):
        self.peers.add(peer)
        self.c.insert(addr, cidr, peer)
        self.brute.insert(addr, cidr, peer)
        return self.ref.insert(addr, cidr, peer)

    def remove(self, addr, cidr, peer):
        self.c.remove(addr, cidr, peer)
        self.brute.remove(addr, cidr, peer)
        return self.ref.remove(addr, cidr, peer)

    def remove_by_peer(self, peer):
        self.c.remove_by_peer(peer)
        self.brute.remove_by_peer(peer)
        return self.ref.remove_by_peer(peer)

    def probes(self):
        out = set()
        for addr, cidr in self.brute.prefixes():
            bits = 8 * len(addr)
            first = int.from_bytes(addr, "big")
            last = first | ((1 << (bits - cidr)) - 1)
            for x in (first - 1, first, first + 1, last - 1, last, last + 1):
                out.add((x % (1 << bits)).to_bytes(len(addr), "big"))
        out.update((bytes(4), b"\xff" * 4, bytes(16), b"\xff" * 16))
        return sorted(out)

    def check(self):
        image = self.c.image()
        assert len(image) == 32 + 32 * self.ref.node_count(), "node count (empty nodes included)"
        for ip in self.probes():
            want = self.brute.find(ip)
            assert self.ref.find(ip) == want, ip.hex()
            want = PEER_NONE if want is None else want
            assert self.c.find(ip) == want, ip.hex()
            assert router.image_find(image, ip) == want, ip.hex()
        for peer in self.peers:
            want = self.ref.peer_prefixes(peer)
            assert self.brute.peer_prefixes(peer) == want
            assert self.c.peer_prefixes(peer) == want, peer


def test_each_insert_case():
    """The ten cases named in parent.insert's comments (3 and 4 are the two
    arms that the later cases hang under)."""
    seen = set()

    def step(t, addr, cidr, peer, cases):
        assert t.insert(V4(addr), cidr, peer) == cases
        seen.update(cases)
        t.check()

    t = Trio()
    step(t, "10.0.0.0", 8, 1, [1])
    step(t, "10.9.9.9", 8, 2, [2])  # masked to the same prefix: replace
    step(t, "0.0.0.0", 0, 3, [3, 6, 7])  # a new root above the old one
    t = Trio()
    step(t, "10.0.0.0", 8, 1, [1])
    step(t, "192.168.0.0", 16, 2, [3, 9])  # an empty /0 root joins the two
    t = Trio()
    step(t, "10.0.0.0", 8, 1, [1])
    step(t, "10.1.0.0", 16, 2, [4, 5])
    step(t, "10.1.2.0", 24, 3, [4, 5])
    step(t, "10.1.0.0", 20, 4, [4, 6, 8])  # between /16 and /24
    step(t, "10.2.0.0", 16, 5, [4, 10])  # an empty /14 joins 10.1/16 and 10.2/16
    assert seen == set(range(1, 11))
    assert t.c.find(V4("10.1.2.3")) == 3 and t.c.find(V4("10.1.9.1")) == 4 and t.c.find(V4("10.3.0.1")) == 1


def test_each_remove_branch():
    t = Trio()
    t.insert(V4("10.0.0.0"), 8, 1)
    t.insert(V4("10.0.0.0"), 9, 2)
    t.insert(V4("10.128.0.0"), 9, 3)
    assert t.remove(V4("10.0.0.0"), 8, 1) == "two-children"  # the node stays, empty
    t.check()
    assert t.c.find(V4("10.1.1.1")) == 2 and len(t.c.image()) == 32 + 3 * 32
    assert t.remove(V4("10.0.0.0"), 9, 2) == "leaf-empty-parent-sibling"  # the sibling becomes the root
    t.check()
    assert len(t.c.image()) == 32 + 32 and t.c.find(V4("10.1.1.1")) == PEER_NONE
    assert t.remove(V4("10.128.0.0"), 9, 3) == "root-leaf"
    t.check()
    assert len(t.c.image()) == 32

    t = Trio()
    t.insert(V4("10.0.0.0"), 8, 1)
    t.insert(V4("10.1.0.0"), 16, 2)
    assert t.remove(V4("10.0.0.0"), 8, 1) == "one-child"  # the child takes the root slot
    t.check()
    t.insert(V4("10.0.0.0"), 8, 1)
    assert t.remove(V4("10.1.0.0"), 16, 2) == "leaf"  # under a parent that has a peer
    t.check()
    t.insert(V4("10.1.0.0"), 16, 2)
    t.insert(V4("10.1.1.0"), 24, 3)
    assert t.remove(V4("10.1.0.0"), 16, 2) == "one-child"  # in the middle of a chain
    t.check()
    assert t.c.find(V4("10.1.1.9")) == 3 and t.c.find(V4("10.1.2.9")) == 1

    # an empty commonNode with a sibling, below a parent (not at the root)
    t = Trio()
    t.insert(V4("10.0.0.0"), 8, 1)
    t.insert(V4("10.1.0.0"), 16, 2)
    assert t.insert(V4("10.2.0.0"), 16, 3) == [4, 10]
    assert t.remove(V4("10.2.0.0"), 16, 3) == "leaf-empty-parent-sibling"
    t.check()
    assert len(t.c.image()) == 32 + 2 * 32


def test_host_routes_and_default_routes():
    """/0, /32 and /128: find's `index == ipLen` break, and cidr 0's mask."""
    t = Trio()
    t.insert(V4("0.0.0.0"), 0, 1)
    t.insert(V4("10.0.0.1"), 32, 2)
    t.insert(V4("255.255.255.255"), 32, 3)
    t.insert(V6("::"), 0, 4)
    t.insert(V6("2001:db8::1"), 128, 5)
    t.insert(V6("ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff"), 128, 6)
    t.check()
    assert t.c.find(V4("10.0.0.1")) == 2 and t.c.find(V4("10.0.0.2")) == 1
    assert t.c.find(V6("2001:db8::1")) == 5 and t.c.find(V6("2001:db8::2")) == 4
    t.insert(V4("10.0.0.1"), 32, 7)  # exact replace of a host route
    t.remove(V6("2001:db8::1"), 128, 5)
    t.check()
    assert t.c.find(V4("10.0.0.1")) == 7 and t.c.find(V6("2001:db8::1")) == 4


def test_ipv6_prefixes_that_differ_beyond_bit_64():
    """commonBits' second half (router.go:83-87)."""
    t = Trio()
    t.insert(V6("2001:db8::"), 64, 1)
    t.insert(V6("2001:db8::8000:0:0:0"), 65, 2)
    t.insert(V6("2001:db8::1:0:0"), 96, 3)
    t.insert(V6("2001:db8::1:0:1"), 128, 4)
    t.insert(V6("2001:db8::1:0:2"), 127, 5)
    t.check()
    assert t.c.find(V6("2001:db8::1:0:1")) == 4 and t.c.find(V6("2001:db8::1:0:3")) == 5
    assert t.c.find(V6("2001:db8::2:0:0")) == 1 and t.c.find(V6("2001:db8::ffff:0:0:1")) == 2
    assert t.c.find(V6("2001:db9::")) == PEER_NONE


def test_replace_wrong_peer_remove_by_peer_and_prefix_order():
    t = Trio()
    for i, (a, c) in enumerate([("10.0.0.0", 8), ("10.1.0.0", 16), ("10.2.0.0", 16), ("172.16.0.0", 12)]):
        t.insert(V4(a), c, 1)
    t.insert(V6("fd00::"), 8, 1)
    t.insert(V4("10.1.0.0"), 16, 2)  # exact replace by another peer
    t.check()
    assert t.c.find(V4("10.1.2.3")) == 2
    assert t.c.peer_prefixes(1) == [(V4("10.0.0.0"), 8), (V4("10.2.0.0"), 16), (V4("172.16.0.0"), 12), (V6("fd00::"), 8)]
    t.insert(V4("10.0.0.0"), 8, 1)  # an exact re-insert moves the prefix to the back
    t.insert(V4("10.1.0.0"), 16, 1)  # and one taken back from peer 2 joins there
    t.check()
    assert t.c.peer_prefixes(1) == [(V4("10.2.0.0"), 16), (V4("172.16.0.0"), 12), (V6("fd00::"), 8), (V4("10.0.0.0"), 8),
                                    (V4("10.1.0.0"), 16)]
    assert t.c.peer_prefixes(2) == []
    assert t.remove(V4("10.2.0.0"), 16, 2) is None  # the wrong peer: a no-op
    assert t.remove(V4("10.2.0.0"), 17, 1) is None  # not present exactly
    t.check()
    assert t.c.find(V4("10.2.0.1")) == 1
    t.insert(V4("192.168.0.0"), 16, 3)
    t.remove_by_peer(1)
    t.check()
    assert t.c.peer_prefixes(1) == [] and t.c.find(V4("10.2.0.1")) == PEER_NONE and t.c.find(V6("fd00::1")) == PEER_NONE
    assert t.c.find(V4("192.168.1.1")) == 3 and len(t.c.image()) == 32 + 32
    t.remove_by_peer(9)  # a peer without prefixes
    t.check()


def test_argument_checks():
    L = _lib.load()
    r = Router()
    a4 = V4("10.0.0.0")
    assert L.wgcs_router_insert(r.h, a4, 5, 8, 1) == _lib.ERR_INVALID_ARG  # Go panics: unknown address type
    assert L.wgcs_router_insert(r.h, a4, 4, 33, 1) == _lib.ERR_INVALID_ARG
    assert L.wgcs_router_insert(r.h, V6("::"), 16, 129, 1) == _lib.ERR_INVALID_ARG
    assert L.wgcs_router_insert(r.h, a4, 4, 8, PEER_NONE) == _lib.ERR_INVALID_ARG
    assert L.wgcs_router_insert(None, a4, 4, 8, 1) == _lib.ERR_INVALID_ARG
    assert L.wgcs_router_find(r.h, a4, 5) == PEER_NONE and L.wgcs_router_find(None, a4, 4) == PEER_NONE
    assert len(r.image()) == 32 and r.find(a4) == PEER_NONE  # nothing went in
    r.insert(a4, 8, 1)
    img = r.image()
    n = C.c_size_t(0)
    small = np.zeros(len(img) - 1, np.uint8)
    assert L.wgcs_router_write_image(r.h, small.ctypes.data, len(small), C.byref(n)) == _lib.ERR_OUT_OF_RANGE
    peer = C.c_uint32(0)
    assert L.wgcs_router_image_find(img.ctypes.data, len(img), a4, 3, C.byref(peer)) == _lib.ERR_INVALID_ARG
    assert L.wgcs_router_image_find(img.ctypes.data, len(img) - 1, a4, 4, C.byref(peer)) == _lib.ERR_INVALID_ARG
    assert peer.value == PEER_NONE
    unaligned = np.zeros(len(img) + 1, np.uint8)
    unaligned[1:] = img
    assert router.image_find(unaligned[1:], V4("10.1.1.1")) == 1  # a host image may sit anywhere
    assert L.wgcs_strerror(_lib.ERR_SOURCE) == b"packet with disallowed source address"
    r.close()


def rand_prefix(rng):
    """A deliberately small universe, so that prefixes nest and collide."""
    if rng.random() < 0.6:
        addr = bytes([10, rng.choice((0, 1, 128)), rng.choice((0, 1)), rng.choice((0, 1, 255))])
        cidr = rng.choice((0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32))
    else:
        addr = V6("2001:db8::")[:8] + bytes([rng.choice((0, 128)), 0, 0, rng.choice((0, 1)), 0, 0, rng.choice((0, 1)),
                                             rng.choice((0, 1, 255))])
        cidr = rng.choice((0, 1, 32, 63, 64, 65, 96, 97, 120, 127, 128))
    return addr, cidr


def test_random_operations_against_both_references():
    rng = random.Random(20261019)
    t = Trio()
    cases, branches = set(), set()
    for _ in range(2000):
        op = rng.random()
        present = t.brute.prefixes()
        if op < 0.5 or not present:
            addr, cidr = rand_prefix(rng)
            cases.update(t.insert(addr, cidr, rng.randrange(1, 5)))
        elif op < 0.9:
            addr, cidr = rng.choice(present) if rng.random() < 0.8 else rand_prefix(rng)
            owner = t.brute.find(addr) if rng.random() < 0.8 else rng.randrange(1, 5)  # often the right peer
            branches.add(t.remove(addr, cidr, owner or 1))
        else:
            branches.update(t.remove_by_peer(rng.randrange(1, 5)))
        t.check()
    assert cases == set(range(1, 11))
    assert "leaf-empty-parent-alone" not in branches  # unreachable: see the module docstring
    assert branches >= {"two-children", "one-child", "root-leaf", "leaf", "leaf-empty-parent-sibling", None}


def slots_as_dict(slots):
    used = slots[slots["key"] != 0xFFFFFFFF]
    assert len(set(used["index"].tolist())) == len(used), "an index sits in two slots"
    return dict(zip(used["index"].tolist(), used["key"].tolist()))


def test_session_table():
    s = router.session_table([], [])
    assert len(s) == 1 and slots_as_dict(s) == {}  # n == 0: one empty slot
    assert slots_as_dict(router.session_table([], [], 8)) == {}
    s = router.session_table([0xDEADBEEF], [5], 2)
    assert len(s) == 2 and slots_as_dict(s) == {0xDEADBEEF: 5}
    rng = np.random.default_rng(7)
    idx = np.concatenate([[0, 0xFFFFFFFF], rng.integers(1, 2**32 - 1, 62, dtype=np.uint64)]).astype(np.uint32)
    assert len(set(idx.tolist())) == 64
    keys = np.arange(64, dtype=np.uint32)[::-1].copy()
    s = router.session_table(idx, keys, 128)
    assert len(s) == 128 and slots_as_dict(s) == dict(zip(idx.tolist(), keys.tolist()))
    assert router.session_table(idx, keys).shape == (128,)  # the default size
    for bad in (64, 96, 0, 127):  # < 2n, not a power of two
        with pytest.raises(_lib.WgcsError) as ei:
            router.session_table(idx, keys, bad)
        assert ei.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.WgcsError):  # a duplicate index
        router.session_table([7, 8, 7], [0, 1, 2], 8)
    with pytest.raises(_lib.WgcsError):  # the empty marker as a value
        router.session_table([7], [0xFFFFFFFF], 2)
    # sequential indices (a peer that counts up) still fit: linear probing, load <= 1/2
    seq = np.arange(1000, dtype=np.uint32)
    assert slots_as_dict(router.session_table(seq, seq, 2048)) == dict(zip(seq.tolist(), seq.tolist()))
