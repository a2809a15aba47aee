"""Two independent references for the allowed-IPs router, written from the Go
text of device/router.go (tests only; the product is router.cpp).

RefRouter   a line-by-line restatement with objects, the parent{child,
            childIndex} indirection (a slot object stands for the **node) and
            per-peer node lists, as the reference has them.
BruteRouter longest-prefix match over a dict {(family, masked addr, cidr):
            peer}, with Insert's replace and Remove's only-if-same-peer rules.

Addresses are bytes of length 4 or 16; peers are ints; None is Go's nil.
The decisions of the receive and send loops that the GPU tests compare against
(classify / source / dst) are restated at the bottom.
"""
from __future__ import annotations

import struct


def common_bits(ip1: bytes, ip2: bytes) -> int:
    """commonBits, router.go:63-91."""
    if len(ip1) == 4:
        x = int.from_bytes(ip1, "big") ^ int.from_bytes(ip2[:4], "big")
        return 32 - x.bit_length()
    if len(ip1) == 16:
        x = int.from_bytes(ip1[:8], "big") ^ int.from_bytes(ip2[:8], "big")
        if x != 0:
            return 64 - x.bit_length()
        x = int.from_bytes(ip1[8:], "big") ^ int.from_bytes(ip2[8:16], "big")
        return 64 + 64 - x.bit_length()
    raise ValueError("wrong size bit string")


def mask_addr(addr: bytes, cidr: int) -> bytes:
    """maskSelf, :126-139 (net.CIDRMask)."""
    bits = len(addr) * 8
    m = ((1 << bits) - 1) ^ ((1 << (bits - cidr)) - 1)
    return (int.from_bytes(addr, "big") & m).to_bytes(len(addr), "big")


class _Slot:
    """What a **node points at: one element of a children array, or a root."""

    def __init__(self, owner, index):
        self.owner, self.index = owner, index  # owner: _Node or RefRouter

    def get(self):
        return self.owner.children[self.index] if isinstance(self.owner, _Node) else self.owner.roots[self.index]

    def set(self, n):
        if isinstance(self.owner, _Node):
            self.owner.children[self.index] = n
        else:
            self.owner.roots[self.index] = n


class _Parent:
    def __init__(self, child: _Slot | None, child_index: int):
        self.child, self.child_index = child, child_index


class _Node:
    def __init__(self, cidr, addr, peer=None, parent=None):
        self.parent = parent or _Parent(None, 0)
        self.children = [None, None]
        self.cidr, self.index, self.shift = cidr, cidr // 8, 7 - (cidr % 8)
        self.addr = bytearray(addr)
        self.peer = peer
        self.in_list = False  # peerNode != nil

    def child_index(self, ip) -> int:  # :95-97
        return (ip[self.index] >> self.shift) & 1

    def mask_self(self):
        self.addr[:] = mask_addr(bytes(self.addr), self.cidr)


class RefRouter:
    def __init__(self):
        self.roots = [None, None]  # IPv4, IPv6
        self.peer_nodes: dict[int, list[_Node]] = {}  # Peer.nodes

    # -- list plumbing, :141-150
    def _add_to_peer_nodes(self, n):
        self.peer_nodes.setdefault(n.peer, []).append(n)
        n.in_list = True

    def _remove_from_peer_nodes(self, n):
        if n.in_list:
            self.peer_nodes[n.peer].remove(n)
            n.in_list = False

    @staticmethod
    def _placement(n, ip, cidr):  # nodePlacement, :99-122
        parent, exact = None, False
        while n is not None and n.cidr <= cidr and common_bits(bytes(n.addr), ip) >= n.cidr:
            parent = n
            if parent.cidr == cidr:
                return parent, True
            n = n.children[n.child_index(ip)]
        return parent, exact

    def _insert(self, p: _Parent, ip: bytearray, cidr: int, peer: int):  # :160-270
        """Returns the case numbers of router.go's comments that this insert took."""
        if p.child.get() is None:  # CASE 1
            nn = _Node(cidr, ip, peer, p)
            nn.mask_self()
            self._add_to_peer_nodes(nn)
            p.child.set(nn)
            return [1]
        parent_node, exact = self._placement(p.child.get(), bytes(ip), cidr)
        if exact:  # CASE 2
            self._remove_from_peer_nodes(parent_node)
            parent_node.peer = peer
            self._add_to_peer_nodes(parent_node)
            return [2]
        nn = _Node(cidr, ip, peer)
        nn.mask_self()
        ip = nn.addr  # the Go slice aliases newNode.addr: masked from here on
        self._add_to_peer_nodes(nn)
        if parent_node is None:  # CASE 3
            cases = [3]
            down = p.child.get()
        else:  # CASE 4
            cases = [4]
            index = parent_node.child_index(ip)
            down = parent_node.children[index]
            if down is None:  # CASE 5
                nn.parent = _Parent(_Slot(parent_node, index), index)
                parent_node.children[index] = nn
                return cases + [5]
        common = common_bits(bytes(down.addr), bytes(ip))
        cidr = min(cidr, common)
        if nn.cidr == cidr:  # CASE 6
            index = nn.child_index(down.addr)
            down.parent = _Parent(_Slot(nn, index), index)
            nn.children[index] = down
            if parent_node is None:  # CASE 7
                nn.parent = p
                p.child.set(nn)
                return cases + [6, 7]
            index = parent_node.child_index(nn.addr)  # CASE 8
            nn.parent = _Parent(_Slot(parent_node, index), index)
            parent_node.children[index] = nn
            return cases + [6, 8]
        cn = _Node(cidr, bytes(nn.addr))  # commonNode
        cn.mask_self()
        index = cn.child_index(down.addr)
        down.parent = _Parent(_Slot(cn, index), index)
        cn.children[index] = down
        index = cn.child_index(nn.addr)
        nn.parent = _Parent(_Slot(cn, index), index)
        cn.children[index] = nn
        if parent_node is None:  # CASE 9
            cn.parent = p
            p.child.set(cn)
            return cases + [9]
        index = parent_node.child_index(cn.addr)  # CASE 10
        cn.parent = _Parent(_Slot(parent_node, index), index)
        parent_node.children[index] = cn
        return cases + [10]

    def _remove(self, n: _Node):  # node.remove, :273-372
        """Returns the name of the branch taken."""
        self._remove_from_peer_nodes(n)
        n.peer = None
        if n.children[0] is not None and n.children[1] is not None:
            return "two-children"
        index = 1 if n.children[0] is None else 0
        child = n.children[index]
        if child is not None:
            child.parent = n.parent
        n.parent.child.set(child)
        if child is not None or n.parent.child_index > 1:
            return "one-child" if child is not None else "root-leaf"
        parent = n.parent.child.owner  # the pointer arithmetic of :347-351
        if parent.peer is not None:
            return "leaf"
        child = parent.children[n.parent.child_index ^ 1]
        if child is not None:
            child.parent = parent.parent
        parent.parent.child.set(child)
        return "leaf-empty-parent-sibling" if child is not None else "leaf-empty-parent-alone"

    # -- Router, :405-495
    def insert(self, addr: bytes, cidr: int, peer: int):
        fam = {4: 0, 16: 1}[len(addr)]
        return self._insert(_Parent(_Slot(self, fam), 2), bytearray(addr), cidr, peer)

    def find(self, ip: bytes):
        n = self.roots[{4: 0, 16: 1}[len(ip)]]
        peer = None
        while n is not None and common_bits(bytes(n.addr), ip) >= n.cidr:  # node.find, :374-403
            if n.peer is not None:
                peer = n.peer
            if n.index == len(ip):
                break
            n = n.children[n.child_index(ip)]
        return peer

    def remove(self, addr: bytes, cidr: int, peer: int):
        n, exact = self._placement(self.roots[{4: 0, 16: 1}[len(addr)]], addr, cidr)
        if n is None or not exact or peer != n.peer:
            return None
        return self._remove(n)

    def remove_by_peer(self, peer: int):
        return [self._remove(n) for n in list(self.peer_nodes.get(peer, []))]

    def peer_prefixes(self, peer: int):
        return [(bytes(n.addr), n.cidr) for n in self.peer_nodes.get(peer, [])]

    def node_count(self) -> int:
        def count(n):
            return 0 if n is None else 1 + count(n.children[0]) + count(n.children[1])
        return count(self.roots[0]) + count(self.roots[1])


class BruteRouter:
    """Keys are (address length, masked address as an int, cidr)."""

    def __init__(self):
        self.table: dict[tuple[int, int, int], int] = {}
        self.order: dict[tuple[int, int, int], int] = {}
        self.tick = 0

    @staticmethod
    def _key(addr: bytes, cidr: int):
        return len(addr), int.from_bytes(mask_addr(addr, cidr), "big"), cidr

    def insert(self, addr: bytes, cidr: int, peer: int):
        k = self._key(addr, cidr)
        self.table[k] = peer
        self.tick += 1
        self.order[k] = self.tick

    def remove(self, addr: bytes, cidr: int, peer: int):
        k = self._key(addr, cidr)
        if self.table.get(k) == peer:
            del self.table[k], self.order[k]

    def remove_by_peer(self, peer: int):
        for k in [k for k, p in self.table.items() if p == peer]:
            del self.table[k], self.order[k]

    def find(self, ip: bytes):
        best, best_cidr = None, -1
        bits, x = 8 * len(ip), int.from_bytes(ip, "big")
        for (fam, addr, cidr), peer in self.table.items():
            if fam == len(ip) and cidr > best_cidr and (x ^ addr) >> (bits - cidr) == 0:
                best, best_cidr = peer, cidr
        return best

    def prefixes(self):
        """[(address bytes, cidr)] of every prefix present."""
        return [(addr.to_bytes(fam, "big"), cidr) for fam, addr, cidr in self.table]

    def peer_prefixes(self, peer: int):
        ks = sorted((k for k, p in self.table.items() if p == peer), key=self.order.get)
        return [(k[1].to_bytes(k[0], "big"), k[2]) for k in ks]


# ---- the per-packet decisions of the receive and send loops ----

ERR_INVALID_ARG, ERR_PACKET_TOO_SHORT, ERR_OUT_OF_RANGE, ERR_SOURCE = -1, -8, -13, -19
NO_KEY = 0xFFFFFFFF


def classify(msg: bytes, size: int, sessions: dict[int, int], stride: int | None = None):
    """(type, len, key) of RoutineReceiveFromPeers' loop body (receive.go:145-207)
    as the batch entry point reports it; msg holds at least max(size, 0) bytes."""
    if size < 32:
        return 0, size & 0xFFFFFFFF, NO_KEY
    if size > 65535 or (stride is not None and size > stride):
        return ERR_OUT_OF_RANGE, 0, NO_KEY
    t, = struct.unpack_from("<I", msg, 0)
    if t == 4:
        receiver, = struct.unpack_from("<I", msg, 4)
        if receiver in sessions:
            return 4, size, sessions[receiver]
        return 0, size, NO_KEY
    if (t, size) in ((1, 148), (2, 92), (3, 64)):
        return t, size, NO_KEY
    return 0, size, NO_KEY


def source_verdict(router, packet: bytes, pkt_len: int, key: int, key_peer: list[int]):
    """(verdict, found peer or None) of the allowed-source check (receive.go:432-482)."""
    if pkt_len <= 0:
        return pkt_len, None
    if key >= len(key_peer):
        return ERR_INVALID_ARG, None
    v = packet[0] >> 4
    if v == 4 and pkt_len >= 20:
        peer = router.find(bytes(packet[12:16]))
    elif v == 6 and pkt_len >= 40:
        peer = router.find(bytes(packet[8:24]))
    else:
        return ERR_PACKET_TOO_SHORT, None
    return (pkt_len if peer == key_peer[key] else ERR_SOURCE), peer


def route_dst(router, packet: bytes, size: int):
    """The peer RoutineReadFromTUN routes the packet to, or None (send.go:264-293)."""
    if size < 1:
        return None
    v = packet[0] >> 4
    if v == 4 and size >= 20:
        return router.find(bytes(packet[16:20]))
    if v == 6 and size >= 40:
        return router.find(bytes(packet[24:40]))
    return None
