"""Named cases and a seeded generator for the endpoint tests: control buffers,
receive batches, and a World that keeps the C tables (ENDPOINT_DTYPE rows,
claim words, TIMERS_DTYPE rows) beside the restatement's Peer objects."""
import struct

import numpy as np

import endpoint_ref as ref
from cookiegen_cases import arena_of
from wireguard_amd import endpoint as ep, noise, router, timers as tm
from wireguard_amd._lib import HS_FINISHED, HS_INITIATED, HS_NONE, HS_RESPONDED, PEER_NONE
from wireguard_amd.cookie import SRC_ADDR_DTYPE
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

OOB_STRIDE = 96  # bytes of control per slot: room for every named case
CLEAR_SRC = ep.TIMERS_CLEAR_SRC

PKTINFO4 = ref.cmsg(ref.IPPROTO_IP, ref.IP_PKTINFO, struct.pack("<i4s4s", 3, bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])))
PKTINFO6 = ref.cmsg(ref.IPPROTO_IPV6, ref.IPV6_PKTINFO, bytes.fromhex("20010db8" + "00" * 11 + "07") + struct.pack("<I", 5))
GRO = ref.cmsg(ref.SOL_UDP, ref.UDP_GRO, struct.pack("<H", 1400))
UNKNOWN = ref.cmsg(1, 29, bytes(range(8)))  # SOL_SOCKET / SCM_TIMESTAMP, say


def pktinfo4_len(length: int, room: int = 48) -> bytes:
    """An IP_PKTINFO message whose Cmsghdr.Len is `length`, in `room` bytes of 0x11.. data."""
    body = struct.pack("<Qii", length, ref.IPPROTO_IP, ref.IP_PKTINFO) + bytes(range(0x11, 0x11 + room))
    return body[:max(16 + room, 16)]


def control_cases() -> dict:
    """name -> msg.OOB[:msg.NN]"""
    return {
        "no control": b"",
        "pktinfo4": PKTINFO4,
        "pktinfo4 before gro": PKTINFO4 + GRO,
        "pktinfo4 after gro": GRO + PKTINFO4,
        "pktinfo6": PKTINFO6,
        "len 16": pktinfo4_len(16, 16),
        "len 20": pktinfo4_len(20, 16),
        "len 28": pktinfo4_len(28, 16),
        "len 29": pktinfo4_len(29, 16),
        "len 64": pktinfo4_len(64, 48),
        "len beyond the buffer": pktinfo4_len(40, 16),
        "exactly 16 bytes": pktinfo4_len(16, 0),
        "unknown in front": UNKNOWN + PKTINFO6,
        "pktinfo6 len 64": struct.pack("<Qii", 64, ref.IPPROTO_IPV6, ref.IPV6_PKTINFO) + bytes(range(0x40, 0x70)),
        "bad len then pktinfo": struct.pack("<Qii", 8, 1, 1) + bytes(8) + PKTINFO4,
        "two pktinfo": PKTINFO6 + PKTINFO4,
    }


def dst_bytes(ip: bytes, port: int) -> bytes:
    return bytes(ip) + struct.pack("<H", port)


def addr_row(dst: bytes) -> np.ndarray:
    r = np.zeros(1, SRC_ADDR_DTYPE)
    r["b"][0, :len(dst)] = np.frombuffer(dst, np.uint8)
    r["len"] = len(dst)
    return r


def ep_row(endpoint) -> np.ndarray:
    """The canonical ENDPOINT_DTYPE row of a restatement endpoint (dst, src), or the zero row of None."""
    r = np.zeros(1, ep.ENDPOINT_DTYPE)
    if endpoint is not None:
        dst, src = endpoint
        r["dst"] = addr_row(dst)
        r["src_len"] = len(src)
        r["src"][0, :len(src)] = np.frombuffer(src, np.uint8)
    return r


def ep_rows(endpoints) -> np.ndarray:
    return np.concatenate([ep_row(e) for e in endpoints]) if len(endpoints) else np.zeros(0, ep.ENDPOINT_DTYPE)


def oob_of(controls, stride: int = OOB_STRIDE, fill: int = 0xCC):
    """(oob, nn): control q at q * stride in a buffer of exactly n * stride bytes; the rest keeps `fill`."""
    oob, nn = np.full(len(controls) * stride, fill, np.uint8), np.zeros(len(controls), np.int32)
    for q, c in enumerate(controls):
        assert len(c) <= stride
        oob[q * stride:q * stride + len(c)] = np.frombuffer(c, np.uint8)
        nn[q] = len(c)
    return oob, nn


def recv_ref(addrs, src_from, sizes, controls, n_msgs: int):
    """bind.go:308-319 per batch over what splitMessages left: slot i's Addr is that of message
    src_from[i] of its batch (-1: its own).  A src_from outside [-1, n_msgs) is not the
    reference's: the slot gets no endpoint."""
    out = []
    for b in range(len(sizes) // n_msgs):
        lo = b * n_msgs
        moved, size = [], []
        for s in range(n_msgs):
            f = -1 if src_from is None else int(src_from[lo + s])
            ok = -1 <= f < n_msgs
            moved.append(addrs[lo + s] if f == -1 else addrs[lo + f] if ok else None)
            size.append(int(sizes[lo + s]) if ok else 0)
        out += ref.receive_endpoints(moved, size, controls[lo:lo + n_msgs])
    return out


ADDRS = [dst_bytes(bytes([203, 0, 113, 5]), 40001), dst_bytes(bytes.fromhex("20010db8" + "00" * 11 + "09"), 7),
         dst_bytes(bytes([198, 51, 100, 7]), 51820), dst_bytes(bytes.fromhex("00" * 10 + "ffff" + "c0000201"), 9)]


def random_endpoints(rng, n: int):
    """n restatement endpoints (None: a slot of size 0), as a receive batch would hand them on."""
    controls = list(control_cases().values())
    out = []
    for _ in range(n):
        if rng.random() < 0.1:
            out.append(None)
        else:
            out.append((ADDRS[int(rng.integers(0, len(ADDRS)))], ref.get_src_from_control(controls[int(rng.integers(0, len(controls)))])))
    return out


class World:
    """n_peers peers: the C tables and the restatement's Peer objects, kept in step by the tests."""

    def __init__(self, rng, n_peers: int = 5, n_ids: int = 16):
        self.rng, self.n_peers, self.n_ids = rng, n_peers, n_ids
        self.ids = [int(i) for i in rng.permutation(n_ids - 2)[:n_peers] + 1]  # ids 0 and n_ids - 1 have no row
        self.peer_rows = np.full(n_ids, PEER_NONE, np.uint32)
        for r, i in enumerate(self.ids):
            self.peer_rows[i] = r
        self.table, self.claim = ep.table(n_peers)
        self.timers = tm.timers_table(n_peers)
        self.ref = [ref.Peer() for _ in range(n_peers)]

    def want_table(self) -> np.ndarray:
        return ep_rows([p.val for p in self.ref])

    def check(self):
        """The tables are what the restatement holds; clearSrcOnTx is the flag wherever a peer has an endpoint."""
        assert self.table.tobytes() == self.want_table().tobytes()
        assert not self.claim.any()
        for r, p in enumerate(self.ref):
            if p.val is not None:
                assert bool(int(self.timers["flags"][r]) & CLEAR_SRC) == p.clear_src_on_tx, r

    # ---- the three set calls: C arrays and the restatement's turns
    def groups(self, rows):
        """WRITE_GROUP_DTYPE rows from (peer id, tail) pairs; tail -1 is an unused row."""
        g = np.zeros(len(rows), WRITE_GROUP_DTYPE)
        for c, (peer, tail) in enumerate(rows):
            g[c] = (peer, tail, 0, 1 if tail >= 0 else 0, 0)
        return g

    def ref_set(self, picks, endpoints):
        """SetEndpointFromPacket in row order: picks are (peer row or None, source row)."""
        for row, src in picks:
            if row is not None and 0 <= src < len(endpoints) and endpoints[src] is not None:
                self.ref[row].set_endpoint_from_packet(endpoints[src])

    def row_of_id(self, peer: int):
        r = int(self.peer_rows[peer]) if peer < self.n_ids else PEER_NONE
        return r if r < self.n_peers else None

    def ref_mark(self, rows):
        for r in rows:
            self.ref[r].mark_endpoint_src_for_clearing()

    def ref_send(self, row, bufs=()):
        """Peer.Send of the restatement as (dst row, v6, status)."""
        if row is None:
            return ep_row(None), 0, 0
        got = self.ref[row].send(bufs)
        if got == ref.ERR_NO_ENDPOINT:
            return ep_row(None), 0, ref.ERR_NO_ENDPOINT
        return ep_row(got), int(ref.is6(got[0])), 0


def finished_rows(rng, w: World, peer_rows, gates):
    """The arrays of a finish batch whose row q is a response for a handshake of peer row
    peer_rows[q] (None: an index no state answers to) with verdict gates[q]."""
    n = len(peer_rows)
    states = np.zeros(max(n, 1), noise.HS_STATE_DTYPE)
    index, msgs = {}, []
    for q, r in enumerate(peer_rows):
        local = 0x5000 + q
        if r is not None:
            states[q]["local_index"], states[q]["peer_row"], states[q]["state"] = local, r, noise.HS_STATE_ZEROED
            index[local] = q
        msgs.append(struct.pack("<III", 2, int(rng.integers(1, 2**32)), local) + rng.bytes(80))  # msg.Receiver at [8:12]
    arena, pkts = arena_of(msgs)
    hs_slots = router.session_table(list(index), list(index.values()))
    return arena, pkts, np.asarray(gates, np.int32), hs_slots, states


STATUS = {"init": HS_INITIATED, "resp": HS_RESPONDED, "finish": HS_FINISHED, "none": HS_NONE}
