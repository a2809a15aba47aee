"""Worlds and batches for the cookie-generator tests (test infrastructure only),
shared by tests/test_cookiegen_ref.py, tests/test_cookiegen_host.py and
tests/test_gpu_cookiegen.py.

A World is one device's tables as the calls of wireguard_amd/cookiegen.py take
them, built beside the restatement's view of the same state: one
cookiegen_ref.CookieGenerator per peer row and the {index: peer row} dict that
d.indexTable.Lookup stands for.  Nothing here calls the code under test but
`gen_build`, which tests/test_cookiegen_ref.py pins first.
"""
from __future__ import annotations

import struct

import numpy as np

import cookiegen_ref as ref
from wireguard_amd import cookie, cookiegen as cg, noise, router
from wireguard_amd._lib import HS_INITIATED, HS_PEER_COOKIE, HS_PEER_SEEN, HS_RESPONDED, PEER_NONE, SESSION_NO_KEYPAIR
from wireguard_amd.transport import AEAD_PKT_DTYPE

SECOND = 10**9
REFRESH = ref.COOKIE_REFRESH_NS
SENTINEL = 0xA5


class World:
    """n_peers peers with ids 7, 10, 13, ...; indices are added with the four
    add_* calls and the tables built by finish()."""

    def __init__(self, rng: np.random.Generator, n_peers: int = 5, n_states: int = 8, n_keys: int = 12):
        self.rng, self.n_peers, self.n_states, self.n_keys = rng, n_peers, n_states, n_keys
        self.pubs = [rng.bytes(32) for _ in range(n_peers)]
        self.ids = [7 + 3 * r for r in range(n_peers)]
        self.table = np.zeros(n_peers, noise.PEER_KEY_DTYPE)
        for r in range(n_peers):
            self.table["public_key"][r] = np.frombuffer(self.pubs[r], np.uint8)
        self.table["peer"] = self.ids
        self.peer_rows = noise.peer_rows_build(self.table, max(self.ids, default=0) + 3)
        self.gen = cg.gen_build(self.table)
        self.peers = np.zeros(n_peers, noise.HS_PEER_DTYPE)
        self.peers["claim"] = noise.HS_CLAIM_NONE
        self.peers["flags"][::2] = HS_PEER_SEEN  # a bit the calls must leave alone
        self.peers["last_consumption_ns"] = 77
        self.states = np.zeros(n_states, noise.HS_STATE_DTYPE)
        self.states["claim"] = 0xFFFFFFFF
        self.key_peer = np.full(n_keys, PEER_NONE, np.uint32)
        self._hs, self._kp = {}, {}  # index -> state row; index -> key
        self.index_table: dict[int, int] = {}  # the restatement's: index -> peer row
        self.ref = [ref.CookieGenerator(pk) for pk in self.pubs]
        self.valid = [False] * n_peers  # WGCS_HS_PEER_COOKIE as the calls leave it
        self.hs_slots = self.slots = None

    # ---- indices
    def add_handshake(self, index: int, state_row: int, peer_row: int, state: int = noise.HS_STATE_INITIATED) -> None:
        """A handshake we initiated: hs_slots index -> state_row, whose row holds index and peer_row."""
        self._hs[index] = state_row
        self.states[state_row]["local_index"], self.states[state_row]["peer_row"] = index, peer_row
        self.states[state_row]["state"] = state
        if peer_row < self.n_peers:
            self.index_table[index] = peer_row

    def add_stale_handshake(self, index: int, state_row: int) -> None:
        """hs_slots still lists index, but its state row was reused under another index."""
        self._hs[index] = state_row
        assert int(self.states[state_row]["local_index"]) != index

    def add_keypair(self, index: int, key: int, peer_id: int) -> None:
        """A response we sent: slots index -> key, key_peer[key] = peer_id."""
        self._kp[index] = key
        if key < self.n_keys:
            self.key_peer[key] = peer_id
            if peer_id < len(self.peer_rows) and int(self.peer_rows[peer_id]) < self.n_peers:
                self.index_table[index] = int(self.peer_rows[peer_id])

    def add_no_keypair(self, index: int) -> None:
        """NewIndex was called, no keypair yet: WGCS_SESSION_NO_KEYPAIR."""
        self._kp[index] = SESSION_NO_KEYPAIR

    def finish(self) -> "World":
        self.hs_slots = router.session_table(list(self._hs), list(self._hs.values()))
        self.slots = router.session_table(list(self._kp), list(self._kp.values()))
        return self

    # ---- what the tables should hold, from the restatement
    def want_gen(self) -> np.ndarray:
        g = np.zeros(self.n_peers, cg.COOKIE_GEN_DTYPE)
        for r, c in enumerate(self.ref):
            g["cookie_key"][r] = np.frombuffer(c.encryption_key, np.uint8)
            g["last_mac1"][r] = np.frombuffer(c.last_mac1, np.uint8)
            g["cookie_set_at_ns"][r] = c.cookie_set_at or 0
            g["flags"][r] = 1 if c.has_last_mac1 else 0
        return g

    def want_peers(self, before: np.ndarray) -> np.ndarray:
        """`before` with the restatement's cookie and the valid bit."""
        p = before.copy()
        for r, c in enumerate(self.ref):
            p["cookie"][r] = np.frombuffer(c.cookie, np.uint8)
            p["flags"][r] = (int(before["flags"][r]) & ~HS_PEER_COOKIE) | (HS_PEER_COOKIE if self.valid[r] else 0)
        return p

    # ---- the restatement's side of the five calls
    def ref_sent(self, peer_row, status, want_status: int, mac1s) -> None:
        for j in range(len(status)):  # the descriptors in order
            if int(status[j]) == want_status and int(peer_row[j]) < self.n_peers:
                self.ref[int(peer_row[j])].sent(bytes(mac1s[j]))

    def ref_consume(self, rows, now: int) -> np.ndarray:
        """rows: (type, message bytes) in order; the verdicts."""
        out = []
        for type_, msg in rows:
            v = ref.receive_cookie_reply(type_, msg if type_ == 3 else None, self.index_table, self.ref, now)
            if v == ref.HS_COOKIE_KEPT:
                self.valid[self.index_table[struct.unpack_from("<I", msg, 4)[0]]] = True
            out.append(v)
        return np.array(out, np.int32)

    def ref_age(self, now: int) -> None:
        for r, c in enumerate(self.ref):
            if self.valid[r] and c.cookie_for(now) is None:
                self.valid[r] = False

    # ---- messages
    def reply(self, receiver: int, peer_row: int, cookie_bytes: bytes | None = None, mac1: bytes | None = None,
              fast: bool = False) -> bytes:
        """The reply peer_row's responder sends to `receiver` for a message with
        `mac1` (default: the last one sent to that peer).  fast: sealed by the
        library's CreateReply (pinned by tests/test_cookie_ref.py), for bulk."""
        c = self.ref[peer_row]
        mac1 = c.last_mac1 if mac1 is None else mac1
        nonce = self.rng.bytes(24)
        if not fast:
            return ref.seal_reply(c.encryption_key, receiver, nonce, self.rng.bytes(16) if cookie_bytes is None else cookie_bytes, mac1)
        assert cookie_bytes is None
        checker = cookie.checker_init(self.pubs[peer_row], secret=self.rng.bytes(32))
        msg = struct.pack("<II", 1, receiver) + bytes(108) + mac1 + bytes(16)
        return cookie.create_reply(checker, msg, cookie.src_addr("10.0.0.1", 9), nonce)


def sent_arrays(rng, kind: str, peer_row, status):
    """(descriptors, status, msgs, the MAC1 of every row) of an initiate ("init") or
    respond ("resp") batch with random message bytes: only the MAC1 field is read."""
    n = len(peer_row)
    dtype, pitch, at = ((noise.HS_START_DTYPE, noise.INITIATION_PITCH, 116) if kind == "init"
                        else (noise.HS_RESP_DTYPE, noise.RESPONSE_PITCH, 60))
    d = np.zeros(n, dtype)
    d["peer_row"] = peer_row
    d["local_index"] = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    msgs = rng.integers(0, 256, (n, pitch), dtype=np.uint8)
    return d, np.asarray(status, np.int32), msgs.reshape(-1), [msgs[j, at:at + 16].tobytes() for j in range(n)]


def sent_status(kind: str) -> int:
    return HS_INITIATED if kind == "init" else HS_RESPONDED


def arena_of(msgs, tail: int = 8):
    """(arena, pkts): message q at an offset that is q mod 4 past a multiple of 4,
    in an arena filled with SENTINEL that ends `tail` bytes after the last message."""
    off, at = [], 0
    for q, m in enumerate(msgs):
        at = (at + 3) // 4 * 4 + q % 4
        off.append(at)
        at += len(m) + 5
    size = (off[-1] + len(msgs[-1]) + tail) if msgs else tail
    arena = np.full(size, SENTINEL, np.uint8)
    pkts = np.zeros(len(msgs), AEAD_PKT_DTYPE)
    for q, m in enumerate(msgs):
        arena[off[q]:off[q] + len(m)] = np.frombuffer(m, np.uint8)
        pkts["off"][q], pkts["len"][q] = off[q], len(m)
    pkts["key"] = PEER_NONE
    return arena, pkts


def lookup_world(rng) -> World:
    """Five peers and every kind of index the lookup cases name."""
    w = World(rng)
    w.add_handshake(0x1001, 2, 0)
    w.add_handshake(0x1002, 5, 3)
    w.add_handshake(0x1003, 7, 4, state=noise.HS_STATE_ZEROED)  # "in whatever state"
    w.add_handshake(0x1004, 1, 9)          # a state row whose peer_row is past the table
    w.add_handshake(0x2002, 3, 1)          # row 3 reused: it now answers to 0x2002 ...
    w.add_stale_handshake(0x2001, 3)       # ... and 0x2001 still points at it
    w.add_keypair(0x3001, 4, w.ids[2])
    w.add_keypair(0x3002, 11, w.ids[1])
    w.add_keypair(0x3003, 6, 2)            # an id no peer row has
    w.add_keypair(0x3004, 40, w.ids[0])    # a key past the table
    w.add_no_keypair(0x4001)
    return w.finish()


UNKNOWN = 0x5555  # an index nothing lists
