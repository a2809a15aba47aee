"""peer.qus.staged restated from device/send.go at packet granularity: a
collections.deque of byte strings per peer, StagePackets (:331-350),
FlushStagedPackets (:352-361) and SendStagedPackets (:363-426) with its gate
rule (:368-374) and its nonce loop (:383-407).  Written from send.go; it shares
no code with the library's host forms, which tests/test_staged_ref.py checks
against it.

What the restatement adds to the Go text is only what a fixed table needs to be
compared with: the ring position a packet lands on (the queue is a channel in
Go, a ring of `cap` slots here: the oldest packet sits at `head`, and a new one
goes behind the newest), and the batch budget of the release call."""
from collections import deque
from dataclasses import dataclass, field

import numpy as np

REJECT_AFTER_TIME_NS = 180 * 10**9  # constants.go:26
ERR_KEY_EXPIRED, ERR_BATCH_FULL = -26, -14
HS_NONE, RELEASED = 0, 11
NONE, EVICTED = 0xFFFFFFFF, 0xFFFFFFFE
NO_KEY = 0xFFFFFFFF
PEER_NONE = 0xFFFFFFFF
WANT_NO_KEYPAIR, WANT_REJECT_MESSAGES, WANT_REJECT_TIME = 0x01, 0x02, 0x04
KEYPAIR_SET = 0x1
ACT_FLUSH_STAGED = 0x80


@dataclass
class Packet:
    data: bytes
    tag: tuple = ()   # (call, slot q) of the stage call that brought it
    pos: int = 0      # its ring position


@dataclass
class Peer:
    staged: deque = field(default_factory=deque)
    head: int = 0
    lost: int = 0  # PutQuOutItems, counted


class Queues:
    def __init__(self, n_peers: int, cap: int, stride: int):
        self.peers = [Peer() for _ in range(n_peers)]
        self.cap, self.stride, self.calls = cap, stride, 0

    # ---- StagePackets, send.go:331-350, one packet
    def stage_packet(self, r: int, pkt: Packet) -> None:
        p = self.peers[r]
        while True:
            if len(p.staged) < self.cap:  # case peer.qus.staged <- items
                pkt.pos = (p.head + len(p.staged)) % self.cap
                p.staged.append(pkt)
                return
            if p.staged:  # case tooOld := <-peer.qus.staged
                p.staged.popleft()
                p.head = (p.head + 1) % self.cap
                p.lost = (p.lost + 1) & 0xFFFFFFFF

    def fits(self, size: int) -> bool:
        return size >= 0 and 16 + size + 32 <= self.stride

    def stage(self, arena, sizes, peer, count, status_in, status_out, job_key, max_segs, peer_rows):
        """The jobs the gate refused or send-assign dropped, in job order, each
        packet staged on its own.  Returns d_where."""
        self.calls += 1
        n_jobs, n_peers = len(count), len(self.peers)
        where = np.full(n_jobs * max_segs, NONE, np.uint32)
        staged = []
        for j in range(n_jobs):
            if status_in[j] != 0 or not 1 <= count[j] <= max_segs:
                continue
            pid = int(peer[j * max_segs])
            r = int(peer_rows[pid]) if pid < len(peer_rows) else PEER_NONE
            if r >= n_peers:
                continue
            refused = status_out[j] == ERR_KEY_EXPIRED
            dropped = status_out[j] == 0 and job_key[j] == NO_KEY
            if not (refused or dropped):
                continue
            for q in range(j * max_segs, j * max_segs + int(count[j])):
                size = int(sizes[q])
                if not self.fits(size):
                    continue
                o = q * self.stride + 16
                pkt = Packet(bytes(arena[o:o + size]), (self.calls, q))
                self.stage_packet(r, pkt)
                staged.append((r, pkt))
        for r, pkt in staged:
            alive = any(x is pkt for x in self.peers[r].staged)
            where[pkt.tag[1]] = r * self.cap + pkt.pos if alive else EVICTED
        return where

    # ---- FlushStagedPackets, send.go:352-361
    def flush(self, actions=None) -> None:
        for r, p in enumerate(self.peers):
            if actions is not None and not actions[r] & ACT_FLUSH_STAGED:
                continue
            while p.staged:
                p.staged.popleft()
                p.lost = (p.lost + 1) & 0xFFFFFFFF
            p.head = 0

    # ---- SendStagedPackets, send.go:363-374: the gate
    @staticmethod
    def gate(cur, now, send_nonce, limit) -> int:
        """The reasons of :369-371, 0 for a keypair that may send.  cur is the
        peer's KEYPAIR_REF_DTYPE row."""
        if not cur["flags"] & KEYPAIR_SET:
            return WANT_NO_KEYPAIR
        key = int(cur["send_key"])
        if key >= len(send_nonce):
            return 0
        w = 0
        if int(send_nonce[key]) >= limit:
            w |= WANT_REJECT_MESSAGES
        if now - int(cur["created_ns"]) >= REJECT_AFTER_TIME_NS:
            w |= WANT_REJECT_TIME
        return w

    def release(self, now, table_peer, kp, send_nonce, limit, n_out_max):
        """SendStagedPackets over the peer rows up to the nonce loop, under the
        batch budget.  Returns (status per row, want bits per row, the jobs
        [(peer id, bytes)] in order)."""
        status, want, jobs, below = [], [], [], 0
        for r, p in enumerate(self.peers):
            w = 0
            if not p.staged:  # :365
                status.append(HS_NONE)
            elif (w := self.gate(kp["current"][r], now, send_nonce, limit)):  # :369-373
                status.append(ERR_KEY_EXPIRED)
            else:
                n = len(p.staged)
                if below + n <= n_out_max:
                    while p.staged:  # case items := <-peer.qus.staged
                        jobs.append((int(table_peer[r]), p.staged.popleft().data))
                    p.head = 0
                    status.append(RELEASED)
                else:
                    status.append(ERR_BATCH_FULL)
                below += n
            want.append(w)
        return status, want, jobs

    # ---- SendStagedPackets whole, send.go:363-426, for one peer: gate, nonce loop, re-staging
    def send_staged(self, r, now, cur, send_nonce, limit):
        """Returns (reasons a handshake is wanted, [(nonce, bytes)] that went on
        to encryption).  The staged packets are taken as one item list."""
        p, sent = self.peers[r], []
        while True:  # top:
            if not p.staged:
                return 0, sent
            w = self.gate(cur, now, send_nonce, limit)
            if w:
                return w, sent
            key = int(cur["send_key"])
            items = [p.staged.popleft() for _ in range(len(p.staged))]
            p.head = 0
            out_of_order, kept = [], []
            for item in items:
                nonce = int(send_nonce[key])  # sendNonce.Add(1) - 1
                send_nonce[key] = nonce + 1
                if nonce >= limit:  # :385
                    send_nonce[key] = limit
                    out_of_order.append(item)
                    continue
                kept.append((nonce, item.data))
            self.calls += 1
            for item in out_of_order:  # :402-407
                self.stage_packet(r, item)
            sent += kept
            if not out_of_order:
                return 0, sent
            # goto top

    # ---- what a table of rings is compared with
    def lens(self):
        return [len(p.staged) for p in self.peers]

    def heads(self):
        return [p.head for p in self.peers]

    def losts(self):
        return [p.lost for p in self.peers]

    def entries(self, r):
        return [x.data for x in self.peers[r].staged]
