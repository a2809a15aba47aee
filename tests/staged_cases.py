"""Worlds, job tables and call sequences for the staged queue, shared by
tests/test_staged_ref.py (the host forms against tests/staged_ref.py) and
tests/test_gpu_staged.py (the device calls against the host forms).

A case is a function of a driver.  The driver owns two implementations, runs
every call on both, compares everything they write and hands back the host
side's outputs; the cases add what each call must have done.  A driver has
  .w                          the World (tables the calls read; release updates its rekey rows)
  .stage(jobs) -> where
  .release(now, n_out_max) -> Out
  .flush(actions)
  .st                         the host forms' state (staged.State) after the last call"""
from dataclasses import dataclass

import numpy as np

from replay_ref import send_assign_ref
from wireguard_amd import keypairs, rekey, staged
from wireguard_amd._lib import (ERR_BATCH_FULL, ERR_KEY_EXPIRED, HS_NONE, KEYPAIR_INITIATOR, KEYPAIR_SET, PEER_NONE,
                                REJECT_AFTER_TIME_NS, REKEY_WANT_NO_KEYPAIR, REKEY_WANT_REJECT_MESSAGES,
                                REKEY_WANT_REJECT_TIME, STAGED_EVICTED, STAGED_NONE, STAGED_RELEASED,
                                TIMERS_ACT_FLUSH_STAGED)
from wireguard_amd.noise import PEER_KEY_DTYPE

STRIDE = 128          # the largest packet a slot holds is 80 bytes
LARGEST = STRIDE - 48
SENTINEL = 0xA5       # what rings, arenas and job tables hold where nothing was written
SECOND = 10**9
NOW = 5000 * SECOND
LIMIT = 1000          # RejectAfterMessages of these worlds: small, so that sequences reach it
NO_KEY = 0xFFFFFFFF


@dataclass
class World:
    n_peers: int
    cap: int
    stride: int
    ids: np.ndarray        # peer id of row r
    table: np.ndarray      # PEER_KEY_DTYPE
    peer_rows: np.ndarray  # id -> row
    kp: np.ndarray
    nonce: np.ndarray      # uint64 per key row; row r owns key rows 2r and 2r + 1
    rekey: np.ndarray
    limit: int = LIMIT

    def set_current(self, r, created, nonce=0):
        """A fresh current keypair for row r, as wgcs_keypairs_begin_* leave one: the key row it did not use last."""
        old = self.kp["current"][r]
        key = 2 * r + (1 if (old["flags"] & KEYPAIR_SET and old["send_key"] == 2 * r) else 0)
        self.kp["previous"][r] = old
        self.kp["current"][r] = (key, key, 0x1000 + key, KEYPAIR_SET | KEYPAIR_INITIATOR, created)
        self.nonce[key] = nonce

    def clear_current(self, r):
        self.kp["current"][r] = (0, 0, 0, 0, 0)

    def peer_key(self):
        """peer id -> the key row send-assign finds: current's send key"""
        cur = self.kp["current"]
        return {int(self.ids[r]): int(cur["send_key"][r]) for r in range(self.n_peers) if cur["flags"][r] & KEYPAIR_SET}


def world(rng, n_peers, cap, stride=STRIDE, limit=LIMIT) -> World:
    ids = (rng.permutation(n_peers + 4)[:n_peers] + 3).astype(np.uint32)
    table = np.zeros(n_peers, PEER_KEY_DTYPE)
    table["public_key"] = rng.integers(0, 256, (n_peers, 32), dtype=np.uint8)
    table["peer"], table["flags"] = ids, 1
    peer_rows = np.full(n_peers + 9, PEER_NONE, np.uint32)
    peer_rows[ids] = np.arange(n_peers, dtype=np.uint32)
    if n_peers:
        peer_rows[-1] = n_peers  # an id whose row lies past the table
    return World(n_peers, cap, stride, ids, table, peer_rows, keypairs.keypairs_table(n_peers),
                 np.zeros(2 * n_peers + 1, np.uint64), rekey.rekey_table(n_peers, NOW), limit)


@dataclass
class Jobs:
    arena: np.ndarray
    sizes: np.ndarray
    peer: np.ndarray
    count: np.ndarray
    status_in: np.ndarray
    status_out: np.ndarray
    job_key: np.ndarray
    max_segs: int

    def packet(self, q):
        o = q * (len(self.arena) // len(self.sizes)) + 16
        return self.arena[o:o + int(self.sizes[q])].tobytes()


def jobs(rng, w: World, spec, max_segs, status_out=None, job_key=None) -> Jobs:
    """spec: one (peer id, [segment sizes], status_in[, count]) per job.  The
    arena's last slot ends where the array ends."""
    n = len(spec)
    arena = np.full(n * max_segs * w.stride, SENTINEL, np.uint8)
    sizes = np.full(n * max_segs, 0x55AA55, np.int32)  # an unused slot's size is never read
    peer = np.full(n * max_segs, PEER_NONE, np.uint32)
    count, status_in = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for j, row in enumerate(spec):
        pid, segs, st = row[:3]
        count[j], status_in[j] = (row[3] if len(row) > 3 else len(segs)), st
        peer[j * max_segs:(j + 1) * max_segs] = pid
        for k, size in enumerate(segs[:max_segs]):
            q = j * max_segs + k
            sizes[q] = size
            if 0 <= size <= w.stride - 16:
                arena[q * w.stride + 16:q * w.stride + 16 + size] = rng.integers(0, 256, size, dtype=np.uint8)
    jb = Jobs(arena, sizes, peer, count, status_in, np.zeros(n, np.int32), np.full(n, NO_KEY, np.uint32), max_segs)
    if status_out is not None:
        jb.status_out[:], jb.job_key[:] = status_out, job_key
    return jb


def front(w: World, jb: Jobs, now) -> Jobs:
    """send gate -> send-assign -> sent over jb on the world's tables: what the stage call finds."""
    n = len(jb.count)
    if n == 0:
        return jb
    rekey.send_gate_host(jb.peer, jb.count, jb.status_in, jb.max_segs, now, w.peer_rows, w.kp, w.nonce, w.limit, w.rekey,
                         jb.status_out)
    _, _, jb.job_key, w.nonce = send_assign_ref(jb.sizes, jb.peer, jb.count, jb.status_out, jb.max_segs, w.stride,
                                                w.peer_key(), w.nonce, w.limit)
    rekey.sent_host(jb.peer, jb.count, jb.status_out, jb.job_key, jb.max_segs, now, w.peer_rows, w.kp, w.nonce, w.limit,
                    w.rekey)
    return jb


def refused(rng, w, spec, max_segs=1) -> Jobs:
    """jobs that the gate refused, whatever the keypairs say"""
    jb = jobs(rng, w, spec, max_segs)
    jb.status_out[:] = np.where(jb.status_in == 0, ERR_KEY_EXPIRED, jb.status_in)
    return jb


@dataclass
class Out:
    status: np.ndarray
    out: np.ndarray
    peer: np.ndarray
    count: np.ndarray
    sizes: np.ndarray
    out_status: np.ndarray
    n_out: int

    def packets(self, stride):
        return [(int(self.peer[k]), self.out[k * stride + 16:k * stride + 16 + int(self.sizes[k])].tobytes())
                for k in range(self.n_out)]

    def as_jobs(self) -> Jobs:
        n = len(self.count)
        return Jobs(self.out.copy(), self.sizes.copy(), self.peer.copy(), self.count.copy(), self.out_status.copy(),
                    np.zeros(n, np.int32), np.full(n, NO_KEY, np.uint32), 1)


class HostSide:
    """the library's host forms on a state of their own"""

    def __init__(self, w: World):
        self.w, self.st = w, staged.state(w.n_peers, w.cap, w.stride, fill=SENTINEL)

    def stage(self, jb: Jobs):
        where = np.full(len(jb.sizes), 0x77777777, np.uint32)
        staged.stage_host(jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key, jb.max_segs,
                          self.w.peer_rows, self.st, where)
        return where

    def release(self, now, n_out_max, rk):
        m = n_out_max
        o = Out(np.full(self.w.n_peers, 0x77, np.int32), np.full(m * self.w.stride, SENTINEL, np.uint8),
                np.full(m, 0x77, np.uint32), np.full(m, 0x77, np.int32), np.full(m, 0x77, np.int32),
                np.full(m, 0x77, np.int32), 0)
        n_out = np.full(1, 0x77, np.uint32)
        staged.release_host(now, self.w.table, self.w.kp, self.w.nonce, self.w.limit, rk, self.st, m, o.out, o.peer, o.count,
                            o.sizes, o.out_status, n_out, o.status)
        o.n_out = int(n_out[0])
        return o

    def flush(self, actions):
        staged.flush_host(actions, self.st)


def live_state(st):
    """(len, head, lost, every peer's entries, the size word of every live slot)"""
    n = st.n_peers
    ln, hd = np.asarray(st.len).view(np.uint32), np.asarray(st.head).view(np.uint32)
    sizes = np.asarray(st.slot_size).view(np.int32)
    live = [[int(sizes[r * st.cap + ((int(hd[r]) + i) & (st.cap - 1))]) for i in range(int(ln[r]))] for r in range(n)]
    return ln.tolist(), hd.tolist(), np.asarray(st.lost).view(np.uint32).tolist(), [staged.entries(st, r) for r in range(n)], live


# ------------------------------------------------------------------ the cases
def stage_fill_and_evict(d, rng):
    """fill to exactly cap; cap + 1: the oldest goes and lost == 1"""
    w = d.w
    pid, cap = int(w.ids[0]), w.cap
    jb = refused(rng, w, [(pid, [20 + k], 0) for k in range(cap)])
    where = d.stage(jb)
    assert where.tolist() == list(range(cap))
    assert d.st.len[0] == cap and d.st.head[0] == 0 and d.st.lost[0] == 0
    first = [jb.packet(q) for q in range(cap)]
    assert staged.entries(d.st, 0) == first
    one = refused(rng, w, [(pid, [33], 0)])
    assert d.stage(one).tolist() == [0]  # the oldest packet's slot
    assert d.st.len[0] == cap and d.st.head[0] == 1 % cap and d.st.lost[0] == 1
    assert staged.entries(d.st, 0) == first[1:] + [one.packet(0)]


def stage_more_than_cap(d, rng):
    """m > cap in one call, on an empty and then on a full ring: only the last cap remain"""
    w = d.w
    pid, cap = int(w.ids[1]), w.cap
    for lost_before, extra in ((0, 3), (3, 2 * cap + 1)):
        m = cap + extra
        jb = refused(rng, w, [(pid, [10 + (k % 50)], 0) for k in range(m)])
        L = int(d.st.len[1])
        where = d.stage(jb)
        assert (where[:extra] == STAGED_EVICTED).all() and (where[extra:] < STAGED_EVICTED).all()
        assert len(set(where[extra:].tolist())) == cap
        assert staged.entries(d.st, 1) == [jb.packet(q) for q in range(extra, m)]
        assert d.st.len[1] == cap and d.st.lost[1] == lost_before + L + m - cap


def stage_straddle_and_wrap(d, rng):
    """a 3-segment job that straddles the wrap; the head wraps past cap twice"""
    w = d.w
    pid, cap = int(w.ids[0]), w.cap
    lead = max(cap - 2, 0)
    if lead:
        d.stage(refused(rng, w, [(pid, [12], 0) for _ in range(lead)]))
    jb = refused(rng, w, [(pid, [40, 41, 42], 0)], max_segs=4)
    where = d.stage(jb)
    assert where[3] == STAGED_NONE
    if cap >= 4:
        assert where[:3].tolist() == [cap - 2, cap - 1, 0] and d.st.head[0] == 1 and d.st.lost[0] == 1
        assert staged.entries(d.st, 0)[-3:] == [jb.packet(q) for q in range(3)]
    total = lead + 3
    for _ in range(2 * cap + 1):  # one by one: the head goes round twice
        one = refused(rng, w, [(pid, [7], 0)])
        d.stage(one)
        total += 1
        assert staged.entries(d.st, 0)[-1] == one.packet(0)
        assert d.st.head[0] == max(total - cap, 0) % cap and d.st.lost[0] == max(total - cap, 0)


def stage_what_is_passed_by(d, rng):
    """a keepalive, sizes around a row, the largest that fits and one more, a peer without a row,
    a job with a status, counts out of range, jobs that were sent"""
    w = d.w
    a, b = int(w.ids[0]), int(w.ids[-1])
    no_row, past = int(len(w.peer_rows) - 2), int(len(w.peer_rows) - 1)
    spec = [(a, [0], 0), (b, [1, 15, 16], 0), (a, [17, LARGEST, LARGEST + 1], 0), (no_row, [30], 0), (past, [30], 0),
            (10**6, [30], 0), (a, [30], -3), (b, [30, 30], 0, 0), (b, [30, 30], 0, 4), (a, [-1, 31, -8], 0),
            (b, [32], 0), (a, [34], 0), (PEER_NONE, [30], 0)]
    jb = refused(rng, w, spec, max_segs=3)
    jb.status_out[10], jb.job_key[10] = 0, 7         # sent under key row 7
    jb.status_out[11], jb.job_key[11] = 0, NO_KEY    # dropped by send-assign
    where = d.stage(jb).reshape(-1, 3)
    staged_q = {(0, 0), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (9, 1), (11, 0)}
    for j in range(len(spec)):
        for k in range(3):
            assert (where[j, k] != STAGED_NONE) == ((j, k) in staged_q), (j, k)
    rows = {a: 0, b: w.n_peers - 1}
    for pid in {a, b}:
        want = [jb.packet(j * 3 + k) for j, k in sorted(staged_q) if spec[j][0] == pid]
        assert staged.entries(d.st, rows[pid])[-len(want):] == want[-w.cap:]


def release_rules(d, rng):
    """current nil; nonce at limit and one below; age at RejectAfterTime and one nanosecond less"""
    w = d.w
    assert w.n_peers >= 6
    now = NOW
    for r in range(6):
        d.stage(refused(rng, w, [(int(w.ids[r]), [24 + r], 0)]))
    w.set_current(1, now, nonce=w.limit)
    w.set_current(2, now, nonce=w.limit - 1)
    w.set_current(3, now - REJECT_AFTER_TIME_NS)
    w.set_current(4, now - REJECT_AFTER_TIME_NS + 1)
    w.set_current(5, now - REJECT_AFTER_TIME_NS, nonce=w.limit)
    before = w.rekey["want"].copy()
    o = d.release(now, 64)
    assert o.status[:6].tolist() == [ERR_KEY_EXPIRED, ERR_KEY_EXPIRED, STAGED_RELEASED, ERR_KEY_EXPIRED, STAGED_RELEASED,
                                     ERR_KEY_EXPIRED]
    assert (o.status[6:] == HS_NONE).all() and o.n_out == 2
    got = (w.rekey["want"] ^ before)[:6].tolist()
    assert got == [REKEY_WANT_NO_KEYPAIR, REKEY_WANT_REJECT_MESSAGES, 0, REKEY_WANT_REJECT_TIME, 0,
                   REKEY_WANT_REJECT_MESSAGES | REKEY_WANT_REJECT_TIME]
    assert [p for p, _ in o.packets(w.stride)] == [int(w.ids[2]), int(w.ids[4])]
    assert d.st.len[:6].tolist() == [1, 1, 0, 1, 0, 1]
    assert o.peer[2:].tolist() == [PEER_NONE] * 62 and not o.count[2:].any() and o.count[:2].tolist() == [1, 1]


def release_budget(d, rng):
    """budget exactly the sum and one less; a deferred row followed by a small one, deferred too"""
    w = d.w
    assert w.n_peers >= 4 and w.cap >= 4
    now = NOW
    lens = [3, 4, 1, 2]
    for r, n in enumerate(lens):
        w.set_current(r, now)
        d.stage(refused(rng, w, [(int(w.ids[r]), [16 + r], 0) for _ in range(n)]))
    o = d.release(now, 6)  # 3 fit, 4 do not: and then neither does the 1 that would
    assert o.status[:4].tolist() == [STAGED_RELEASED, ERR_BATCH_FULL, ERR_BATCH_FULL, ERR_BATCH_FULL] and o.n_out == 3
    assert d.st.len[:4].tolist() == [0, 4, 1, 2]
    o = d.release(now, 6)  # 4 + 1 + 2 is one too many
    assert o.status[:4].tolist() == [HS_NONE, STAGED_RELEASED, STAGED_RELEASED, ERR_BATCH_FULL] and o.n_out == 5
    assert o.peer[5] == PEER_NONE and d.st.len[:4].tolist() == [0, 0, 0, 2]
    d.stage(refused(rng, w, [(int(w.ids[0]), [50], 0)]))
    o = d.release(now, 3)  # exactly the sum
    assert o.status[:4].tolist() == [STAGED_RELEASED, HS_NONE, HS_NONE, STAGED_RELEASED] and o.n_out == 3
    assert not d.st.len.any() and not d.st.head.any()
    o = d.release(now, 0)
    assert o.n_out == 0 and not o.status.any()


def nonce_limit_residue(d, rng):
    """release -> send-assign with the nonce three below the limit and five packets -> stage again:
    the queue then holds the last two, in order"""
    w = d.w
    pid, now = int(w.ids[0]), NOW
    five = refused(rng, w, [(pid, [20 + k], 0) for k in range(5)])
    d.stage(five)
    w.set_current(0, now, nonce=w.limit - 3)
    key = int(w.kp["current"]["send_key"][0])
    o = d.release(now, 8)
    assert o.n_out == 5 and o.status[0] == STAGED_RELEASED and not d.st.len[0]
    jb = front(w, o.as_jobs(), now)
    assert jb.job_key.tolist() == [key] * 3 + [NO_KEY] * 5 and w.nonce[key] == w.limit
    where = d.stage(jb)
    assert where.tolist() == [STAGED_NONE] * 3 + [0, 1] + [STAGED_NONE] * 3
    assert staged.entries(d.st, 0) == [five.packet(3), five.packet(4)]
    assert w.rekey["want"][0] & REKEY_WANT_REJECT_MESSAGES
    assert d.release(now, 8).status[0] == ERR_KEY_EXPIRED


def flush_rows(d, rng):
    """flush with and without d_actions"""
    w = d.w
    for r in range(w.n_peers):
        d.stage(refused(rng, w, [(int(w.ids[r]), [9], 0) for _ in range(r % 3 + 1)]))
    actions = np.array([(TIMERS_ACT_FLUSH_STAGED | 0x3) if r % 2 else 0x17F for r in range(w.n_peers)], np.uint32)
    d.flush(actions)
    assert d.st.len.tolist() == [0 if r % 2 else r % 3 + 1 for r in range(w.n_peers)]
    assert d.st.lost.tolist() == [r % 3 + 1 if r % 2 else 0 for r in range(w.n_peers)]
    d.flush(None)
    assert not d.st.len.any() and not d.st.head.any() and d.st.lost.tolist() == [r % 3 + 1 for r in range(w.n_peers)]


CASES = [(stage_fill_and_evict, 3, c) for c in (1, 4, 8)] + [(stage_more_than_cap, 3, c) for c in (1, 4, 8)] + \
        [(stage_straddle_and_wrap, 2, c) for c in (1, 4, 8)] + [(stage_what_is_passed_by, 3, c) for c in (1, 4, 8)] + \
        [(release_rules, 7, 4), (release_budget, 5, 4), (nonce_limit_residue, 2, 8), (flush_rows, 9, 4)]


def random_sequence(d, seed):
    """The three calls mixed with the gate, send-assign, new keypairs and the clock."""
    rng = np.random.default_rng(seed)
    w = d.w
    cap, now = w.cap, NOW
    released = staged_total = 0
    for r in range(w.n_peers):  # half of the peers begin with a session
        if rng.random() < 0.5:
            w.set_current(r, now - int(rng.integers(0, REJECT_AFTER_TIME_NS)), nonce=int(rng.choice([0, w.limit - 5])))
    for _ in range(int(rng.integers(6, 14))):
        op = rng.choice(["send", "send", "send", "release", "renew", "renew", "flush", "key", "clock"])
        if op == "send":
            max_segs = int(rng.choice([1, 3]))
            spec = []
            for _ in range(int(rng.integers(0, 3 * cap + 4))):
                pid = int(rng.choice(w.ids)) if w.n_peers and rng.random() < 0.9 else int(rng.integers(0, len(w.peer_rows) + 2))
                segs = [int(rng.choice([0, 1, 15, 16, 17, 40, LARGEST, LARGEST + 1, -1], p=[.1, .1, .1, .1, .1, .3, .1, .05, .05]))
                        for _ in range(int(rng.integers(1, max_segs + 1)))]
                spec.append((pid, segs, int(rng.choice([0, 0, 0, 0, -3])), int(rng.choice([len(segs)] * 8 + [0, max_segs + 1]))))
            jb = front(w, jobs(rng, w, spec, max_segs), now)
            where = d.stage(jb)
            staged_total += int((where < STAGED_EVICTED).sum())
        elif op in ("release", "renew"):
            if op == "renew":  # a handshake completes for most of the peers that wait
                for r in np.flatnonzero(d.st.len):
                    if rng.random() < 0.7:
                        w.set_current(int(r), now, nonce=int(rng.choice([0, 0, w.limit - 2])))
            o = d.release(now, int(rng.choice([0, 1, cap, 2 * cap + 1, w.n_peers * cap])))
            released += o.n_out
            d.stage(front(w, o.as_jobs(), now))  # what send-assign dropped at the nonce limit comes back
        elif op == "flush":
            d.flush(None if rng.random() < 0.2 else
                    rng.choice([0, TIMERS_ACT_FLUSH_STAGED, 0x1FF, 0x17F], w.n_peers).astype(np.uint32))
        elif op == "key" and w.n_peers:
            r = int(rng.integers(0, w.n_peers))
            if rng.random() < 0.2:
                w.clear_current(r)
            else:
                w.set_current(r, now, nonce=int(rng.choice([0, 0, w.limit - 2, w.limit])))
        else:
            now += int(rng.choice([1, SECOND, REJECT_AFTER_TIME_NS - 1, REJECT_AFTER_TIME_NS]))
    return staged_total, released


def random_world(seed):
    rng = np.random.default_rng(10_000 + seed)
    return world(rng, int(rng.integers(0, 10)), int(rng.choice([1, 4, 8])))
