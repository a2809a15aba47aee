"""Plain-Python references of the per-keypair state (test infrastructure only;
Python ints and numpy, no torch, no GPU).

  Filter            replay.Filter.Validate restated on Python ints (replay/replay.go:32-70)
  SetModel          the same verdicts from a set of seen values and a maximum
  trip_validate     the trip rule of replay_kernels.hip: any number of consecutive
                    rows of one key, all decided from the state before the trip
  replay_batch_ref  wgcs_replay_batch, sequentially in slot order
  send_assign_ref   wgcs_send_assign_batch, sequentially in job order
"""
from __future__ import annotations

import numpy as np

from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

BLOCK_SHIFT, N_BLOCKS = 6, 128
BIT_MASK, BLOCK_MASK = 63, 127
WINDOW = (N_BLOCKS - 1) * 64  # 8,128
REJECT_AFTER_MESSAGES = (1 << 64) - (1 << 13) - 1  # constants.go:14
ERR_REPLAY, ERR_PACKET_TOO_SHORT = -20, -8
NO_KEY = PEER_NONE = 0xFFFFFFFF
U64 = (1 << 64) - 1


class Filter:
    """replay.Filter: `last` and a ring of 128 blocks of 64 bits."""

    def __init__(self, last: int = 0, ring=None):
        self.last = last
        self.ring = [0] * N_BLOCKS if ring is None else [int(x) for x in ring]

    def validate(self, value: int, limit: int) -> bool:
        if value >= limit:
            return False
        block = value >> BLOCK_SHIFT
        if value > self.last:
            current = self.last >> BLOCK_SHIFT
            for i in range(current + 1, current + min(block - current, N_BLOCKS) + 1):
                self.ring[i & BLOCK_MASK] = 0
            self.last = value
        elif self.last - value > WINDOW:
            return False
        block &= BLOCK_MASK
        old = self.ring[block]
        self.ring[block] = old | 1 << (value & BIT_MASK)
        return old != self.ring[block]

    def state(self):
        return self.last, tuple(self.ring)

    def copy(self) -> "Filter":
        return Filter(self.last, self.ring)


class SetModel:
    """What the filter means: accept a value below the limit that was not
    accepted before and is no more than the window behind the highest one."""

    def __init__(self):
        self.last, self.seen = 0, set()

    def validate(self, value: int, limit: int) -> bool:
        if value >= limit:
            return False
        if value <= self.last and self.last - value > WINDOW:
            return False
        self.last = max(self.last, value)
        if value in self.seen:
            return False
        self.seen.add(value)
        return True


def trip_validate(f: Filter, values, limit: int) -> list[bool]:
    """One trip: the verdict of every row from (f.last, f.ring) as they are
    before the trip, then the state update.  Nothing here depends on a row's
    verdict or on an earlier row's update of the ring."""
    L, ring = f.last, f.ring
    ok = [v < limit for v in values]
    out = []
    m = L
    for i, v in enumerate(values):
        win = ok[i] and (v > m or m - v <= WINDOW)
        dup = any(ok[j] and values[j] == v for j in range(i))
        old = win and (v >> BLOCK_SHIFT) <= (L >> BLOCK_SHIFT) and bool(ring[(v >> 6) & BLOCK_MASK] >> (v & 63) & 1)
        out.append((win, win and not dup and not old))
        if ok[i]:
            m = max(m, v)
    new_last = m
    lb, nb = L >> BLOCK_SHIFT, new_last >> BLOCK_SHIFT
    for i in range(lb + 1, lb + min(nb - lb, N_BLOCKS) + 1):
        ring[i & BLOCK_MASK] = 0
    for (win, _), v in zip(out, values):
        if win and nb - (v >> BLOCK_SHIFT) < N_BLOCKS:
            ring[(v >> 6) & BLOCK_MASK] |= 1 << (v & 63)
    f.last = new_last
    return [a for _, a in out]


def filters_to_array(filters: list[Filter]) -> np.ndarray:
    a = np.zeros(len(filters), REPLAY_FILTER_DTYPE)
    for k, f in enumerate(filters):
        a["last"][k] = f.last
        a["ring"][k] = np.array(f.ring, np.uint64)
    return a


def filters_from_array(a: np.ndarray) -> list[Filter]:
    return [Filter(int(r["last"]), r["ring"].tolist()) for r in a]


def takes_part(key: int, pkt_len: int, n_keys: int) -> bool:
    return key < n_keys and (pkt_len >= 0 or pkt_len == ERR_PACKET_TOO_SHORT)


def replay_batch_ref(pkts, pkt_len, counter, filters: np.ndarray, limit: int = REJECT_AFTER_MESSAGES):
    """(verdict, filters after) of wgcs_replay_batch: sequential Validate calls
    in slot order on copies of the REPLAY_FILTER_DTYPE rows."""
    fl = filters_from_array(filters)
    verdict = np.array(pkt_len, np.int32).copy()
    for i in range(len(verdict)):
        key = int(pkts["key"][i])
        if takes_part(key, int(verdict[i]), len(fl)) and not fl[key].validate(int(counter[i]), limit):
            verdict[i] = ERR_REPLAY
    return verdict, filters_to_array(fl)


def send_assign_ref(sizes, peer, count, status, max_segs: int, stride: int, peer_key: dict, send_nonce,
                    limit: int = REJECT_AFTER_MESSAGES):
    """(pkts, nbufs, job_key, send_nonce after) of wgcs_send_assign_batch:
    the jobs in order, each key's nonce counted up as send.go:383-390 does.
    peer_key maps a peer id to its key row; n_keys = len(send_nonce)."""
    nj, n_keys = len(count), len(send_nonce)
    nonce = [int(x) for x in send_nonce]
    dead = [False] * n_keys
    pk = np.zeros(nj * max_segs, AEAD_PKT_DTYPE)
    pk["off"] = np.arange(nj * max_segs, dtype=np.uint64) * np.uint64(stride)
    pk["key"] = NO_KEY
    nbufs, job_key = np.zeros(nj, np.int32), np.full(nj, NO_KEY, np.uint32)
    for j in range(nj):
        c, p = int(count[j]), int(peer[j * max_segs])
        if status[j] != 0 or not 1 <= c <= max_segs or p == PEER_NONE:
            continue
        k = peer_key.get(p, NO_KEY)
        if k >= n_keys or dead[k]:
            continue
        if nonce[k] + c > limit:  # Python ints: no wrap
            dead[k], nonce[k] = True, limit
            continue
        nbufs[j], job_key[j] = c, k
        for q in range(j * max_segs, j * max_segs + c):
            pk[q] = (q * stride, nonce[k], int(sizes[q]) & 0xFFFFFFFF, k)
            nonce[k] += 1
    return pk, nbufs, job_key, np.array(nonce, np.uint64)


# ------------------------------------------------------------------ test data
def sequence(rng, n, limit=None):
    """(values, limit): counters as a receiver sees them, mostly ascending,
    with displaced and repeated values, window edges, jumps of >= 128 blocks
    and values around the limit (the one given, or one drawn here)."""
    small = limit is None and rng.random() < 0.15  # a limit that the sequence itself reaches
    limit = int(rng.integers(1 << 18, 1 << 20)) if small else (limit or REJECT_AFTER_MESSAGES)
    jumps = [63, 64, 65, 127 * 64, 128 * 64 - 1, 128 * 64, 128 * 64 + 1, 300 * 64] + ([] if small else [1 << 40])
    out, cur = [], 0 if small else int(rng.integers(0, 3)) * int(rng.integers(0, 1 << 33))
    for i in range(n):
        r = rng.random()
        if 0.90 <= r < 0.95 and i < 0.9 * n:
            r = 0.0  # a value next to the limit ends a sequence: those come late
        if r < 0.55:
            cur += int(rng.integers(1, 4))
            v = cur
        elif r < 0.65 and out:
            v = out[int(rng.integers(max(0, len(out) - 70), len(out)))]  # a repeat
        elif r < 0.75:
            v = max(0, cur - int(rng.integers(0, 200)))
        elif r < 0.85:
            v = max(0, cur - WINDOW + int(rng.integers(-3, 4)))  # the window's edge
        elif r < 0.90:
            cur += int(rng.choice(jumps))
            v = cur
        elif r < 0.95:
            v = limit + int(rng.integers(-2, 3))
        elif r < 0.99:
            v = cur + int(rng.integers(1, 1 << 20))
        else:
            v = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        v = min(v, U64)  # a counter is 64 bits on the wire
        out.append(v)
        if v < limit:
            cur = max(cur, v)
    return out, limit


# Hand-derived (values, verdicts) on an empty filter with the limit REJECT_AFTER_MESSAGES.
EDGES = {
    "zero": ([0, 0], [True, False]),
    "behind_by_window": ([WINDOW + 5, 5, 5], [True, True, False]),
    "behind_by_window_plus_one": ([WINDOW + 6, 5], [True, False]),
    "limit": ([REJECT_AFTER_MESSAGES - 1, REJECT_AFTER_MESSAGES, REJECT_AFTER_MESSAGES + 1, (1 << 64) - 1, REJECT_AFTER_MESSAGES - 1], [True, False, False, False, False]),
    "advance_63": ([1, 64, 1, 64], [True, True, False, False]),
    "advance_64": ([1, 65, 1, 65], [True, True, False, False]),
    "advance_127_blocks": ([1, 1 + 127 * 64, 1, 2], [True, True, False, True]),
    "advance_128_blocks": ([1, 1 + 128 * 64, 1], [True, True, False]),
    "advance_2_40": ([7, 7 + (1 << 40), 7, 7 + (1 << 40) - WINDOW, 7 + (1 << 40) - WINDOW - 1],
                     [True, True, False, True, False]),
    # 100 is set, a jump of >= 128 blocks pushes it out, then 100 + 8192 reuses its ring slot
    "slot_reuse": ([100, 100 + 200 * 64, 100 + 8192, 100 + 8192, 100], [True, True, True, False, False]),
}
