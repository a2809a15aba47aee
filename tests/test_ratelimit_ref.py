"""The host forms of the rate limiter (wgcs_ratelimit_allow, _batch_host,
_cleanup_host; wireguard_amd/csrc/ratelimit.cpp over wgcs_ratelimit.h) against
tests/ratelimit_ref.py, the literal restatement of ratelimiter.go that calls
Allow once per row (CPU only).

The batch form decides the m rows of one address by a closed form; the
restatement knows none.  Every comparison here is therefore also the proof that
the closed form is what sequential Allow calls under one clock value leave.
Tables are compared through entries(), and every table must be one the probe
can read (ratelimit_cases.check_reachable)."""
import random

import numpy as np
import pytest

import ratelimit_ref as ref
from ratelimit_cases import (COST, ERR_MAC1, HS_COOKIE, HS_NONE, HS_PASS, MAX, SECOND, by_home, check_reachable,
                             colliding, key_of, srcs, v4)
from wireguard_amd import _lib, ratelimit as rl
from wireguard_amd.cookie import SRC_ADDR_DTYPE

LIMITED, FULL = rl.ERR_RATE_LIMITED, rl.ERR_RATE_TABLE_FULL


class Pair:
    """The library's table and the restatement side by side."""

    def __init__(self, n_slots):
        self.tab, self.ref = rl.table(n_slots), ref.RateLimiter(capacity=n_slots)

    def batch(self, addrs, now, gate=None, src=None):
        s = srcs(addrs) if src is None else src
        g = np.full(len(s), HS_PASS, np.int32) if gate is None else np.asarray(gate, np.int32)
        stats = np.full(4, 0xEEEEEEEE, np.uint32)
        got = rl.allow_host(g, s, self.tab, now, stats=stats)
        want, want_stats = self.ref.batch(g, s, now)
        assert got.tolist() == want
        assert stats.tolist() == want_stats
        self.same()
        return got.tolist()

    def cleanup(self, now):
        self.tab, live = rl.cleanup_host(self.tab, now)
        self.ref.now_ns = now
        assert self.ref.cleanup() == (live == 0)
        assert live == len(self.ref.table)
        self.same()
        return live

    def same(self):
        assert rl.entries(self.tab) == self.ref.entries()
        check_reachable(self.tab)


A, B = ("1.2.3.4", 1000), ("2001:db8::1", 1000)


def test_constants_and_symbols():
    assert (rl.RL_PACKET_COST_NS, rl.RL_MAX_TOKENS_NS, rl.RL_CLEANUP_NS) == (ref.packetCost, ref.maxTokens, ref.cleanupInterval)
    assert (LIMITED, FULL) == (ref.ERR_RATE_LIMITED, ref.ERR_RATE_TABLE_FULL) == (-28, -29)
    L = _lib.load()
    texts = {L.wgcs_strerror(c) for c in (LIMITED, FULL)}
    assert len(texts) == 2 and b"unknown status" not in texts
    for name in ("wgcs_ratelimit_home_slot", "wgcs_ratelimit_allow", "wgcs_ratelimit_batch", "wgcs_ratelimit_cleanup_batch",
                 "wgcs_ratelimit_batch_host", "wgcs_ratelimit_cleanup_host"):
        assert name in _lib.declared_symbols() and hasattr(L, name)


def test_new_address():
    p = Pair(8)
    assert p.batch([A], 10 * SECOND) == [HS_PASS]
    assert rl.entries(p.tab) == {key_of("1.2.3.4"): (MAX - COST, 10 * SECOND)}


def test_burst_of_five_then_refused():
    p = Pair(8)
    assert p.batch([A] * 6, SECOND) == [HS_PASS] * 5 + [LIMITED]
    assert rl.entries(p.tab)[key_of("1.2.3.4")] == (0, SECOND)
    p = Pair(8)
    assert p.batch([A] * 3, SECOND) == [HS_PASS] * 3
    assert p.batch([A] * 40, SECOND) == [HS_PASS] * 2 + [LIMITED] * 38


def test_refill_of_exactly_packet_cost_and_a_nanosecond_less():
    for short, want in ((0, HS_PASS), (1, LIMITED)):
        p = Pair(8)
        p.batch([A] * 5, SECOND)
        assert p.batch([A, A], SECOND + COST - short) == [want, LIMITED]
        assert rl.entries(p.tab)[key_of("1.2.3.4")] == (COST - 1 if short else 0, SECOND + COST - short)


def test_cap_at_max_tokens_after_a_long_idle():
    p = Pair(8)
    p.batch([A] * 5, SECOND)
    assert p.batch([A] * 7, 3600 * SECOND) == [HS_PASS] * 5 + [LIMITED] * 2
    assert rl.entries(p.tab)[key_of("1.2.3.4")] == (0, 3600 * SECOND)


def test_refused_call_still_moves_last_ns():
    p = Pair(8)
    p.batch([A] * 5, SECOND)
    assert p.batch([A], SECOND + 30_000_000) == [LIMITED]
    assert rl.entries(p.tab)[key_of("1.2.3.4")] == (30_000_000, SECOND + 30_000_000)
    assert p.batch([A], SECOND + 50_000_000) == [HS_PASS]  # 30 ms + 20 ms


def test_clock_that_went_back():
    p = Pair(8)
    p.batch([A], 10 * SECOND)
    assert p.batch([A] * 5, 10 * SECOND - 120_000_000) == [HS_PASS] + [LIMITED] * 4  # 200 ms - 120 ms
    assert rl.entries(p.tab)[key_of("1.2.3.4")] == (30_000_000, 10 * SECOND - 120_000_000)
    p.batch([A] * 2, 9 * SECOND)  # far enough back for the tokens to go below zero
    assert rl.entries(p.tab)[key_of("1.2.3.4")][0] < 0


def test_v4_and_v4_mapped_v6_are_two_addresses():
    p = Pair(8)
    mapped = ("::ffff:1.2.3.4", 1000)
    assert p.batch([A] * 5 + [mapped] * 6, SECOND) == [HS_PASS] * 10 + [LIMITED]
    assert set(rl.entries(p.tab)) == {key_of("1.2.3.4"), key_of("::ffff:1.2.3.4")}
    short4 = ("1.2.3.4", 1)  # and an IPv6 address whose first four bytes are those of A, the rest zero
    assert p.batch([(bytes([1, 2, 3, 4]) + bytes(12), 1), short4], SECOND) == [HS_PASS, LIMITED]


def test_same_address_with_two_ports_is_one_bucket():
    p = Pair(8)
    assert p.batch([("1.2.3.4", 1), ("1.2.3.4", 2)] * 3, SECOND) == [HS_PASS] * 5 + [LIMITED]
    assert len(rl.entries(p.tab)) == 1
    assert p.batch([B, ("2001:db8::1", 7)] * 3, SECOND) == [HS_PASS] * 5 + [LIMITED]


def test_non_pass_gate_is_untouched_and_bad_len():
    p = Pair(8)
    s = srcs([A] * 8)
    s["len"][3] = 7
    s["len"][5] = 0  # behind a gate that is not a pass, a bad len is never looked at
    gate = [HS_PASS, HS_NONE, HS_COOKIE, HS_PASS, ERR_MAC1, HS_COOKIE, HS_PASS, 12345]
    assert p.batch(None, SECOND, gate=gate, src=s) == [HS_PASS, HS_NONE, HS_COOKIE, -1, ERR_MAC1, HS_COOKIE, HS_PASS, 12345]
    assert rl.entries(p.tab)[key_of("1.2.3.4")] == (MAX - 2 * COST, SECOND)
    # verdict in place of gate
    g = np.array(gate, np.int32)
    tab = rl.table(8)
    assert rl.allow_host(g, s, tab, SECOND, verdict=g) is not None and g.tolist() == [1, 0, 2, -1, ERR_MAC1, 2, 1, 12345]


def test_empty_batch_writes_stats():
    stats = np.full(4, 7, np.uint32)
    assert len(rl.allow_host(np.zeros(0, np.int32), np.zeros(0, SRC_ADDR_DTYPE), rl.table(8), SECOND, stats=stats)) == 0
    assert stats.tolist() == [0, 0, 0, 0]


def test_bad_arguments():
    L = _lib.load()
    s, tab = srcs([A]), rl.table(8)
    assert L.wgcs_ratelimit_allow(tab.ctypes.data, 6, s.ctypes.data, 0) == _lib.ERR_INVALID_ARG
    assert L.wgcs_ratelimit_allow(tab.ctypes.data, 0, s.ctypes.data, 0) == _lib.ERR_INVALID_ARG
    assert L.wgcs_ratelimit_allow(None, 8, s.ctypes.data, 0) == _lib.ERR_INVALID_ARG
    s["len"] = 5
    assert L.wgcs_ratelimit_allow(tab.ctypes.data, 8, s.ctypes.data, 0) == _lib.ERR_INVALID_ARG
    assert L.wgcs_ratelimit_home_slot(s.ctypes.data, 8) == 0 and not tab.view(np.uint8).any()
    live = np.zeros(1, np.uint32)
    assert L.wgcs_ratelimit_cleanup_host(tab.ctypes.data, tab.ctypes.data, 8, 0, live.ctypes.data) == _lib.ERR_INVALID_ARG
    assert L.wgcs_ratelimit_cleanup_host(tab.ctypes.data, tab[4:].ctypes.data, 8, 0, live.ctypes.data) == _lib.ERR_INVALID_ARG
    assert L.wgcs_ratelimit_batch(None, None, None, 0, None, 8, 0, None, None, None, 0, None) == _lib.ERR_INVALID_ARG


def test_cleanup_at_exactly_one_second_and_a_nanosecond_more():
    p = Pair(8)
    p.batch([A, B], 5 * SECOND)
    p.batch([B], 5 * SECOND + 1)
    assert p.cleanup(6 * SECOND) == 2           # now - last == 1 s: kept
    assert p.cleanup(6 * SECOND + 1) == 1       # A is 1 s + 1 ns idle, B exactly 1 s
    assert set(rl.entries(p.tab)) == {key_of("2001:db8::1")}
    assert p.cleanup(6 * SECOND + 2) == 0 and not p.tab.view(np.uint8).any()
    assert p.batch([A] * 6, 7 * SECOND) == [HS_PASS] * 5 + [LIMITED]  # forgotten: a new address again


def test_table_full_before_the_call():
    p = Pair(4)
    known = [(v4(i), 9) for i in range(4)]
    assert p.batch(known, SECOND) == [HS_PASS] * 4
    new = (v4(100), 9)
    assert p.batch([new, known[2], new, known[2]], SECOND) == [FULL, HS_PASS, FULL, HS_PASS]
    assert key_of(v4(100)) not in rl.entries(p.tab)
    assert p.cleanup(3 * SECOND) == 0
    assert p.batch([new], 3 * SECOND) == [HS_PASS]


def test_more_new_addresses_than_free_slots_in_row_order():
    p = Pair(4)
    p.batch([(v4(0), 1)], SECOND)
    rows = [(v4(i), 1) for i in (7, 8, 7, 9, 10, 8, 11, 0, 9)]
    assert p.batch(rows, SECOND) == [HS_PASS, HS_PASS, HS_PASS, HS_PASS, FULL, HS_PASS, FULL, HS_PASS, HS_PASS]
    assert set(rl.entries(p.tab)) == {key_of(v4(i)) for i in (0, 7, 8, 9)}


def test_forty_addresses_with_one_home_slot():
    p = Pair(64)
    ips = colliding(64, 61, 40)
    assert p.batch([(ip, 1) for ip in ips] * 2, SECOND) == [HS_PASS] * 80
    occupied = np.flatnonzero(p.tab["state"]).tolist()
    assert occupied == sorted((61 + i) % 64 for i in range(40))  # one run from the home slot, round the end


@pytest.mark.parametrize("n_slots", [8, 64])
def test_random_sequences_against_the_restatement(n_slots):
    count = 0
    for seed in range(100):
        rng = random.Random(1000 * n_slots + seed)
        n_addr = rng.randint(1, 40)
        homes = [rng.randrange(n_slots) if rng.random() < 0.5 else rng.randrange(min(3, n_slots)) for _ in range(n_addr)]
        pool = [(ip, rng.randrange(65536)) for ip in by_home(n_slots, homes, start=rng.randrange(1000))]
        pool += [("fd00::" + format(i + 1, "x"), 5) for i in range(rng.randint(0, 3))]
        p, now = Pair(n_slots), rng.randrange(10**12)
        for _ in range(rng.randint(3, 12)):
            now += rng.choice([0, 1, COST - 1, COST, 3 * COST + 7, MAX, SECOND - 1, SECOND, SECOND + 1, -COST])
            if rng.random() < 0.25:
                p.cleanup(now)
                continue
            rows = [rng.choice(pool) if rng.random() < 0.7 else pool[0] for _ in range(rng.randint(0, 30))]
            gate = [HS_PASS if rng.random() < 0.85 else rng.choice([HS_NONE, HS_COOKIE, ERR_MAC1]) for _ in rows]
            s = srcs(rows)
            if rows and rng.random() < 0.2:
                s["len"][rng.randrange(len(rows))] = rng.choice([0, 5, 17, 19])
            p.batch(None, now, gate=gate, src=s)
            count += 1
    assert count > 300


def test_allow_row_by_row_leaves_what_one_batch_leaves():
    rng = random.Random(7)
    for n_slots in (8, 64):
        ips = by_home(n_slots, [rng.randrange(3) for _ in range(n_slots + 3)])
        one, many, now = rl.table(n_slots), rl.table(n_slots), 0
        for _ in range(30):
            now += rng.choice([0, COST, 2 * COST + 1, SECOND // 2])
            rows = srcs([(rng.choice(ips), 1) for _ in range(rng.randint(1, 25))])
            want = rl.allow_host(np.full(len(rows), HS_PASS, np.int32), rows, one, now).tolist()
            got = []
            for r in rows:
                try:
                    got.append(HS_PASS if rl.allow(many, r, now) else LIMITED)
                except _lib.WgcsError as e:
                    got.append(e.code)
            assert got == want and rl.entries(many) == rl.entries(one)
            check_reachable(many)
        assert len(rl.entries(one)) == n_slots  # the pool is larger than the table: it filled up
