"""The rate limiter on the GPU (wgcs_ratelimit_batch and _cleanup_batch; the
kernels of ratelimit_kernels.hip) against the host forms of ratelimit.cpp:
verdicts and stats whole, tables through entries() -- where an entry lands
among the slots of its probe depends on which lane claimed first -- and every
device table must be one the probe can read.  tests/test_ratelimit_ref.py pins
the host forms to the restatement of the reference.

Every output sits between sentinel bytes that must keep their fill, and every
read-only input is compared with its upload afterwards."""
import random

import numpy as np
import pytest
import torch

from ratelimit_cases import (COST, ERR_MAC1, HS_COOKIE, HS_NONE, HS_PASS, SECOND, check_reachable, colliding,
                             distinct_homes, key_of, srcs, v4)
from wireguard_amd import ratelimit as rl

pytestmark = pytest.mark.gpu

LIMITED, FULL = rl.ERR_RATE_LIMITED, rl.ERR_RATE_TABLE_FULL
GUARD, FILL = 64, 0xA5
NOW = 1000 * SECOND


class Guarded:
    """A device buffer with GUARD sentinel bytes in front of and behind its payload."""

    def __init__(self, payload):
        b = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.n = len(b)
        self.whole = torch.from_numpy(np.concatenate([np.full(GUARD, FILL, np.uint8), b, np.full(GUARD, FILL, np.uint8)])).cuda()
        self.t = self.whole[GUARD:GUARD + self.n]

    def get(self, dtype) -> np.ndarray:
        a = self.whole.cpu().numpy()
        assert (a[:GUARD] == FILL).all() and (a[GUARD + self.n:] == FILL).all(), "sentinel bytes were written"
        return a[GUARD:GUARD + self.n].copy().view(dtype)


def up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def enqueue(dev, gate, src, d_tab, now, alias=False, stream=None):
    """One allow_batch, not synchronised: a function that fetches (verdict, stats) and checks the inputs."""
    n = len(gate)
    d_gate = Guarded(gate) if alias else up(gate)
    d_src = up(src)
    d_verdict = d_gate if alias else Guarded(np.full(n, 0x6E6E6E6E, np.int32))
    d_stats = Guarded(np.full(4, 0xEEEEEEEE, np.uint32))
    d_work = torch.full((rl.work_bytes(n) + 16,), 0x77, dtype=torch.uint8, device="cuda")
    rl.allow_batch(dev, d_verdict.t if alias else d_gate, d_src, d_tab.t, now, d_verdict.t, d_work, stats=d_stats.t,
                   stream=stream, n=n, n_slots=d_tab.n // 40)

    def fetch():
        assert d_src.cpu().numpy().tobytes() == src.tobytes(), "src was written"
        if not alias:
            assert d_gate.cpu().numpy().tobytes() == gate.tobytes(), "gate was written"
        return d_verdict.get(np.int32), d_stats.get(np.uint32), d_work

    return fetch


def both(dev, tab, steps, alias=False):
    """The steps (addrs or (gate, src), now) on the host form and on the device, compared after each."""
    d_tab = Guarded(tab)
    tab = tab.copy()
    out = []
    for rows, now in steps:
        if isinstance(rows, tuple):
            gate, s = np.asarray(rows[0], np.int32), rows[1]
        else:
            s = srcs(rows)
            gate = np.full(len(s), HS_PASS, np.int32)
        stats = np.zeros(4, np.uint32)
        want = rl.allow_host(gate, s, tab, now, stats=stats)
        fetch = enqueue(dev, gate, s, d_tab, now, alias=alias)
        torch.cuda.synchronize()
        got, got_stats, _ = fetch()
        assert got.tolist() == want.tolist()
        assert got_stats.tolist() == stats.tolist()
        got_tab = d_tab.get(rl.RL_ENTRY_DTYPE)
        check_reachable(got_tab)
        assert rl.entries(got_tab) == rl.entries(tab)
        out.append(got.tolist())
    return out, tab, d_tab


def mixed(n, seed):
    """n rows over about n / 4 addresses, a tenth behind other gates, a few with a bad len."""
    rng = random.Random(seed)
    pool = [(v4(rng.randrange(1 << 20)), rng.randrange(65536)) for _ in range(max(1, n // 4))]
    pool += [("fd00::%x" % rng.randrange(1 << 16), 1) for _ in range(1 + n // 50)]
    rows = [rng.choice(pool) for _ in range(n)]
    gate = [HS_PASS if rng.random() < 0.9 else rng.choice([HS_NONE, HS_COOKIE, ERR_MAC1, 77]) for _ in rows]
    s = srcs(rows)
    for q in rng.sample(range(n), n // 40):
        s["len"][q] = rng.choice([0, 4, 16, 20])
    return (gate, s)


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_new_and_known_mixed(dev, n, alias):
    # the same pool twice: the second batch meets its addresses known, 50 ms on, with other rows gated
    first, second = mixed(n, 10 + n), mixed(n, 10 + n)
    random.Random(n).shuffle(second[0])
    # at most 3 * (n / 4 + n / 50 + 1) < 1024 addresses: the table never fills, so the device has no choice to make
    both(dev, rl.table(1024), [(first, NOW), (second, NOW + COST), (mixed(n, 99 + n), NOW + 3 * COST)], alias=alias)


def test_one_address_over_all_rows(dev):
    out, tab, _ = both(dev, rl.table(64), [([("9.9.9.9", i) for i in range(1000)], NOW)] * 2 + [([("9.9.9.9", 1)] * 1000, NOW + 2 * COST)])
    assert out[0] == [HS_PASS] * 5 + [LIMITED] * 995 and out[1] == [LIMITED] * 1000
    assert out[2] == [HS_PASS] * 2 + [LIMITED] * 998 and rl.entries(tab) == {key_of("9.9.9.9"): (0, NOW + 2 * COST)}


@pytest.mark.parametrize("start", [60, 252])
def test_run_of_seven_across_a_wave_and_a_block_boundary(dev, start):
    # `start` addresses with lower slots and one row each, then the run, then ten more: its first row sits at
    # position `start` of the key order, so rows 5 and 6 look back, and the first row looks ahead, across 64 / 256
    homes = distinct_homes(4096, start + 11)
    rows = [(ip, 1) for _, ip in homes[:start]] + [(homes[start][1], 1)] * 7 + [(ip, 1) for _, ip in homes[start + 1:]]
    order = list(range(len(rows)))
    random.Random(start).shuffle(order)
    rows = [rows[i] for i in order]
    out, tab, _ = both(dev, rl.table(4096), [(rows, NOW), (rows, NOW + COST)])
    assert all(tab["state"][h] == 1 for h, _ in homes)  # every address in its home slot: the order is as built
    run = [v for v, r in zip(out[0], rows) if r[0] == homes[start][1]]
    assert run == [HS_PASS] * 5 + [LIMITED] * 2 and out[0].count(LIMITED) == 2
    run = [v for v, r in zip(out[1], rows) if r[0] == homes[start][1]]
    assert run == [HS_PASS] + [LIMITED] * 6


def test_last_run_with_uncharged_rows_behind_it(dev):
    homes = distinct_homes(64, 3)
    rows = [(homes[0][1], 1), (homes[1][1], 1)] + [(homes[2][1], 1)] * 7 + [(homes[0][1], 1)] * 5
    s = srcs(rows)
    gate = [HS_PASS] * 9 + [HS_NONE, HS_COOKIE, ERR_MAC1, HS_NONE, HS_PASS]
    s["len"][13] = 3
    for n in (14, 9, 7):  # the run ends behind gated rows and a bad len; at the batch's end; and four rows short of seven
        out, _, _ = both(dev, rl.table(64), [((gate[:n], s[:n]), NOW)])
        assert out[0][2:9] == ([HS_PASS] * 5 + [LIMITED] * 2)[:n - 2]


def test_forty_addresses_sharing_one_home_slot(dev):
    ips = colliding(64, 61, 40)
    rows = [(ip, 1) for ip in ips] * 3
    random.Random(5).shuffle(rows)
    _, tab, d_tab = both(dev, rl.table(64), [(rows, NOW), (rows[:60], NOW + COST)])
    assert sorted(np.flatnonzero(d_tab.get(rl.RL_ENTRY_DTYPE)["state"]).tolist()) == sorted((61 + i) % 64 for i in range(40))


def test_full_table(dev):
    known = [(v4(i), 1) for i in range(16)]
    new = [(v4(100 + i), 1) for i in range(5)]
    rows = new * 2 + known[3:9] * 6 + new
    out, tab, _ = both(dev, rl.table(16), [(known, NOW), (rows, NOW)])
    assert out[1][:10] == [FULL] * 10 and out[1][-5:] == [FULL] * 5 and len(rl.entries(tab)) == 16


def test_more_new_addresses_than_free_slots(dev):
    known = [(v4(i), 1) for i in range(10)]
    new = [v4(200 + i) for i in range(20)]
    rows = [(ip, 1) for ip in new] * 3 + known[:4]
    random.Random(3).shuffle(rows)
    tab = rl.table(16)
    rl.allow_host(np.full(10, HS_PASS, np.int32), srcs(known), tab, NOW)
    d_tab, s = Guarded(tab), srcs(rows)
    fetch = enqueue(dev, np.full(len(rows), HS_PASS, np.int32), s, d_tab, NOW)
    torch.cuda.synchronize()
    got, stats, _ = fetch()
    got_tab = d_tab.get(rl.RL_ENTRY_DTYPE)
    check_reachable(got_tab)
    in_table = set(rl.entries(got_tab)) - {key_of(ip) for ip, _ in known}
    refused = {key_of(ip) for (ip, _), v in zip(rows, got) if v == FULL}
    assert not (in_table & refused) and in_table | refused == {key_of(ip) for ip in new}
    assert len(rl.entries(got_tab)) == 16 and len(in_table) == 6
    for (ip, _), v in zip(rows, got):  # every row of an address fares as the address does; nobody is out of tokens
        assert v == (FULL if key_of(ip) in refused else HS_PASS)
    assert stats.tolist() == [6 * 3 + 4, 0, 14 * 3, 6]


def cleanup(dev, tab, now, stream=None):
    d_old, d_new = up(tab), Guarded(np.full(tab.nbytes, 0x3C, np.uint8))
    d_live = Guarded(np.full(1, 0xEEEEEEEE, np.uint32))
    rl.cleanup_batch(dev, d_old, d_new.t, now, d_live.t, stream=stream, n_slots=len(tab))
    return d_old, d_new, d_live


@pytest.mark.parametrize("n_slots,idle", [(64, "all"), (64, "none"), (64, "some"), (1024, "some"), (1, "none"), (1, "all")])
def test_cleanup(dev, n_slots, idle):
    rng = random.Random(n_slots)
    ips = colliding(n_slots, n_slots - 1, min(20, n_slots)) + [v4(5000 + i) for i in range(n_slots // 2)]
    ips = list(dict.fromkeys(ips))[:n_slots]
    stays = [ip for ip in ips if idle == "none" or (idle == "some" and rng.random() < 0.5)]
    tab = rl.table(n_slots)
    rl.allow_host(np.full(len(ips), HS_PASS, np.int32), srcs([(ip, 1) for ip in ips]), tab, NOW - 1)
    rl.allow_host(np.full(len(stays), HS_PASS, np.int32), srcs([(ip, 1) for ip in stays]), tab, NOW)
    now = NOW + SECOND  # an entry last used at NOW is exactly a second idle and stays; NOW - 1 goes
    want, want_live = rl.cleanup_host(tab, now)
    d_old, d_new, d_live = cleanup(dev, tab, now)
    # an allow_batch on the new table, on the same stream, with nothing in between
    again = ([(ip, 1) for ip in ips[:n_slots // 2 + 1]] + [("fd00::9", 1)]) * 2  # known, forgotten and new
    fetch = enqueue(dev, np.full(len(again), HS_PASS, np.int32), srcs(again), d_new, now)
    torch.cuda.synchronize()
    assert d_old.cpu().numpy().tobytes() == tab.tobytes(), "the old table was written"
    assert int(d_live.get(np.uint32)[0]) == want_live
    assert want_live == len(stays) and set(rl.entries(want)) == {key_of(ip) for ip in stays}
    want_v = rl.allow_host(np.full(len(again), HS_PASS, np.int32), srcs(again), want, now)
    got_v, _, _ = fetch()
    got = d_new.get(rl.RL_ENTRY_DTYPE)
    check_reachable(got)
    assert got_v.tolist() == want_v.tolist() and rl.entries(got) == rl.entries(want)


def test_cleanup_of_only_idle_entries_leaves_zeros(dev):
    tab = rl.table(64)
    rl.allow_host(np.full(30, HS_PASS, np.int32), srcs([(v4(i), 1) for i in range(30)]), tab, NOW)
    _, d_new, d_live = cleanup(dev, tab, NOW + SECOND + 1)
    torch.cuda.synchronize()
    assert int(d_live.get(np.uint32)[0]) == 0 and not d_new.get(np.uint8).any()


def test_two_batches_back_to_back_on_one_stream(dev):
    rng = random.Random(11)
    pool = [(v4(i), 1) for i in range(40)]
    a, b = [rng.choice(pool[:25]) for _ in range(700)], [rng.choice(pool) for _ in range(700)]
    tab, d_tab = rl.table(128), Guarded(rl.table(128))
    gate = np.full(700, HS_PASS, np.int32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        f1 = enqueue(dev, gate, srcs(a), d_tab, NOW, stream=stream)
        f2 = enqueue(dev, gate, srcs(b), d_tab, NOW + COST, stream=stream)
    stream.synchronize()
    (v1, s1, _), (v2, s2, _) = f1(), f2()
    w1, w2 = rl.allow_host(gate, srcs(a), tab, NOW), rl.allow_host(gate, srcs(b), tab, NOW + COST)
    assert v1.tolist() == w1.tolist() and v2.tolist() == w2.tolist()
    assert s1[3] == 25 and s2[3] == len(rl.entries(tab)) - 25
    got = d_tab.get(rl.RL_ENTRY_DTYPE)
    check_reachable(got)
    assert rl.entries(got) == rl.entries(tab)


def test_bad_arguments_leave_everything_untouched(dev):
    from wireguard_amd._lib import WgcsError
    d_tab = Guarded(rl.table(8))
    gate, s = np.full(4, HS_PASS, np.int32), srcs([("1.1.1.1", 1)] * 4)
    d_gate, d_src, d_v = up(gate), up(s), Guarded(np.full(4, 0x6E6E6E6E, np.int32))
    d_work = torch.zeros(rl.work_bytes(4), dtype=torch.uint8, device="cuda")
    for kw in (dict(n_slots=6), dict(n_slots=0), dict(work_bytes=64), dict(n=(1 << 24) + 1)):
        with pytest.raises(WgcsError):
            rl.allow_batch(dev, d_gate, d_src, d_tab.t, NOW, d_v.t, d_work, **{**dict(n=4, n_slots=8), **kw})
    with pytest.raises(WgcsError):
        rl.cleanup_batch(dev, d_tab.t, d_tab.t, NOW, d_work, n_slots=8)
    torch.cuda.synchronize()
    assert (d_v.get(np.int32) == 0x6E6E6E6E).all() and not d_tab.get(np.uint8).any()
