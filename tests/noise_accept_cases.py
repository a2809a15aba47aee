"""The batches of the handshake accept tests (tests/test_noise_accept_ref.py,
tests/test_noise_accept_host.py, tests/test_gpu_noise_accept.py).

A case is a peer table with its id -> row map, the wgcs_hs_peer rows it starts
from, and one or more steps -- (init rows, gate, now, tickets) -- that run one
after another on the peer rows the step before left.  The accept call reads
only peer, sender and timestamp of an init row and only `peer` of a table row,
so the rest of both is random bytes, no handshake is computed here."""
import functools
from types import SimpleNamespace

import numpy as np

from noise_accept_ref import COOKIE, ERR_FLOOD, HS_CONSUMED, PEER_NONE, RATE_NS, SEEN
from wireguard_amd import noise
from wireguard_amd.noise import HS_INIT_DTYPE, HS_PEER_DTYPE, HS_TICKET_DTYPE, PEER_KEY_DTYPE

NOW = 1_700_000_000_123_456_789
MS = 1_000_000
CLAIM_NONE = 0xFFFFFFFF
FILL = 0xEE
# four timestamps in bytes.Compare order whose little-endian words sort otherwise
T = [bytes.fromhex(h) for h in ("400000006543210000000001", "400000006543210001000000", "4000000065432100ff000000",
                                "400000016543200000000000")]
assert T == sorted(T) and len(set(T)) == 4


def table_of(n_peers: int, seed: int = 7):
    """(PEER_KEY_DTYPE rows with ids 10 + 3 i shuffled over the rows, the id -> row map, n_ids)."""
    rng = np.random.default_rng(seed)
    table = np.frombuffer(rng.bytes(72 * n_peers), PEER_KEY_DTYPE).copy()
    table["peer"] = 10 + 3 * rng.permutation(n_peers)
    n_ids = 10 + 3 * n_peers + 2
    rows = noise.peer_rows_build(table, n_ids)
    assert sorted(rows[rows != PEER_NONE].tolist()) == list(range(n_peers))
    return table, rows, n_ids


def peers_of(n_peers: int, seed: int = 11) -> np.ndarray:
    """Fresh rows: never consumed, claim none; every third with a valid cookie,
    the others with cookie bytes that no flag makes valid."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n_peers, HS_PEER_DTYPE)
    p["claim"] = CLAIM_NONE
    p["cookie"] = np.frombuffer(rng.bytes(16 * n_peers), np.uint8).reshape(n_peers, 16)
    p["flags"][::3] = COOKIE
    return p


def seen(p: np.ndarray, row: int, last: bytes, consumed_at: int) -> None:
    p["last_timestamp"][row] = np.frombuffer(last, np.uint8)
    p["last_consumption_ns"][row] = consumed_at
    p["flags"][row] |= SEEN
    p["state"][row] = 1
    p["remote_index"][row] = 0x01020304 + row


def tickets_of(m: int, seed: int = 13) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.frombuffer(rng.bytes(48 * m), HS_TICKET_DTYPE).copy()  # pad too: it is not copied
    t["send_key"], t["recv_key"] = 2 * np.arange(m) + 1, 2 * np.arange(m) + 2
    return t


def rows_of(table, spec, seed: int = 17):
    """(init, gate) for spec rows (table row | raw peer id as ("id", x), timestamp, gate = HS_CONSUMED).
    A row whose gate is not HS_CONSUMED is all 0xEE: nothing of it may be read into a decision."""
    rng = np.random.default_rng(seed)
    init = np.frombuffer(rng.bytes(128 * len(spec)), HS_INIT_DTYPE).copy()
    gate = np.zeros(len(spec), np.int32)
    for q, s in enumerate(spec):
        who, ts, g = s if len(s) == 3 else (*s, HS_CONSUMED)
        gate[q] = g
        if g != HS_CONSUMED:
            init[q:q + 1].view(np.uint8)[:] = FILL
            continue
        init["peer"][q] = who[1] if isinstance(who, tuple) else table["peer"][who]
        init["timestamp"][q] = np.frombuffer(ts, np.uint8)
    return init, gate


def step(table, spec, now=NOW, n_tickets=None, seed=17):
    init, gate = rows_of(table, spec, seed)
    return SimpleNamespace(init=init, gate=gate, now=now, tickets=tickets_of(len(spec) if n_tickets is None else n_tickets, seed + 1))


def case(name, n_peers, steps, setup=None, table=None):
    tab, rows, n_ids = table or table_of(n_peers)
    peers = peers_of(n_peers)
    if setup:
        setup(peers)
    return SimpleNamespace(name=name, table=tab, peer_rows=rows, n_ids=n_ids, peers=peers, steps=steps(tab))


@functools.lru_cache(maxsize=None)
def named():
    c = []
    c.append(case("n_1", 3, lambda t: [step(t, [(1, T[1])])]))
    # never consumed: no flood whatever now is; an all-zero timestamp is not after the zero lastTimestamp
    c.append(case("fresh_peers", 4, lambda t: [step(t, [(0, T[0]), (3, T[3]), (2, bytes(12)), (1, T[1])], now=5)]))
    c.append(case("flooding_at_exactly_20_ms", 2, lambda t: [step(t, [(0, T[1]), (1, T[1])])],
                  lambda p: (seen(p, 0, T[0], NOW - RATE_NS), seen(p, 1, T[0], NOW - RATE_NS - 1))))
    c.append(case("clock_went_back", 2, lambda t: [step(t, [(0, T[2]), (0, T[0]), (1, T[2])])],
                  lambda p: (seen(p, 0, T[1], NOW + 5), seen(p, 1, T[1], NOW - 25 * MS))))
    c.append(case("three_rising", 2, lambda t: [step(t, [(0, T[1]), (0, T[2]), (0, T[3])])]))
    c.append(case("equal_to_the_winner", 2, lambda t: [step(t, [(1, T[2]), (1, T[2]), (1, T[1]), (1, T[3])])]))
    c.append(case("old_row_in_front_of_the_winner", 3, lambda t: [step(t, [(2, T[0]), (2, T[1]), (2, T[2]), (2, T[3]), (2, T[1])])],
                  lambda p: seen(p, 2, T[1], NOW - 21 * MS)))

    def bad_ids():
        tab, rows, n_ids = table_of(4)
        rows = rows.copy()
        gone = int(tab["peer"][2])
        rows[gone] = PEER_NONE                  # an id whose row is WGCS_PEER_NONE
        rows[11] = 4                            # a row past the table
        rows[12] = 0                            # a row of another peer
        assert 11 not in tab["peer"] and 12 not in tab["peer"]
        spec = [(("id", n_ids), T[1]), (("id", 0xFFFFFFFF), T[1]), (("id", gone), T[1]), (("id", 11), T[1]),
                (("id", 12), T[1]), (("id", 0), T[1]), (0, T[1]), (("id", n_ids - 1), T[1])]
        return case("ids_without_a_peer", 4, lambda t: [step(t, spec)], table=(tab, rows, n_ids))
    c.append(bad_ids())
    # every gate value but HS_CONSUMED passes through, this call's own verdicts among them, from rows of 0xEE
    c.append(case("gated_rows_are_not_read", 3, lambda t: [step(t, [(0, T[1], 0), (0, T[1]), (1, T[1], -18), (1, T[2], 7),
                                                                   (1, T[1]), (2, T[3], ERR_FLOOD), (2, T[0], 1),
                                                                   (0, T[2], -23), (0, T[1])])]))
    # four winners and two tickets: the rows behind a winner without a ticket are still judged against it
    c.append(case("fewer_tickets_than_winners", 5, lambda t: [
        step(t, [(0, T[1]), (2, T[1]), (1, T[2]), (2, T[1]), (4, T[0]), (1, T[1]), (4, T[0]), (1, T[3]), (4, T[2])], n_tickets=2),
        step(t, [(1, T[2]), (4, T[0]), (0, T[2])], now=NOW + MS, n_tickets=3, seed=40)]))     # the retries
    c.append(case("no_tickets", 2, lambda t: [step(t, [(0, T[1]), (1, T[1]), (0, T[2])], n_tickets=0)]))
    c.append(case("more_tickets_than_rows", 2, lambda t: [step(t, [(0, T[1]), (0, T[0])], n_tickets=5)]))
    c.append(case("no_rows", 2, lambda t: [step(t, [], n_tickets=3)]))
    c.append(case("second_call_later", 3, lambda t: [step(t, [(0, T[1]), (1, T[2]), (0, T[3])]),
                                                     step(t, [(0, T[1]), (0, T[2]), (1, T[2]), (1, T[3]), (2, T[0])],
                                                          now=NOW + 30 * MS, seed=50)]))
    same = [(0, T[1]), (1, T[2]), (0, T[3]), (2, T[0])]
    c.append(case("the_same_call_again_within_20_ms", 3, lambda t: [step(t, same), step(t, same, now=NOW + 20 * MS),
                                                                   step(t, same, now=NOW + 20 * MS + 1)]))
    return c


@functools.lru_cache(maxsize=None)
def random_case(seed: int):
    """1 to 64 rows over 1 to 6 peers, timestamps from the pool of four, now
    within 40 ms either side of the stored consumption times, two steps."""
    rng = np.random.default_rng(9000 + seed)
    n_peers = int(rng.integers(1, 7))
    base = NOW + int(rng.integers(-10**6, 10**6))

    def setup(p):
        for r in range(n_peers):
            if rng.random() < 0.7:
                seen(p, r, T[int(rng.integers(0, 4))] if rng.random() < 0.8 else bytes(12), base + int(rng.integers(-5, 6)) * 10 * MS)

    def steps(t):
        out = []
        for k in range(2):
            n = int(rng.integers(1, 65))
            spec = []
            for _ in range(n):
                u = rng.random()
                who = int(rng.integers(0, n_peers)) if u < 0.9 else ("id", int(rng.integers(0, 40)))
                spec.append((who, T[int(rng.integers(0, 4))], HS_CONSUMED if rng.random() < 0.85 else int(rng.integers(-24, 8))))
            now = base + int(rng.integers(-40 * MS, 40 * MS + 1)) if rng.random() < 0.8 else base + int(rng.choice([-1, 0, 1])) * RATE_NS
            out.append(step(t, spec, now=now, n_tickets=int(rng.integers(0, n + 2)), seed=100 * seed + k))
        return out

    return case(f"random_{seed}", n_peers, steps, setup)


def wide(n=300, n_peers=8):
    """n rows over n_peers peers; one peer's rows sit at 3 (an old timestamp), 70
    (its winner) and 290 (floods): three waves, two 256-thread blocks, and the
    winner not in the last of them."""
    rng = np.random.default_rng(300)
    special = 5

    def setup(p):
        seen(p, special, T[1], NOW - 40 * MS)
        seen(p, 0, T[0], NOW - 10 * MS)      # floods at the start
        seen(p, 1, T[3], NOW - 50 * MS)      # every timestamp is a replay

    def steps(t):
        others = [r for r in range(n_peers) if r != special]
        spec = []
        for q in range(n):
            if q in (3, 70, 290):
                spec.append((special, {3: T[1], 70: T[2], 290: T[3]}[q]))
            elif q % 17 == 5:
                spec.append((0, T[0], int(rng.integers(-24, 3))))
            elif q % 29 == 7:
                spec.append((("id", int(rng.integers(0, 60))), T[2]))
            else:
                spec.append((others[int(rng.integers(0, len(others)))], T[int(rng.integers(0, 4))]))
        return [step(t, spec, n_tickets=n_peers + 2)]

    return case("wide", n_peers, steps, setup)
