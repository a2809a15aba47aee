"""The worlds and steps of the keypair rotation tests (tests/test_keypairs_ref.py,
tests/test_keypairs_host.py, tests/test_gpu_keypairs.py).

A world is what the host sets up ahead of a run of calls: a peer table with its
id -> row map, an all-nil wgcs_keypairs table, the two slot arrays with every
index and every peer id registered under WGCS_SESSION_NO_KEYPAIR, an AEAD key
table of random bytes (as if respond / finish had filled it) with its key ->
peer id column, and the initiator's handshake states with their slots.  A case
is a world and steps -- one call each -- that run one after another on the
tables the step before left.  The calls read only a few fields of a
descriptor, a state row or a packet row, so the rest is random bytes, and a
row that is gated off is all 0xEE: nothing of it may be read into a decision.
"""
import functools
from types import SimpleNamespace

import numpy as np

import keypairs_ref as ref
from keypairs_ref import (ERR_PACKET_TOO_SHORT, HS_FINISHED, HS_RESPONDED, NO_KEYPAIR, PEER_NONE)
from noise_accept_cases import table_of
from wireguard_amd import keypairs, router
from wireguard_amd.noise import HS_RESP_DTYPE, HS_STATE_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

NOW = 1_700_000_000_123_456_789
FILL = 0xEE
ERR_AUTH, ERR_REPLAY, ERR_SOURCE = -18, -20, -19
TABLES = ("kp", "slots", "peer_keys", "keys", "key_peer")


def world(n_peers, n_keys, indices, handshakes=(), seed=3, stray=True):
    """indices: every receiver index registered in d_slots.  handshakes: (local_index, peer_row, send_key,
    recv_key) per state row of the initiator.  With `stray`, the last two key rows start out naming peer ids
    that have no row: one past n_ids, one whose entry of the id map is WGCS_PEER_NONE."""
    rng = np.random.default_rng(seed)
    table, peer_rows, n_ids = table_of(n_peers)
    keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    key_peer = np.full(n_keys, PEER_NONE, np.uint32)
    if stray:
        key_peer[n_keys - 1], key_peer[n_keys - 2] = n_ids + 5, 11
        assert peer_rows[11] == PEER_NONE
    idx = np.array(indices, np.uint32)
    slots = router.session_table(idx, np.full(len(idx), NO_KEYPAIR, np.uint32))
    peer_keys = router.session_table(table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
    states = np.frombuffer(rng.bytes(128 * len(handshakes)), HS_STATE_DTYPE).copy()
    for r, (li, pr, sk, rk) in enumerate(handshakes):
        states["local_index"][r], states["peer_row"][r], states["send_key"][r], states["recv_key"][r] = li, pr, sk, rk
    hs_index = {int(h[0]): r for r, h in enumerate(handshakes)}
    hs_slots = router.session_table(np.array(list(hs_index), np.uint32), np.array(list(hs_index.values()), np.uint32))
    return SimpleNamespace(table=table, peer_rows=peer_rows, n_ids=n_ids, kp=keypairs.keypairs_table(n_peers),
                           slots=slots, peer_keys=peer_keys, keys=keys, key_peer=key_peer, states=states,
                           hs_slots=hs_slots, hs_index=hs_index, indices=[int(i) for i in indices])


def tables_of(w):
    return {k: getattr(w, k).copy() for k in TABLES}


def resp_step(descs, now=NOW, seed=21):
    """descs: (peer_row, local_index, send_key, recv_key[, gate = HS_RESPONDED])"""
    rng = np.random.default_rng(seed)
    resp = np.frombuffer(rng.bytes(80 * len(descs)), HS_RESP_DTYPE).copy()
    gate = np.zeros(len(descs), np.int32)
    for j, d in enumerate(descs):
        pr, li, sk, rk, g = d if len(d) == 5 else (*d, HS_RESPONDED)
        gate[j] = g
        if g != HS_RESPONDED:
            resp[j:j + 1].view(np.uint8)[:] = FILL
            continue
        resp["peer_row"][j], resp["local_index"][j], resp["send_key"][j], resp["recv_key"][j] = pr, li, sk, rk
    return SimpleNamespace(kind="resp", resp=resp, gate=gate, now=now, n=len(descs))


def init_step(rows, now=NOW, seed=22):
    """rows: (msg.Receiver[, gate = HS_FINISHED]); the 92-byte messages lie at offsets of every residue mod 4"""
    rng = np.random.default_rng(seed)
    pitch = 97
    arena = np.frombuffer(rng.bytes(pitch * len(rows) + 8), np.uint8).copy()
    pkts = np.frombuffer(rng.bytes(24 * len(rows)), AEAD_PKT_DTYPE).copy()
    gate = np.zeros(len(rows), np.int32)
    for q, r in enumerate(rows):
        receiver, g = r if isinstance(r, tuple) else (r, HS_FINISHED)
        off = 3 + pitch * q
        gate[q] = g
        if g != HS_FINISHED:
            pkts[q:q + 1].view(np.uint8)[:] = FILL  # an offset far outside the arena: it must not be followed
            continue
        pkts["off"][q], pkts["len"][q] = off, 92
        arena[off + 8:off + 12] = np.frombuffer(int(receiver).to_bytes(4, "little"), np.uint8)
    return SimpleNamespace(kind="init", arena=arena, pkts=pkts, gate=gate, now=now, n=len(rows))


def recv_step(rows, seed=23):
    """rows: (key row, replay_batch's verdict)"""
    rng = np.random.default_rng(seed)
    pkts = np.frombuffer(rng.bytes(24 * len(rows)), AEAD_PKT_DTYPE).copy()
    pkts["key"] = [r[0] for r in rows]
    return SimpleNamespace(kind="recv", pkts=pkts, verdict=np.array([r[1] for r in rows], np.int32), n=len(rows))


def run_host(w, t, s):
    """One step through the library's host form on the tables t (in place); the step's output."""
    if s.kind == "recv":
        out = np.full(s.n, 0xEEEEEEEE, np.uint32)
        keypairs.received_host(s.pkts, s.verdict, t["key_peer"], w.peer_rows, t["kp"], t["slots"], t["peer_keys"],
                               t["keys"], out)
        return out
    out = np.full(s.n, -286331154, np.int32)  # 0xEEEEEEEE
    if s.kind == "resp":
        keypairs.begin_responder_host(s.resp, s.gate, s.now, w.table, t["kp"], t["slots"], t["peer_keys"], t["keys"],
                                      t["key_peer"], out)
    else:
        keypairs.begin_initiator_host(s.arena, s.pkts, s.gate, s.now, w.hs_slots, w.states, w.table, t["kp"],
                                      t["slots"], t["peer_keys"], t["keys"], t["key_peer"], out)
    return out


def device_of(w):
    d = ref.Device(w.table, w.peer_rows, w.keys, w.key_peer)
    for i in w.indices:
        d.sessions_new_index(i, None)  # NewIndex: the peer is not looked at
    return d


def run_ref(w, d, s):
    if s.kind == "recv":
        return d.received(s.pkts, s.verdict)
    if s.kind == "resp":
        return d.begin_responder(s.resp, s.gate, s.now)
    return d.begin_initiator(s.arena, s.pkts, s.gate, s.now, w.hs_index, w.states)


def case(name, w, steps):
    return SimpleNamespace(name=name, world=w, steps=steps)


I = [0x1000 + 77 * i for i in range(12)]  # registered receiver indices
OK = 100                                  # a packet length


@functools.lru_cache(maxsize=None)
def named():
    c = []
    w = lambda **kw: world(4, 16, I, **kw)  # noqa: E731
    # the initiator's handshakes of the named cases: index, peer row, send key, recv key
    hs = [(I[6], 1, 8, 9), (I[7], 1, 10, 11), (I[8], 1, 12, 13), (I[9], 2, 6, 7), (0x7777, 2, 4, 5), (I[10], 9, 2, 3),
          (I[11], 2, 16, 3), (I[5], 2, 3, 3)]
    c.append(case("responder_first", w(), [resp_step([(0, I[0], 0, 1)])]))
    c.append(case("responder_then_received", w(), [resp_step([(0, I[0], 0, 1)]), recv_step([(1, OK)]),
                                                   recv_step([(1, OK)])]))
    c.append(case("responder_twice", w(), [resp_step([(0, I[0], 0, 1)]), resp_step([(0, I[1], 2, 3)], now=NOW + 5)]))
    c.append(case("initiator_first", w(handshakes=hs), [init_step([I[6]])]))
    c.append(case("initiator_rekey_deletes_the_old_previous", w(handshakes=hs),
                  [init_step([I[6]]), init_step([I[7]], now=NOW + 1), init_step([I[8]], now=NOW + 2)]))
    c.append(case("initiator_with_a_staged_next", w(handshakes=hs),
                  [init_step([I[6]]), resp_step([(1, I[0], 0, 1)], now=NOW + 1), init_step([I[7]], now=NOW + 2)]))
    c.append(case("two_begins_of_one_peer_in_one_call", w(handshakes=hs),
                  [resp_step([(3, I[0], 0, 1), (2, I[1], 2, 3), (3, I[2], 4, 5)]),
                   init_step([I[6], I[9], I[7]], now=NOW + 9)]))
    c.append(case("a_gated_off_row", w(handshakes=hs),
                  [resp_step([(0, I[0], 0, 1, 0), (0, I[1], 2, 3), (1, I[2], 4, 5, -22), (1, I[3], 6, 7, 8)]),
                   init_step([(I[6], 0), I[7], (I[8], -24), (I[9], 8)])]))
    c.append(case("each_invalid_arg_row", w(handshakes=hs),
                  [resp_step([(4, I[0], 0, 1), (0, I[1], 16, 1), (0, I[2], 0, 16), (0, I[3], 5, 5),
                              (0xFFFFFFFF, I[4], 0, 1), (0, I[5], 0xFFFFFFFF, 0xFFFFFFFE), (0, I[0], 0, 1)]),
                   init_step([I[10], I[11], I[5]])]))
    c.append(case("an_unregistered_index", w(handshakes=hs), [resp_step([(0, 0x4242, 0, 1), (0, I[0], 2, 3)]),
                                                              init_step([0x7777])]))
    c.append(case("an_index_that_already_has_a_keypair", w(handshakes=hs),
                  [resp_step([(0, I[0], 0, 1)]), resp_step([(0, I[0], 2, 3), (1, I[0], 4, 5)], now=NOW + 1),
                   init_step([I[6]]), init_step([I[6], I[6]], now=NOW + 2)]))
    # the initiator's own lookups: an index finish never registered, a slot that names a row past the state
    # table, a state row that answers to another index
    def lookups():
        x = world(4, 16, I, handshakes=hs)
        x.hs_slots = router.session_table(np.array([I[6], I[7], I[8]], np.uint32), np.array([0, 40, 2], np.uint32))
        x.hs_index = {I[6]: 0, I[7]: 40, I[8]: 2}
        x.states["local_index"][2] = I[8] + 1
        return case("initiator_lookups", x, [init_step([0x5151, I[7], I[8], I[6]])])
    c.append(lookups())
    # received: peer row 1 with current = the initiator's (recv key 9) and next = the responder's (recv key 1).
    # A responder's begin clears previous and an initiator's clears next, so the three are never set at once.
    staged = [init_step([I[6]]), resp_step([(1, I[0], 0, 1)], now=NOW + 1)]
    c.append(case("received_under_current_or_previous", w(handshakes=hs),
                  staged + [recv_step([(9, OK), (9, 0)]), recv_step([(1, OK)]),
                            recv_step([(9, OK), (1, OK), (9, ERR_PACKET_TOO_SHORT), (1, 0)])]))
    c.append(case("three_rows_under_next", w(handshakes=hs),
                  staged + [recv_step([(9, OK), (9, OK), (1, 0), (1, OK), (9, OK), (1, ERR_PACKET_TOO_SHORT)]),
                            recv_step([(1, OK), (9, OK)])]))
    c.append(case("next_with_a_replay_or_auth_verdict", w(handshakes=hs),
                  staged + [recv_step([(1, ERR_REPLAY), (1, ERR_AUTH), (1, ERR_SOURCE), (1, -1), (1, -13)]),
                            recv_step([(1, ERR_REPLAY), (1, ERR_PACKET_TOO_SHORT), (1, OK)])]))
    c.append(case("a_key_row_whose_peer_has_no_row", w(handshakes=hs),
                  staged + [recv_step([(15, OK), (14, OK), (13, OK), (16, OK), (NO_KEYPAIR, OK), (0xFFFFFFFF, OK)])]))
    return c


@functools.lru_cache(maxsize=None)
def random_case(seed: int):
    """8 to 14 calls over 6 peers: 24 handshakes planned ahead (index, peer, two key rows, role), taken in
    order by begin calls of one to four descriptors; now and then a descriptor repeats an index, names one
    nobody registered, or carries a bad row; receive calls draw keys from every row and verdicts from the lot."""
    rng = np.random.default_rng(4000 + seed)
    n_peers, n_hs, n_keys = 6, 24, 50
    idx = [int(x) for x in rng.choice(1 << 20, n_hs, replace=False) + 1]
    plan = [(idx[h], int(rng.integers(0, n_peers)), 2 * h, 2 * h + 1, bool(rng.random() < 0.5)) for h in range(n_hs)]
    inits = [p for p in plan if p[4]]
    w = world(n_peers, n_keys, idx, handshakes=[p[:4] for p in inits], seed=seed)
    steps, h = [], 0
    for k in range(int(rng.integers(8, 15))):
        if rng.random() < 0.45 or h >= n_hs:
            rows = [(2 * int(rng.integers(0, h)) + 1 if h and rng.random() < 0.75 else int(rng.integers(0, n_keys + 2)),
                     int(rng.choice([OK, OK, OK, 0, ERR_PACKET_TOO_SHORT, ERR_REPLAY, ERR_AUTH])))
                    for _ in range(int(rng.integers(1, 13)))]  # mostly receive keys of handshakes begun so far
            steps.append(recv_step(rows, seed=100 * seed + k))
            continue
        role = plan[h][4]
        take = []
        while h < n_hs and plan[h][4] == role and len(take) < 4:
            take.append(plan[h])
            h += 1
        u = rng.random()
        if u < 0.15 and h > len(take):
            take.insert(int(rng.integers(0, len(take) + 1)), plan[int(rng.integers(0, h - len(take)))])  # an index used before
        now = NOW + 1000 * k
        if role:
            rows = [(p[0], HS_FINISHED if rng.random() < 0.9 else int(rng.integers(-24, 6))) for p in take if p[4]]
            if u > 0.9:
                rows.append(0x300000 + k)
            steps.append(init_step(rows, now=now, seed=100 * seed + k))
        else:
            descs = [(p[1], p[0], p[2], p[3], HS_RESPONDED if rng.random() < 0.9 else int(rng.integers(-24, 4)))
                     for p in take]
            if u > 0.9:
                descs.append((int(rng.integers(0, n_peers + 2)), 0x300000 + k, int(rng.integers(0, n_keys + 2)), 1))
            steps.append(resp_step(descs, now=now, seed=100 * seed + k))
    return case(f"random_{seed}", w, steps)
