"""The worlds and steps of the rekey tests (tests/test_rekey_ref.py,
tests/test_rekey_host.py, tests/test_gpu_rekey.py).

A world is what stands in memory ahead of a run of calls: the peer table's
id -> row map, a wgcs_keypairs table with the keypairs a case needs put in by
hand, the key -> peer id column and the send nonces of the AEAD key table, the
responder's wgcs_hs_peer rows (for their cookies) and the wgcs_rekey table as
NewPeer leaves it.  A case is a world and steps -- one call each -- that run one
after another on the wgcs_rekey table the step before left; every other table
is only read.  The calls read a few fields of a row, so the rest is random
bytes.
"""
import functools
from types import SimpleNamespace

import numpy as np

import rekey_ref as ref
from keypairs_cases import NOW
from noise_accept_cases import peers_of, table_of
from rekey_ref import (HS_RESPONDED, INITIATOR, LAST_MINUTE, NO_KEY, PEER_NONE, SECOND, SET, RejectAfterMessages,
                       RekeyAfterMessages)
from wireguard_amd import keypairs, rekey
from wireguard_amd.noise import HS_RESP_DTYPE, HS_START_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

LIMIT = RejectAfterMessages
STATE = ("rekey", "kp", "key_peer", "send_nonce", "hs_peers")  # what a step finds; it writes rekey alone
OUTS = dict(recv=("pkts",), gate=("status_out",), sent=(), rcvd=(), resp=(),
            start=("status", "reasons", "start", "start_peer", "count"))
FILL = 0xEE


def world(n_peers=4, n_keys=16, seed=5):
    table, peer_rows, n_ids = table_of(n_peers)
    return SimpleNamespace(table=table, ids=table["peer"].copy(), peer_rows=peer_rows, n_ids=n_ids, n_peers=n_peers,
                           n_keys=n_keys, kp=keypairs.keypairs_table(n_peers),
                           key_peer=np.full(n_keys, PEER_NONE, np.uint32), send_nonce=np.zeros(n_keys, np.uint64),
                           hs_peers=peers_of(n_peers, seed=seed), rekey=rekey.rekey_table(n_peers, NOW))


def put(w, row, slot, send_key, recv_key, created, initiator=False):
    """a keypair by hand: slot is "current", "previous" or "next" """
    w.kp[slot][row] = (send_key, recv_key, 0x1000 + 16 * row + send_key, SET | (INITIATOR if initiator else 0), created)
    for k in (send_key, recv_key):
        if k < w.n_keys:
            w.key_peer[k] = w.ids[row]
    return w


def state_of(w):
    return SimpleNamespace(**{k: getattr(w, k).copy() for k in STATE})


def recv_step(keys, now, seed=31):
    rng = np.random.default_rng(seed)
    pkts = np.frombuffer(rng.bytes(24 * len(keys)), AEAD_PKT_DTYPE).copy()
    pkts["key"] = keys
    return SimpleNamespace(kind="recv", now=now, pkts=pkts, n=len(keys))


def _jobs(jobs, max_segs, seed):
    """jobs: (peer id of the first slot, count, status[, kept]) -> peer, count, status, job_key"""
    rng = np.random.default_rng(seed)
    n = len(jobs)
    peer = rng.integers(0, 1 << 32, n * max_segs, dtype=np.uint32)  # the other slots' peers are not the job's
    peer[::max_segs] = [j[0] for j in jobs]
    job_key = np.array([(7 if j[3] else NO_KEY) if len(j) > 3 else NO_KEY for j in jobs], np.uint32)
    return peer, np.array([j[1] for j in jobs], np.int32), np.array([j[2] for j in jobs], np.int32), job_key


def gate_step(jobs, now, max_segs=4, limit=LIMIT, seed=32):
    peer, count, status, _ = _jobs(jobs, max_segs, seed)
    return SimpleNamespace(kind="gate", now=now, peer=peer, count=count, status_in=status, max_segs=max_segs,
                           limit=limit, n=len(jobs))


def sent_step(jobs, now, max_segs=4, limit=LIMIT, seed=33):
    peer, count, status, job_key = _jobs(jobs, max_segs, seed)
    return SimpleNamespace(kind="sent", now=now, peer=peer, count=count, status=status, job_key=job_key,
                           max_segs=max_segs, limit=limit, n=len(jobs))


def rcvd_step(groups, now, calls_per_batch, seed=34):
    """groups: (peer id, tail) per row of d_groups"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(rng.bytes(24 * len(groups)), WRITE_GROUP_DTYPE).copy()
    g["peer"], g["tail"] = [x[0] for x in groups], [x[1] for x in groups]
    assert len(g) % calls_per_batch == 0
    return SimpleNamespace(kind="rcvd", now=now, groups=g, calls_per_batch=calls_per_batch, n=len(g))


def resp_step(descs, now, seed=35):
    """descs: (peer_row, gate); a gated-off descriptor is all 0xEE"""
    rng = np.random.default_rng(seed)
    resp = np.frombuffer(rng.bytes(80 * len(descs)), HS_RESP_DTYPE).copy()
    gate = np.array([d[1] for d in descs], np.int32)
    for j, (row, g) in enumerate(descs):
        if g != HS_RESPONDED:
            resp[j:j + 1].view(np.uint8)[:] = FILL
        else:
            resp["peer_row"][j] = row
    return SimpleNamespace(kind="resp", now=now, resp=resp, gate=gate, n=len(descs))


def start_step(n_tickets, now, seed=36):
    rng = np.random.default_rng(seed)
    tickets = np.frombuffer(rng.bytes(96 * n_tickets), HS_START_DTYPE).copy()  # peer_row, flags, cookie, pads: noise
    return SimpleNamespace(kind="start", now=now, tickets=tickets, n_tickets=n_tickets)


def fresh_outputs(w, s, spare=0, fill=FILL):
    """the output arrays of step s, filled, with `spare` rows past the call's"""
    byte = lambda n, dt: np.full(n * np.dtype(dt).itemsize, fill, np.uint8).view(dt)  # noqa: E731
    if s.kind == "recv":
        return dict(pkts=s.pkts.copy())
    if s.kind == "gate":
        return dict(status_out=byte(s.n + spare, np.int32))
    if s.kind == "start":
        return dict(status=byte(w.n_peers + spare, np.int32), reasons=byte(w.n_peers + spare, np.uint32),
                    start=byte(s.n_tickets + spare, HS_START_DTYPE), start_peer=byte(s.n_tickets + spare, np.uint32),
                    count=byte(1 + spare, np.uint32))
    return {}


def run_host(w, st, s, spare=0):
    """One step through the library's host form on st.rekey (in place); the step's outputs by name."""
    o = fresh_outputs(w, s, spare)
    if s.kind == "recv":
        rekey.recv_gate_host(o["pkts"], s.now, st.key_peer, w.peer_rows, st.kp)
    elif s.kind == "gate":
        rekey.send_gate_host(s.peer, s.count, s.status_in, s.max_segs, s.now, w.peer_rows, st.kp, st.send_nonce, s.limit,
                             st.rekey, o["status_out"])
    elif s.kind == "sent":
        rekey.sent_host(s.peer, s.count, s.status, s.job_key, s.max_segs, s.now, w.peer_rows, st.kp, st.send_nonce,
                        s.limit, st.rekey)
    elif s.kind == "rcvd":
        rekey.received_host(s.groups, s.calls_per_batch, s.now, w.peer_rows, st.kp, st.rekey)
    elif s.kind == "resp":
        rekey.responded_host(s.resp, s.gate, s.now, st.rekey)
    else:
        rekey.start_host(s.now, st.rekey, st.hs_peers, s.tickets, o["start"], o["start_peer"], o["count"], o["status"],
                         o["reasons"])
    return o


def device_of(w, st):
    return ref.Device(w.peer_rows, w.n_peers, st.rekey, st.hs_peers, st.key_peer)


def run_ref(d, st, s):
    """The same step through the restatement, on the keypairs as they stand in st; its outputs by name."""
    d.load_keypairs(st.kp, st.key_peer)
    if s.kind == "recv":
        pkts = s.pkts.copy()
        pkts["key"] = d.recv_gate([int(k) for k in s.pkts["key"]], s.now)
        return dict(pkts=pkts)
    if s.kind == "gate":
        return dict(status_out=np.array(d.send_gate(s.peer, s.count, s.status_in, s.max_segs, s.now, st.send_nonce,
                                                    s.limit), np.int32))
    if s.kind == "sent":
        d.sent(s.peer, s.count, s.status, s.job_key, s.max_segs, s.now, st.send_nonce, s.limit)
    elif s.kind == "rcvd":
        d.received(s.groups, s.now)
    elif s.kind == "resp":
        d.responded(s.resp, s.gate, s.now)
    else:
        return d.start(s.now, s.tickets)
    return {}


def case(name, w, steps):
    return SimpleNamespace(name=name, world=w, steps=steps)


T0 = NOW - 200 * SECOND  # when the keypairs of the named cases were made
RT, KT, PT = 180 * SECOND, 120 * SECOND, 165 * SECOND  # RejectAfterTime, RekeyAfterTime, the last minute


def around(t):
    return (t - 1, t, t + 1)


@functools.lru_cache(maxsize=None)
def named():
    c = []
    ids = world().ids.tolist()
    # peer row r: keys 4r (send) and 4r + 1 (recv)
    cur = lambda w, r, **kw: put(w, r, "current", 4 * r, 4 * r + 1, T0, **kw)  # noqa: E731
    job = lambda r, kept=True: (ids[r], 2, 0, kept)  # noqa: E731

    w = cur(cur(world(), 0), 2, initiator=True)
    c.append(case("recv_at_180s", w, [recv_step([1, 9, 1], T0 + t) for t in around(RT)]))
    c.append(case("send_at_180s", w, [gate_step([job(0), job(2)], T0 + t) for t in around(RT)]))
    c.append(case("sent_at_120s", w, [sent_step([job(0), job(2)], T0 + t) for t in around(KT)]))
    c.append(case("received_at_165s", w, [rcvd_step([(ids[0], 3), (ids[2], 0)], T0 + t, 2) for t in around(PT)]))

    w = cur(world(), 1)
    w.rekey["want"][1] = ref.WANT_HOST
    w.rekey["last_sent_ns"][1] = T0
    c.append(case("start_at_5s", w, [start_step(1, T0 + t) for t in around(5 * SECOND)]))

    def nonces(v):
        x = cur(cur(world(), 0), 1, initiator=True)
        x.send_nonce[0] = x.send_nonce[4] = v
        return x
    for name, v in (("limit_minus_1", LIMIT - 1), ("limit", LIMIT), ("2_60", RekeyAfterMessages),
                    ("2_60_plus_1", RekeyAfterMessages + 1)):
        c.append(case(f"nonce_at_{name}", nonces(v),
                      [gate_step([job(0), job(1)], T0 + SECOND), sent_step([job(0), job(1, False)], T0 + SECOND)]))

    w = cur(cur(world(), 0, initiator=True), 3)
    w.rekey["want"][3], w.rekey["last_sent_ns"][3] = ref.WANT_HOST, T0
    back = T0 - 500 * SECOND
    c.append(case("a_clock_that_went_back", w,
                  [recv_step([1, 13], back), gate_step([job(0), job(3)], back), sent_step([job(0)], back),
                   rcvd_step([(ids[0], 1)], back, 1), start_step(2, back)]))

    w = put(put(put(world(), 1, "current", 4, 5, T0 + 100 * SECOND), 1, "previous", 6, 7, T0), 1, "next", 8, 9, T0)
    c.append(case("a_key_in_previous_and_in_next", w, [recv_step([5, 7, 9, 6, 8], T0 + RT + 1),
                                                        recv_step([7, 9, 5], T0 + RT + 100 * SECOND + 1)]))

    w = cur(world(), 0)
    w.key_peer[12], w.key_peer[13] = w.n_ids + 5, 11  # an id past the map, an id the map has no row for
    assert w.peer_rows[11] == PEER_NONE
    late = T0 + 400 * SECOND
    c.append(case("a_peer_id_without_a_row", w,
                  [recv_step([12, 13, 14, 16, 0xFFFFFFFE, 0xFFFFFFFF], late),
                   gate_step([(11, 1, 0), (w.n_ids + 5, 1, 0), (PEER_NONE, 1, 0), (ids[0], 0, 0), (ids[0], 5, 0),
                              (ids[0], 1, -8), (ids[0], 1, 0)], late),
                   sent_step([(11, 1, 0, True), (w.n_ids + 5, 1, 0, False)], late),
                   rcvd_step([(11, 0), (PEER_NONE, -1), (w.n_ids + 5, 2), (ids[0], -1)], late, 2),
                   resp_step([(4, HS_RESPONDED), (0xFFFFFFFF, HS_RESPONDED), (2, 0), (1, -22), (3, HS_RESPONDED)], late)]))

    w = put(world(), 2, "next", 8, 9, T0)
    c.append(case("current_nil", w, [gate_step([job(2), job(1)], T0 + SECOND), sent_step([job(2), job(1, False)], T0 + SECOND),
                                     rcvd_step([(ids[2], 0)], T0 + RT, 1), start_step(4, NOW)]))

    c.append(case("a_responders_keypair_past_120s", cur(world(), 0),
                  [sent_step([job(0)], T0 + KT + 50 * SECOND), rcvd_step([(ids[0], 0)], T0 + PT + SECOND, 1)]))
    w = put(world(), 1, "current", 20, 5, T0, initiator=True)
    c.append(case("a_send_key_past_the_table", w, [gate_step([job(1)], T0 + RT + 1), sent_step([job(1), job(1, False)], T0 + RT)]))

    w = cur(cur(world(), 0, initiator=True), 1, initiator=True)
    w.rekey["flags"][0] = LAST_MINUTE
    c.append(case("last_minute_already_set", w, [rcvd_step([(ids[0], 0), (ids[1], 0)], T0 + PT + 1, 2),
                                                 rcvd_step([(ids[0], 0), (ids[1], 0)], T0 + PT + 2, 1)]))
    c.append(case("two_groups_of_one_peer_in_one_call", cur(cur(world(), 0, initiator=True), 1, initiator=True),
                  [rcvd_step([(ids[1], 0), (PEER_NONE, -1), (ids[1], 2), (ids[0], 3)], T0 + PT + 1, 2)]))
    c.append(case("responded", world(), [resp_step([(2, HS_RESPONDED), (0, 3), (2, HS_RESPONDED), (1, HS_RESPONDED)], NOW + 7)]))

    def wishes(rows):
        x = world()
        for r in rows:
            x.rekey["want"][r] = 1 << r
        return x
    c.append(case("no_tickets", wishes([0, 2]), [start_step(0, NOW), start_step(1, NOW + 1)]))
    c.append(case("fewer_tickets_than_candidates", wishes([0, 1, 2, 3]),
                  [start_step(2, NOW), start_step(3, NOW + SECOND), start_step(3, NOW + 6 * SECOND)]))
    w = wishes([0, 1, 3])
    assert w.hs_peers["flags"].tolist() == [2, 0, 0, 2]
    c.append(case("a_peer_with_the_cookie_bit", w, [start_step(5, NOW)]))
    c.append(case("gate_sent_start", cur(cur(world(), 0, initiator=True), 1),
                  [gate_step([job(0), job(1), job(2)], T0 + RT), sent_step([job(0), job(1), job(2)], T0 + KT + 1),
                   start_step(2, NOW), start_step(2, NOW + SECOND)]))
    return c
