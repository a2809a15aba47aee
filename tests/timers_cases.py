"""The worlds and steps of the peer-timer tests (tests/test_timers_ref.py,
tests/test_timers_host.py, tests/test_gpu_timers.py).

A world is what stands in memory ahead of a run of calls: the keypair world of
tests/keypairs_cases.py (peer table, id -> row map, wgcs_keypairs rows, the two
slot arrays, the AEAD key table and its key -> peer id column, the initiator's
handshake states) with keypairs put in by hand where a case needs them, the
wgcs_rekey table as NewPeer leaves it and the wgcs_timers table as timersInit
leaves it, every row active.  A case is a world and steps -- one call each --
that run one after another on the tables the step before left.  The calls read
a few fields of a row, so the rest is random bytes.
"""
import functools
from types import SimpleNamespace

import numpy as np

import keypairs_cases as kc
import keypairs_ref as kref
import timers_ref as ref
from keypairs_cases import NOW
from rekey_cases import resp_step  # (peer_row, gate) per descriptor: kind "resp"
from timers_ref import (GROUP_DATA, HS_BEGUN, HS_FINISHED, HS_INITIATED, HS_RESPONDED, KEEPALIVE_NOW, NEED_ANOTHER, NO_KEY,
                        PEER_NONE, SECOND)
from wireguard_amd import rekey, timers
from wireguard_amd.transport import AEAD_PKT_DTYPE
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

STATE = ("timers", "rekey", "kp", "slots", "peer_keys", "keys", "key_peer")  # what a step finds and may write
KEYPAIR_TABLES = ("kp", "slots", "peer_keys", "keys", "key_peer")
EXP_OUTS = ("ka_peer", "ka_count", "ka_sizes", "ka_status", "n_ka", "actions")
OUT_DTYPES = dict(ka_peer=np.uint32, ka_count=np.int32, ka_sizes=np.int32, ka_status=np.int32, n_ka=np.uint32,
                  actions=np.uint32)
FILL = 0xEE
SET, INITIATOR = 1, 2
JSEED = 0x5EED1234
I = kc.I                                   # registered receiver indices
HS = [(I[6], 1, 8, 9), (I[7], 2, 10, 11), (I[8], 9, 12, 13), (I[9], 1, 14, 15)]  # index, peer row, send key, recv key


def world(n_peers=4, n_keys=16, indices=I, handshakes=HS, keepalive_interval_s=0, seed=3):
    w = kc.world(n_peers, n_keys, indices, handshakes=handshakes, seed=seed, stray=False)
    w.n_peers, w.n_keys, w.ids = n_peers, n_keys, w.table["peer"].copy()
    w.rekey = rekey.rekey_table(n_peers, NOW)
    w.timers = timers.timers_table(n_peers, keepalive_interval_s)
    return w


def slot_set(slots, index, key):
    at = np.flatnonzero((slots["index"] == index) & (slots["key"] != 0xFFFFFFFF))
    assert len(at) == 1
    slots["key"][at[0]] = key


def put(w, row, slot, send_key, recv_key, index, created=NOW - 100 * SECOND, initiator=False):
    """a keypair by hand, as begin would have left it: slot is "current", "previous" or "next" """
    w.kp[slot][row] = (send_key, recv_key, index, SET | (INITIATOR if initiator else 0), created)
    w.key_peer[send_key] = w.key_peer[recv_key] = w.ids[row]
    slot_set(w.slots, index, recv_key)
    if slot == "current":
        slot_set(w.peer_keys, int(w.ids[row]), send_key)
    return w


def arm(w, row, i, when):
    w.timers["pending"][row] |= 1 << i
    w.timers["deadline_ns"][row, i] = when
    return w


def state_of(w):
    return SimpleNamespace(**{k: getattr(w, k).copy() for k in STATE})


def sent_step(jobs, now, max_segs=4, seed=41, jitter_seed=JSEED):
    """jobs: (peer id of the first slot, count, status, kept, data); a job of keepalives has only zero sizes"""
    rng = np.random.default_rng(seed)
    n = len(jobs)
    peer = rng.integers(0, 1 << 32, n * max_segs, dtype=np.uint32)  # the other slots' peers are not the job's
    peer[::max_segs] = [j[0] for j in jobs]
    sizes = rng.integers(1, 1500, n * max_segs).astype(np.int32)    # the slots past a job's count are never read
    for j, job in enumerate(jobs):
        if not job[4]:
            sizes[j * max_segs:j * max_segs + min(max(job[1], 0), max_segs)] = 0
        elif job[1] > 1:
            sizes[j * max_segs] = 0                                 # a keepalive in front of data
    return SimpleNamespace(kind="sent", now=now, sizes=sizes, peer=peer, count=np.array([j[1] for j in jobs], np.int32),
                           status=np.array([j[2] for j in jobs], np.int32),
                           job_key=np.array([7 if j[3] else NO_KEY for j in jobs], np.uint32), max_segs=max_segs,
                           jitter_seed=jitter_seed, n=n)


def rcvd_step(groups, now, calls_per_batch, seed=42):
    """groups: (peer id, tail, flags) per row of d_groups"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(rng.bytes(24 * len(groups)), WRITE_GROUP_DTYPE).copy()
    g["peer"], g["tail"], g["flags"] = [x[0] for x in groups], [x[1] for x in groups], [x[2] for x in groups]
    assert len(g) % calls_per_batch == 0
    return SimpleNamespace(kind="rcvd", now=now, groups=g, calls_per_batch=calls_per_batch, n=len(g))


def init_step(reasons, tickets, now, jitter_seed=JSEED):
    """reasons: start's word per peer row; tickets: (start's d_start_peer, initiate's status)"""
    return SimpleNamespace(kind="init", now=now, reasons=np.array(reasons, np.uint32),
                           start_peer=np.array([t[0] for t in tickets], np.uint32),
                           init_status=np.array([t[1] for t in tickets], np.int32), jitter_seed=jitter_seed,
                           n=len(tickets))


def fin_step(rows, now, seed=43):
    """rows: (msg.Receiver, begin's status[, finish's verdict = HS_FINISHED])"""
    s = kc.init_step([(r[0], r[2] if len(r) > 2 else HS_FINISHED) for r in rows], now=now, seed=seed)
    return SimpleNamespace(kind="fin", now=now, arena=s.arena, pkts=s.pkts, gate=s.gate,
                           begun=np.array([r[1] for r in rows], np.int32), n=len(rows))


def rot_step(rows, now, seed=44):
    """rows: (key row, keypairs-received's d_rotated)"""
    rng = np.random.default_rng(seed)
    pkts = np.frombuffer(rng.bytes(24 * len(rows)), AEAD_PKT_DTYPE).copy()
    pkts["key"] = [r[0] for r in rows]
    return SimpleNamespace(kind="rot", now=now, pkts=pkts, rotated=np.array([r[1] for r in rows], np.uint32), n=len(rows))


def exp_step(now, n_ka_max, staged=None):
    return SimpleNamespace(kind="exp", now=now, n_ka_max=n_ka_max,
                           staged=None if staged is None else np.array(staged, np.uint32))


def fresh_outputs(w, s, spare=0, fill=FILL):
    """the output arrays of step s, filled, with `spare` rows past the call's"""
    if s.kind != "exp":
        return {}
    byte = lambda n, dt: np.full(n * np.dtype(dt).itemsize, fill, np.uint8).view(dt)  # noqa: E731
    return dict(ka_peer=byte(s.n_ka_max + spare, np.uint32), ka_count=byte(s.n_ka_max + spare, np.int32),
                ka_sizes=byte(s.n_ka_max + spare, np.int32), ka_status=byte(s.n_ka_max + spare, np.int32),
                n_ka=byte(1 + spare, np.uint32), actions=byte(w.n_peers + spare, np.uint32))


def run_host(w, st, s, spare=0):
    """One step through the library's host form on the tables of st (in place); the step's outputs by name."""
    o = fresh_outputs(w, s, spare)
    if s.kind == "sent":
        timers.sent_host(s.sizes, s.peer, s.count, s.status, s.job_key, s.max_segs, s.now, s.jitter_seed, w.peer_rows,
                         st.timers)
    elif s.kind == "rcvd":
        timers.received_host(s.groups, s.calls_per_batch, s.now, w.peer_rows, st.timers)
    elif s.kind == "init":
        timers.initiated_host(s.reasons, s.start_peer, s.init_status, s.now, s.jitter_seed, st.timers)
    elif s.kind == "resp":
        timers.responded_host(s.resp, s.gate, s.now, st.timers)
    elif s.kind == "fin":
        timers.finished_host(s.arena, s.pkts, s.gate, s.begun, s.now, w.hs_slots, w.states, st.timers, st.rekey)
    elif s.kind == "rot":
        timers.rotated_host(s.pkts, s.rotated, s.now, st.key_peer, w.peer_rows, st.timers, st.rekey)
    else:
        timers.expire_host(s.now, st.timers, st.rekey, w.table, s.staged, st.kp, st.slots, st.peer_keys, st.keys,
                           st.key_peer, o["ka_peer"], o["ka_count"], o["ka_sizes"], o["ka_status"], o["n_ka"],
                           o["actions"], n_ka_max=s.n_ka_max)
    return o


def keypairs_device_of(w, st):
    """the keypairs and sessions of st as a keypairs_ref.Device"""
    kd = kref.Device(w.table, w.peer_rows, st.keys, st.key_peer)
    for i in w.indices:
        kd.sessions_new_index(i, None)
    for r in range(len(st.kp)):
        for name in ("previous", "current", "next"):
            x = st.kp[name][r]
            if int(x["flags"]) & SET:
                k = kref.Keypair(int(x["send_key"]), int(x["recv_key"]), int(x["local_index"]),
                                 bool(int(x["flags"]) & INITIATOR), int(x["created_ns"]))
                setattr(kd.peers[r].keypairs, name, k)
                kd.sessions[k.local_index] = kref.Session(None, keypair=k)
    return kd


def device_of(w, st):
    return ref.Device(w.peer_rows, st.timers, keypairs_device_of(w, st))


def run_ref(d, w, s, rekey_table, key_peer):
    """The same step through the restatement; rekey_table (the section's words of it) is written in place."""
    d.load_rekey(rekey_table)
    out = {}
    if s.kind == "sent":
        d.sent(s.sizes, s.peer, s.count, s.status, s.job_key, s.max_segs, s.now, s.jitter_seed)
    elif s.kind == "rcvd":
        d.received(s.groups, s.now)
    elif s.kind == "init":
        d.initiated(s.reasons, s.start_peer, s.init_status, s.now, s.jitter_seed)
    elif s.kind == "resp":
        d.responded(s.resp, s.gate, s.now)
    elif s.kind == "fin":
        d.finished(s.arena, s.pkts, s.gate, s.begun, s.now, w.hs_index, w.states)
    elif s.kind == "rot":
        d.rotated(s.pkts, s.rotated, s.now, key_peer)
    else:
        out = d.expire(s.now, s.staged, s.n_ka_max)
    d.store_rekey(rekey_table)
    return out


def case(name, w, steps):
    return SimpleNamespace(name=name, world=w, steps=steps)


D = NOW + 7 * SECOND  # a deadline of the named cases


@functools.lru_cache(maxsize=None)
def named():
    c = []
    ids = world().ids.tolist()
    job = lambda r, kept=True, data=True, count=2: (ids[r], count, 0, kept, data)  # noqa: E731

    # each deadline at its value and a nanosecond either side; row 2 is not due, row 3 is not pending
    for i, name in enumerate(ref.NAMES):
        for tag, t in (("minus_1", D - 1), ("deadline", D), ("plus_1", D + 1)):
            w = arm(arm(world(keepalive_interval_s=25), 1, i, D), 2, i, D + 2)
            w.timers["deadline_ns"][3, i] = D - 5
            put(w, 1, "current", 0, 1, I[0])
            c.append(case(f"{name}_at_{tag}", w, [exp_step(t, 4)]))
    for attempts in (18, 19):
        w = arm(arm(world(), 0, 1, D), 0, 2, D + SECOND)
        w.timers["attempts"][0] = attempts
        c.append(case(f"attempts_at_{attempts}", w, [exp_step(D, 4), exp_step(D + 600 * SECOND, 4)]))
    w = world()
    for i in range(5):
        arm(w, 1, i, D)
    w.timers["flags"][1] = KEEPALIVE_NOW | NEED_ANOTHER  # not ACTIVE
    put(w, 1, "current", 0, 1, I[0])
    c.append(case("an_inactive_row", w, [
        exp_step(D + SECOND, 4), sent_step([job(1)], D), rcvd_step([(ids[1], 0, GROUP_DATA)], D, 1),
        init_step([1, 1, 1, 1], [(1, HS_INITIATED)], D), resp_step([(1, HS_RESPONDED)], D),
        fin_step([(I[6], HS_BEGUN)], D), rot_step([(1, 1)], D)]))
    w = world(keepalive_interval_s=25)
    c.append(case("a_clock_that_went_back", w, [
        sent_step([job(0)], D), rcvd_step([(ids[0], 0, GROUP_DATA)], D, 1), init_step([0, 0, 0, 0], [(0, HS_INITIATED)], D),
        resp_step([(0, HS_RESPONDED)], D), exp_step(D - 500 * SECOND, 4), exp_step(D + 5 * SECOND - 1, 4)]))
    # resendHandshake past its attempts deletes sendKeepalive: which of the two comes first decides the keepalive
    for tag, resend, keep in (("resend_first", D - 2, D - 1), ("keepalive_first", D - 1, D - 2), ("tied", D - 1, D - 1)):
        w = arm(arm(world(), 2, 1, resend), 2, 2, keep)
        w.timers["attempts"][2] = 19
        c.append(case(f"two_timers_due_{tag}", w, [exp_step(D, 4)]))
    w = arm(arm(arm(world(keepalive_interval_s=25), 0, 0, D - 3), 0, 3, D - 3), 0, 4, D - 4)
    put(w, 0, "current", 0, 1, I[0])
    c.append(case("three_timers_due", w, [exp_step(D, 4)]))
    for tag, flag in (("set", NEED_ANOTHER), ("clear", 0)):
        w = arm(world(), 1, 2, D)
        w.timers["flags"][1] |= flag
        c.append(case(f"need_another_{tag}", w, [exp_step(D, 4), exp_step(D + 10 * SECOND, 4)]))
    for tag, interval in (("0", 0), ("25", 25)):
        w = arm(world(keepalive_interval_s=interval), 3, 3, D)
        c.append(case(f"interval_{tag}", w, [sent_step([job(2), job(3, data=False, count=1)], D - SECOND),
                                             rcvd_step([(ids[2], 0, 0)], D - SECOND, 1), exp_step(D, 4),
                                             exp_step(D + 24 * SECOND, 4)]))
    for k, slots in enumerate((("current",), ("current", "previous"), ("current", "previous", "next")), 1):
        w = arm(world(), 1, 4, D)
        for j, name in enumerate(slots):
            put(w, 1, name, 2 * j, 2 * j + 1, I[j], initiator=j == 0)
        put(w, 2, "current", 6, 7, I[3])  # another peer's stays
        c.append(case(f"zero_out_keys_with_{k}", w, [exp_step(D, 4)]))
    w = arm(arm(world(), 0, 2, D), 1, 2, D)
    w.timers["flags"][2] |= KEEPALIVE_NOW
    w.timers["flags"][3] |= KEEPALIVE_NOW
    c.append(case("a_staged_peer", w, [exp_step(D, 4, staged=[0, 5, 1, 0])]))
    for tag, room in (("0", 0), ("less", 2), ("more", 6)):
        w = world()
        for r in range(4):
            arm(w, r, 2, D - r)
        c.append(case(f"n_ka_max_{tag}", w, [exp_step(D, room), exp_step(D + 1, room), exp_step(D + 2, 6)]))
    w = world(keepalive_interval_s=25)
    w.key_peer[12], w.key_peer[13] = w.n_ids + 5, 11  # an id past the map, an id the map has no row for
    assert w.peer_rows[11] == PEER_NONE
    c.append(case("a_peer_id_without_a_row", w, [
        sent_step([(11, 1, 0, True, True), (w.n_ids + 5, 1, 0, True, True), (PEER_NONE, 1, 0, True, True),
                   (ids[0], 0, 0, True, True), (ids[0], 5, 0, True, True), (ids[0], 1, -8, True, True),
                   (ids[0], 1, 0, False, True), (ids[1], 1, 0, True, True)], D),
        rcvd_step([(11, 0, 1), (PEER_NONE, -1, 1), (w.n_ids + 5, 2, 1), (ids[0], -1, 1)], D, 2),
        init_step([0, 0, 0, 0], [(4, HS_INITIATED), (PEER_NONE, HS_INITIATED), (2, -1), (3, HS_INITIATED)], D),
        resp_step([(4, HS_RESPONDED), (0xFFFFFFFF, HS_RESPONDED), (2, 0), (1, -22), (3, HS_RESPONDED)], D),
        fin_step([(I[8], HS_BEGUN), (0x5151, HS_BEGUN), (I[6], -24), (I[6], HS_BEGUN, 0), (I[7], HS_BEGUN)], D),
        rot_step([(12, 1), (13, 1), (16, 1), (0xFFFFFFFE, 1), (1, 0), (1, 2)], D)]))
    c.append(case("two_data_groups_of_one_peer_in_one_call", world(), [
        rcvd_step([(ids[1], 0, GROUP_DATA), (PEER_NONE, -1, 0), (ids[1], 2, GROUP_DATA), (ids[0], 3, GROUP_DATA)], D, 2),
        rcvd_step([(ids[0], 3, GROUP_DATA)], D + SECOND, 1), exp_step(D + 10 * SECOND, 4),
        exp_step(D + 20 * SECOND, 4), exp_step(D + 30 * SECOND, 4)]))
    # the event calls as their sites use them
    w = arm(world(keepalive_interval_s=25), 0, 2, D + 9 * SECOND)
    c.append(case("sent_data_and_keepalive", w, [
        sent_step([job(0), job(1, data=False, count=1), job(2, kept=False), job(0)], D),
        sent_step([job(0), job(1)], D + SECOND, jitter_seed=JSEED + 1), exp_step(D + 15 * SECOND + 334_000_000, 4)]))
    w = world(keepalive_interval_s=25)
    w.timers["attempts"][:] = [3, 4, 5, 6]
    c.append(case("initiated_fresh_and_retry", w, [
        init_step([ref.WANT_RETRY, ref.WANT_RETRY | 1, 0, ref.WANT_NEW_HANDSHAKE],
                  [(0, HS_INITIATED), (1, HS_INITIATED), (3, -1), (PEER_NONE, -1)], D),
        exp_step(D + 5 * SECOND + 334_000_000, 4), init_step([ref.WANT_RETRY, ref.WANT_RETRY, 0, 0],
                                                              [(0, HS_INITIATED), (1, HS_INITIATED)], D + 6 * SECOND)]))
    c.append(case("responded", world(keepalive_interval_s=25), [
        resp_step([(2, HS_RESPONDED), (0, 3), (2, HS_RESPONDED), (1, HS_RESPONDED)], D), exp_step(D + 540 * SECOND, 4)]))
    w = arm(arm(world(keepalive_interval_s=25), 1, 1, D + SECOND), 1, 0, D + SECOND)
    w.timers["attempts"][1], w.rekey["flags"][1], w.rekey["flags"][2] = 7, 1, 1
    c.append(case("finished_then_a_keepalive", w, [
        fin_step([(I[6], HS_BEGUN), (I[7], -24), (I[9], HS_BEGUN)], D), exp_step(D, 4), exp_step(D + 2 * SECOND, 4)]))
    w = arm(world(), 2, 1, D + SECOND)
    put(w, 2, "current", 4, 5, I[2])
    w.timers["attempts"][2], w.rekey["flags"][2] = 2, 1
    c.append(case("rotated", w, [rot_step([(5, 0), (5, 1), (9, 1)], D), exp_step(D + 2 * SECOND, 4)]))
    return c
