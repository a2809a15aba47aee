"""The six wgcs_rekey_*_host forms (wireguard_amd/csrc/rekey.cpp) against the
literal restatement of device/receive.go:80-91 and :162-170 and
device/send.go:84-100, :131-133, :213-227 and :368-374 in tests/rekey_ref.py
(CPU only).

After every step -- one call -- the wgcs_rekey table is compared, in all its
bytes, with what the restatement renders, and the step's own outputs (the
packet rows, the statuses, the descriptors) with the restatement's.  The named
cases are those of tests/rekey_cases.py; the random sequences mix the six calls
with the keypair rotation of wgcs_keypairs_begin_*_host and
wgcs_keypairs_received_host, drawn from the seeds fixed below."""
from collections import Counter

import numpy as np
import pytest

import keypairs_cases as kc
import rekey_cases as cases
import rekey_ref as ref
from rekey_cases import LIMIT, NOW, T0
from rekey_ref import (ERR_BATCH_FULL, ERR_KEY_EXPIRED, ERR_REKEY_TIMEOUT, HS_NONE, HS_RESPONDED, HS_STARTED, LAST_MINUTE,
                       NO_KEY, PEER_NONE, SECOND, SESSION_EXPIRED)
from wireguard_amd import _lib, rekey
from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.noise import HS_START_DTYPE

SEEDS = range(200)


def compare(where, w, st, d, s):
    got, want = cases.run_host(w, st, s), cases.run_ref(d, st, s)
    assert set(got) == set(want) == set(cases.OUTS[s.kind]), where
    for name in got:
        assert got[name].tobytes() == want[name].tobytes(), (*where, name, got[name], want[name])
    assert st.rekey.tobytes() == d.render().tobytes(), (*where, "rekey", st.rekey, d.render())
    return got


def check(c):
    w, st = c.world, cases.state_of(c.world)
    d = cases.device_of(w, st)
    frozen = {k: getattr(st, k).tobytes() for k in cases.STATE if k != "rekey"}
    outs = [compare((c.name, k, s.kind), w, st, d, s) for k, s in enumerate(c.steps)]
    assert {k: getattr(st, k).tobytes() for k in frozen} == frozen, c.name  # the read-only tables
    return st, outs


@pytest.mark.parametrize("c", cases.named(), ids=lambda c: c.name)
def test_named_case(c):
    check(c)


def named(name):
    return next(c for c in cases.named() if c.name == name)


def test_what_the_named_cases_reach():
    """The cases are what their names say: spot checks, independent of the restatement."""
    _, outs = check(named("recv_at_180s"))  # Before is strict: equality passes
    assert [o["pkts"]["key"].tolist() for o in outs] == [[1, 9, 1], [1, 9, 1], [SESSION_EXPIRED] * 3]
    st, outs = check(named("send_at_180s"))  # >=: equality expires
    assert [o["status_out"].tolist() for o in outs] == [[0, 0], [ERR_KEY_EXPIRED] * 2, [ERR_KEY_EXPIRED] * 2]
    assert st.rekey["want"].tolist() == [4, 0, 4, 0]
    st, _ = check(named("sent_at_120s"))
    assert st.rekey["want"].tolist() == [0, 0, 0x10, 0]  # the initiator alone, and only past 120 s
    c = named("sent_at_120s")
    w, s3 = c.world, cases.state_of(c.world)
    for k, s in enumerate(c.steps):  # > RekeyAfterTime: 120 s - 1 ns and 120 s leave want alone, + 1 ns sets it
        cases.run_host(w, s3, s)
        assert s3.rekey["want"][2] == (0x10 if k == 2 else 0)
    c = named("received_at_165s")
    w, s3 = c.world, cases.state_of(c.world)
    for k, s in enumerate(c.steps):
        cases.run_host(w, s3, s)
        assert (s3.rekey["want"][2], s3.rekey["flags"][2]) == ((0x20, LAST_MINUTE) if k == 2 else (0, 0))
        assert s3.rekey["want"][0] == 0 and s3.rekey["flags"][0] == 0  # a responder's keypair
    _, outs = check(named("start_at_5s"))  # < RekeyTimeout: equality starts
    assert [o["status"][1] for o in outs] == [ERR_REKEY_TIMEOUT, HS_NONE, HS_NONE]
    c = named("start_at_5s")
    for k, s in enumerate(c.steps):
        s3 = cases.state_of(c.world)
        o = cases.run_host(c.world, s3, s)
        assert o["status"][1] == (ERR_REKEY_TIMEOUT if k == 0 else HS_STARTED) and s3.rekey["want"][1] == 0
        assert s3.rekey["last_sent_ns"][1] == (T0 if k == 0 else s.now) and o["reasons"][1] == 0x40

    for name, gate, want in (("limit_minus_1", [0, 0], [0x08, 0x08 | 0x10]), ("limit", [ERR_KEY_EXPIRED] * 2, [2, 2]),
                             ("2_60", [0, 0], [0, 0x10]), ("2_60_plus_1", [0, 0], [0x08, 0x10])):
        st, outs = check(named(f"nonce_at_{name}"))
        assert outs[0]["status_out"].tolist() == gate, name
    st, _ = check(named("nonce_at_2_60"))
    assert st.rekey["want"].tolist() == [0, 0, 0, 0]  # > RekeyAfterMessages is strict; row 1's job was dropped
    st, _ = check(named("nonce_at_2_60_plus_1"))
    assert st.rekey["want"].tolist() == [8, 0, 0, 0]
    st, _ = check(named("nonce_at_limit_minus_1"))
    assert st.rekey["want"].tolist() == [8, 0, 0, 0]  # a dropped job below the limit asks for nothing

    st, outs = check(named("a_clock_that_went_back"))
    assert outs[0]["pkts"]["key"].tolist() == [1, 13] and outs[1]["status_out"].tolist() == [0, 0]
    assert outs[4]["status"].tolist() == [HS_NONE, HS_NONE, HS_NONE, ERR_REKEY_TIMEOUT] and outs[4]["count"][0] == 0
    assert not st.rekey["want"].any() and not st.rekey["flags"].any()

    _, outs = check(named("a_key_in_previous_and_in_next"))
    assert outs[0]["pkts"]["key"].tolist() == [5, SESSION_EXPIRED, SESSION_EXPIRED, 6, 8]  # send keys receive nothing
    assert outs[1]["pkts"]["key"].tolist() == [SESSION_EXPIRED] * 3

    st, outs = check(named("a_peer_id_without_a_row"))
    assert outs[0]["pkts"]["key"].tolist() == [12, 13, 14, 16, 0xFFFFFFFE, 0xFFFFFFFF]
    assert outs[1]["status_out"].tolist() == [0, 0, 0, 0, 0, -8, ERR_KEY_EXPIRED]
    assert st.rekey["want"].tolist() == [4, 0, 0, 0] and not st.rekey["flags"].any()
    late = T0 + 400 * SECOND
    assert [x == late for x in st.rekey["last_sent_ns"].tolist()] == [False, False, False, True]

    st, outs = check(named("current_nil"))
    assert outs[0]["status_out"].tolist() == [ERR_KEY_EXPIRED] * 2 and outs[3]["status"].tolist() == [0, 9, 9, 0]
    assert outs[3]["reasons"].tolist() == [0, 1, 1, 0] and outs[3]["start_peer"].tolist() == [1, 2, PEER_NONE, PEER_NONE]
    st, _ = check(named("a_responders_keypair_past_120s"))
    assert not st.rekey["want"].any() and not st.rekey["flags"].any()
    st, outs = check(named("a_send_key_past_the_table"))
    assert outs[0]["status_out"].tolist() == [0] and st.rekey["want"].tolist() == [0, 0x10, 0, 0]

    st, _ = check(named("last_minute_already_set"))
    assert st.rekey["want"].tolist() == [0, 0x20, 0, 0] and st.rekey["flags"].tolist() == [1, 1, 0, 0]
    st, _ = check(named("two_groups_of_one_peer_in_one_call"))
    assert st.rekey["want"].tolist() == [0x20, 0x20, 0, 0] and st.rekey["flags"].tolist() == [1, 1, 0, 0]
    st, _ = check(named("responded"))
    assert [x == NOW + 7 for x in st.rekey["last_sent_ns"].tolist()] == [False, True, True, False]

    st, outs = check(named("no_tickets"))
    assert outs[0]["status"].tolist() == [ERR_BATCH_FULL, 0, ERR_BATCH_FULL, 0] and outs[0]["count"][0] == 0
    assert outs[1]["status"].tolist() == [HS_STARTED, 0, ERR_BATCH_FULL, 0] and st.rekey["want"].tolist() == [0, 0, 4, 0]
    st, outs = check(named("fewer_tickets_than_candidates"))
    assert outs[0]["status"].tolist() == [9, 9, ERR_BATCH_FULL, ERR_BATCH_FULL] and outs[0]["count"][0] == 2
    assert outs[1]["status"].tolist() == [0, 0, 9, 9] and outs[1]["reasons"].tolist() == [0, 0, 4, 8]
    assert outs[1]["start_peer"].tolist() == [2, 3, PEER_NONE] and outs[1]["count"][0] == 2
    tail = outs[1]["start"][2]
    assert tail["state_row"] == 0xFFFFFFFF and not tail.tobytes()[4:].strip(b"\0")  # no ticket secret in a tail row
    assert outs[2]["status"].tolist() == [0] * 4 and outs[2]["count"][0] == 0
    _, outs = check(named("a_peer_with_the_cookie_bit"))
    c = named("a_peer_with_the_cookie_bit")
    d, t = outs[0]["start"], c.steps[0].tickets
    assert d["flags"].tolist() == [1, 0, 1, 0, 0] and d["peer_row"].tolist() == [0, 1, 3, 0, 0]
    assert d["cookie"][0].tobytes() == c.world.hs_peers["cookie"][0].tobytes() and not d["cookie"][1].any()
    assert d["cookie"][2].tobytes() == c.world.hs_peers["cookie"][3].tobytes() and not d["pad0"].any() and not d["pad1"].any()
    for f in ("state_row", "local_index", "send_key", "recv_key", "timestamp", "ephemeral_private"):
        assert d[f][:3].tobytes() == t[f][:3].tobytes(), f


def random_sequence(seed: int):
    """(the keypairs world, its steps): 18 to 30 calls over 6 peers under a clock that only moves forward, by
    steps between a second and two minutes.  Handshakes planned ahead are begun and promoted by the rotation
    calls ("rot"); between them the six rekey calls run over jobs, packets and groups of every peer ("sent"
    takes the jobs of the gate before it, with the gate's statuses and a send-assign that keeps four jobs in
    five), the send nonces jump to the thresholds now and then ("nonce"), and the host asks for a handshake of
    its own ("host")."""
    rng = np.random.default_rng(9000 + seed)
    n_peers, n_hs, n_keys = 6, 16, 36
    idx = [int(x) for x in rng.choice(1 << 20, n_hs, replace=False) + 1]
    plan = [(idx[h], int(rng.integers(0, n_peers)), 2 * h, 2 * h + 1, bool(rng.random() < 0.6)) for h in range(n_hs)]
    w = kc.world(n_peers, n_keys, idx, handshakes=[p[:4] for p in plan if p[4]], seed=seed)
    ids = w.table["peer"].tolist()
    steps, h, now = [], 0, NOW
    any_id = lambda: int(rng.choice(ids + ids + [11, w.n_ids + 3, PEER_NONE]))  # noqa: E731
    for k in range(int(rng.integers(18, 31))):
        now += int(rng.choice([1, 1, 1, 3, 3, 20, 60, 100, 125])) * SECOND + int(rng.integers(0, 1000))
        u, sd = rng.random(), 1000 * seed + k
        if u < 0.20 and h < n_hs:
            li, row, sk, rk, initiator = plan[h]
            h += 1
            steps.append(("rot", kc.init_step([li], now=now, seed=sd) if initiator else
                          kc.resp_step([(row, li, sk, rk)], now=now, seed=sd)))
        elif u < 0.30:
            steps.append(("rot", kc.recv_step([(2 * int(rng.integers(0, max(h, 1))) + 1, 100) for _ in range(3)], seed=sd)))
        elif u < 0.40:
            keys = [2 * int(rng.integers(0, max(h, 1))) + 1 if rng.random() < 0.8 else int(rng.integers(0, n_keys + 3))
                    for _ in range(int(rng.integers(1, 9)))]
            steps.append(("rekey", cases.recv_step(keys, now, seed=sd)))
        elif u < 0.65:
            jobs = [(any_id(), int(rng.choice([1, 2, 4, 0, 5])), int(rng.choice([0, 0, 0, 0, -8])))
                    for _ in range(int(rng.integers(1, 7)))]
            steps.append(("nonce", 2 * int(rng.integers(0, max(h, 1))) if rng.random() < 0.85 else int(rng.integers(0, n_keys)),
                          int(rng.choice(np.array([5, LIMIT - 1, LIMIT, 1 << 60, (1 << 60) + 1, 1 << 61, (1 << 64) - 1], np.uint64)))))
            steps.append(("rekey", cases.gate_step(jobs, now, seed=sd)))
            steps.append(("sent", rng.random(len(jobs)) < 0.8))
        elif u < 0.75:
            g = [(any_id(), int(rng.integers(-1, 5))) for _ in range(2 * int(rng.integers(1, 4)))]
            steps.append(("rekey", cases.rcvd_step(g, now, 2, seed=sd)))
        elif u < 0.80:
            steps.append(("rekey", cases.resp_step([(int(rng.integers(0, n_peers + 1)), int(rng.choice([HS_RESPONDED, 0, -22])))
                                                    for _ in range(int(rng.integers(1, 4)))], now, seed=sd)))
        elif u < 0.85:
            steps.append(("host", int(rng.integers(0, n_peers))))
        else:
            steps.append(("rekey", cases.start_step(int(rng.integers(0, 4)), now, seed=sd)))
            if rng.random() < 0.4:  # the host's timers fire a second later: those just started are within RekeyTimeout
                now += SECOND
                steps += [("host", int(r)) for r in rng.choice(n_peers, 3, replace=False)]
                steps.append(("rekey", cases.start_step(int(rng.integers(0, 4)), now, seed=sd + 500)))
    return w, steps


def test_random_sequences():
    seen = Counter()
    for seed in SEEDS:
        kw, steps = random_sequence(seed)
        t = kc.tables_of(kw)  # the rotation's tables; the rekey calls read kp and key_peer of them
        w = cases.world(6, len(kw.keys))
        assert w.peer_rows.tobytes() == kw.peer_rows.tobytes() and w.ids.tolist() == kw.table["peer"].tolist()
        st = cases.state_of(w)
        d = cases.device_of(w, st)
        gate = None
        for k, (what, *a) in enumerate(steps):
            st.kp, st.key_peer = t["kp"], t["key_peer"]
            if what == "rot":
                kc.run_host(kw, t, a[0])
                continue
            if what == "nonce":
                st.send_nonce[a[0]] = a[1]
                continue
            if what == "host":  # the host's own timer, a stream-ordered write
                st.rekey["want"][a[0]] |= ref.WANT_HOST
                d.by_row[a[0]].want |= ref.WANT_HOST
                continue
            if what == "sent":
                g, out = gate
                key = np.where(a[0] & (out == 0), 7, NO_KEY).astype(np.uint32)
                s = cases.SimpleNamespace(kind="sent", now=g.now, peer=g.peer, count=g.count, status=out, job_key=key,
                                          max_segs=g.max_segs, limit=g.limit, n=g.n)
            else:
                s = a[0]
            frozen = (t["kp"].tobytes(), t["key_peer"].tobytes(), st.send_nonce.tobytes())
            o = compare((seed, k, s.kind), w, st, d, s)
            assert frozen == (t["kp"].tobytes(), t["key_peer"].tobytes(), st.send_nonce.tobytes()), (seed, k)
            if s.kind == "recv":
                seen["expired"] += int((o["pkts"]["key"] == SESSION_EXPIRED).sum())
            elif s.kind == "gate":
                gate = (s, o["status_out"].copy())
                seen[ERR_KEY_EXPIRED] += int((o["status_out"] == ERR_KEY_EXPIRED).sum())
            elif s.kind == "start":
                for code in (HS_STARTED, ERR_BATCH_FULL, ERR_REKEY_TIMEOUT):
                    seen[code] += int((o["status"] == code).sum())
                for bit in range(7):
                    seen[f"want_{1 << bit:#04x}"] += int(((o["reasons"] >> bit) & 1).sum())
    # the sequences reach what they are for; the outputs counted are the restatement's too (compare)
    need = ["expired", ERR_KEY_EXPIRED, ERR_REKEY_TIMEOUT, HS_STARTED, ERR_BATCH_FULL] + [f"want_{1 << b:#04x}" for b in range(7)]
    assert all(seen[k] >= 20 for k in need), ", ".join(f"{k}: {seen[k]}" for k in need)


def test_host_forms_refuse_bad_arguments():
    c = named("gate_sent_start")
    w, st = c.world, cases.state_of(c.world)
    g, s, q = c.steps[0], c.steps[1], c.steps[2]
    r, v = cases.recv_step([1], NOW), cases.rcvd_step([(w.ids[0], 0)], NOW, 1)
    e = cases.resp_step([(0, HS_RESPONDED)], NOW)
    o = cases.fresh_outputs(w, q)
    out = np.full(g.n, 77, np.int32)
    L, bad = _lib.load(), _lib.ERR_INVALID_ARG
    p = lambda x: x.ctypes.data  # noqa: E731
    rows = (p(w.peer_rows), w.n_ids, p(st.kp), 4)
    non = (p(st.send_nonce), 16, LIMIT)
    assert L.wgcs_rekey_recv_gate_host(None, 1, NOW, p(st.key_peer), 16, *rows) == bad
    assert L.wgcs_rekey_recv_gate_host(p(r.pkts), 1, NOW, None, 16, *rows) == bad
    assert L.wgcs_rekey_recv_gate_host(p(r.pkts), 1, NOW, p(st.key_peer), 16, None, w.n_ids, p(st.kp), 4) == bad
    assert L.wgcs_rekey_recv_gate_host(p(r.pkts), 1, NOW, p(st.key_peer), 16, p(w.peer_rows), w.n_ids, None, 4) == bad
    assert L.wgcs_rekey_recv_gate_host(p(r.pkts), (1 << 28) + 1, NOW, p(st.key_peer), 16, *rows) == bad
    gate = lambda peer=p(g.peer), count=p(g.count), status=p(g.status_in), n=g.n, segs=g.max_segs, rk=p(st.rekey), o=p(out), nn=non: (  # noqa: E731
        L.wgcs_rekey_send_gate_host(peer, count, status, n, segs, NOW, *rows, *nn, rk, o))
    for kw in (dict(peer=None), dict(count=None), dict(status=None), dict(rk=None), dict(o=None), dict(segs=0),
               dict(n=1 << 27, segs=4), dict(nn=(None, 16, LIMIT))):
        assert gate(**kw) == bad, kw
    sent = lambda peer=p(s.peer), jk=p(s.job_key), rk=p(st.rekey), segs=s.max_segs: (  # noqa: E731
        L.wgcs_rekey_sent_host(peer, p(s.count), p(s.status), jk, s.n, segs, NOW, *rows, *non, rk))
    for kw in (dict(peer=None), dict(jk=None), dict(rk=None), dict(segs=0)):
        assert sent(**kw) == bad, kw
    assert L.wgcs_rekey_received_host(None, 1, 1, NOW, *rows, p(st.rekey)) == bad
    assert L.wgcs_rekey_received_host(p(v.groups), 1, 1, NOW, *rows, None) == bad
    assert L.wgcs_rekey_received_host(p(v.groups), 1 << 20, 1 << 9, NOW, *rows, p(st.rekey)) == bad
    assert L.wgcs_rekey_responded_host(None, p(e.gate), 1, NOW, p(st.rekey), 4) == bad
    assert L.wgcs_rekey_responded_host(p(e.resp), None, 1, NOW, p(st.rekey), 4) == bad
    assert L.wgcs_rekey_responded_host(p(e.resp), p(e.gate), 1, NOW, None, 4) == bad
    start = lambda rk=p(st.rekey), hp=p(st.hs_peers), n=4, tk=p(q.tickets), nt=q.n_tickets, sa=p(o["start"]), sp=p(o["start_peer"]), cn=p(o["count"]), ss=p(o["status"]), rs=p(o["reasons"]): (  # noqa: E731
        L.wgcs_rekey_start_host(NOW, rk, hp, n, tk, nt, sa, sp, cn, ss, rs))
    for kw in (dict(rk=None), dict(hp=None), dict(tk=None), dict(sa=None), dict(sp=None), dict(cn=None), dict(ss=None),
               dict(rs=None), dict(n=(1 << 24) + 1), dict(nt=(1 << 28) + 1), dict(sa=p(q.tickets))):
        assert start(**kw) == bad, kw
    # n == 0 is a no-op whatever else is given
    assert L.wgcs_rekey_recv_gate_host(None, 0, NOW, None, 16, *rows) == 0
    assert gate(n=0, peer=None, count=None, status=None, o=None) == 0
    assert L.wgcs_rekey_sent_host(None, None, None, None, 0, 4, NOW, *rows, *non, None) == 0
    assert L.wgcs_rekey_received_host(None, 0, 8, NOW, *rows, None) == 0 and L.wgcs_rekey_received_host(None, 8, 0, NOW, *rows, None) == 0
    assert L.wgcs_rekey_responded_host(None, None, 0, NOW, None, 4) == 0
    assert (out == 77).all() and st.rekey.tobytes() == w.rekey.tobytes()
    assert all(x.view(np.uint8).min() == cases.FILL == x.view(np.uint8).max() for x in o.values())
    # no peer rows: the count is zero and every descriptor is the tail
    assert start(n=0, rk=None, hp=None, ss=None, rs=None) == 0 and o["count"][0] == 0
    assert (o["start"]["state_row"] == 0xFFFFFFFF).all() and (o["start_peer"] == PEER_NONE).all()


def test_layout_constants_and_error_texts():
    assert rekey.REKEY_DTYPE.itemsize == 16 and rekey.REKEY_DTYPE.fields["want"][1] == 8
    assert KEYPAIRS_DTYPE.fields["current"][1] == 24 and HS_START_DTYPE.fields["cookie"][1] == 72
    assert (rekey.REJECT_AFTER_TIME_NS, rekey.REKEY_AFTER_TIME_NS, rekey.REKEY_TIMEOUT_NS, rekey.KEEPALIVE_TIMEOUT_NS) == (
        ref.RejectAfterTime, ref.RekeyAfterTime, ref.RekeyTimeout, ref.KeepaliveTimeout)
    assert rekey.REKEY_AFTER_MESSAGES == ref.RekeyAfterMessages == 1 << 60 and _lib.REJECT_AFTER_MESSAGES == ref.RejectAfterMessages
    assert (rekey.SESSION_EXPIRED, rekey.ERR_KEY_EXPIRED, rekey.ERR_REKEY_TIMEOUT, rekey.HS_STARTED) == (
        SESSION_EXPIRED, ERR_KEY_EXPIRED, ERR_REKEY_TIMEOUT, HS_STARTED) == (0xFFFFFFFD, -26, -27, 9)
    assert _lib.load().wgcs_abi_version() == 2
    texts = {_lib.load().wgcs_strerror(c) for c in (ERR_KEY_EXPIRED, ERR_REKEY_TIMEOUT)}
    assert len(texts) == 2 and b"unknown status" not in texts
    t = rekey.rekey_table(3, NOW)
    assert t["last_sent_ns"].tolist() == [NOW - 6 * SECOND] * 3 and not t["want"].any() and not t["flags"].any()


