"""The seven wgcs_timers_*_host forms (wireguard_amd/csrc/timers.cpp) against the
literal restatement of device/timers.go and the lines of send.go, receive.go
and peer.go that call it, in tests/timers_ref.py (CPU only).

After every step -- one call -- the wgcs_timers table, the words of the
wgcs_rekey table the section writes, the keypair tables and the call's own
outputs are compared, in all their bytes, with what the restatement renders.
The named cases are those of tests/timers_cases.py; the random sequences mix
the seven calls with the keypair rotation of wgcs_keypairs_*_host and the rekey
calls of wgcs_rekey_*_host under a clock that only moves forward, drawn from
the seeds fixed below."""
from collections import Counter

import numpy as np
import pytest

import keypairs_cases as kc
import timers_cases as cases
import timers_ref as ref
from keypairs_ref import NO_KEYPAIR
from rekey_cases import LIMIT
from timers_cases import D, I, NOW
from timers_ref import (ACT_DEFERRED, ACT_FLUSH_STAGED, ACT_GAVE_UP, ACT_KEEPALIVE, ACT_ZEROED, ACTIVE, CLEAR_SRC, GROUP_DATA,
                        HS_BEGUN, HS_FINISHED, HS_INITIATED, HS_RESPONDED, KEEPALIVE_NOW, NEED_ANOTHER, NO_KEY, PEER_NONE,
                        SECOND, WANT_NEW_HANDSHAKE, WANT_RETRY, fired)
from wireguard_amd import _lib, rekey, timers
from wireguard_amd.noise import HS_START_DTYPE
from wireguard_amd.timers import TIMERS_DTYPE

SEEDS = range(200)


def compare(where, w, st, d, s):
    want_rekey = st.rekey.copy()
    want = cases.run_ref(d, w, s, want_rekey, st.key_peer.copy())
    got = cases.run_host(w, st, s)
    assert set(got) == set(want) == set(cases.EXP_OUTS if s.kind == "exp" else ()), where
    for name in got:
        assert got[name].tobytes() == want[name].tobytes(), (*where, name, got[name], want[name])
    assert st.timers.tobytes() == d.render().tobytes(), (*where, "timers", st.timers, d.render())
    assert st.rekey.tobytes() == want_rekey.tobytes(), (*where, "rekey", st.rekey, want_rekey)
    for name, x in zip(cases.KEYPAIR_TABLES, d.kd.render(st.slots, st.peer_keys)):
        assert getattr(st, name).tobytes() == x.tobytes(), (*where, name)
    return got


def check(c):
    w, st = c.world, cases.state_of(c.world)
    d = cases.device_of(w, st)
    frozen = {k: getattr(w, k).tobytes() for k in ("table", "peer_rows", "states", "hs_slots")}
    outs = [compare((c.name, k, s.kind), w, st, d, s) for k, s in enumerate(c.steps)]
    assert {k: getattr(w, k).tobytes() for k in frozen} == frozen, c.name  # the read-only tables
    return st, outs


@pytest.mark.parametrize("c", cases.named(), ids=lambda c: c.name)
def test_named_case(c):
    check(c)


def named(name):
    return next(c for c in cases.named() if c.name == name)


def pending(st, row):
    return [i for i in range(5) if st.timers["pending"][row] >> i & 1]


def test_what_the_named_cases_reach():
    """The cases are what their names say: spot checks, independent of the restatement."""
    ids = cases.world().ids.tolist()
    for i, name in enumerate(ref.NAMES):  # due iff deadline <= now, and only a pending timer
        for tag, fires in (("minus_1", False), ("deadline", True), ("plus_1", True)):
            st, (o,) = check(named(f"{name}_at_{tag}"))
            assert bool(o["actions"][1] & fired(i)) == fires, (name, tag)
            assert o["actions"][[0, 2, 3]].tolist() == [0, 0, 0] and (i in pending(st, 1)) == (not fires)
            assert pending(st, 2) == [i] and st.timers["deadline_ns"][2, i] == D + 2
    st, (o,) = check(named("newHandshake_at_deadline"))
    assert st.rekey["want"].tolist() == [0, WANT_NEW_HANDSHAKE, 0, 0] and st.timers["flags"][1] == ACTIVE | CLEAR_SRC
    st, (o,) = check(named("keepalive_at_deadline"))
    assert o["ka_peer"].tolist() == [ids[1]] + [PEER_NONE] * 3 and o["ka_count"].tolist() == [1, 0, 0, 0]
    assert o["n_ka"].tolist() == [1] and o["actions"][1] == fired(3) | ACT_KEEPALIVE
    assert not o["ka_sizes"].any() and not o["ka_status"].any()
    st, (o,) = check(named("zeroOutKeys_at_deadline"))
    assert o["actions"][1] == fired(4) | ACT_ZEROED | ACT_FLUSH_STAGED and not st.kp[1:2].tobytes().strip(b"\0")[:-8].strip(b"\xff")

    st, (a, b) = check(named("attempts_at_18"))  # > MaxHandshakeAttempts is strict: the 19th attempt is made
    assert a["actions"][0] == fired(1) and st.timers["attempts"][0] == 19 and st.rekey["want"][0] == WANT_RETRY
    assert st.timers["flags"][0] == ACTIVE | CLEAR_SRC and b["actions"][0] == fired(2) | ACT_KEEPALIVE
    st, (a, b) = check(named("attempts_at_19"))
    assert a["actions"][0] == fired(1) | ACT_GAVE_UP | ACT_FLUSH_STAGED and st.timers["attempts"][0] == 19
    assert st.rekey["want"][0] == 0 and a["n_ka"][0] == 0 and st.timers["deadline_ns"][0, 4] == D + 540 * SECOND
    assert b["actions"][0] == fired(4) | ACT_ZEROED | ACT_FLUSH_STAGED and pending(st, 0) == []  # sendKeepalive was deleted

    st, outs = check(named("an_inactive_row"))
    assert outs[0]["actions"][1] == 0 and outs[0]["n_ka"][0] == 0 and pending(st, 1) == [0, 1, 2, 3, 4]
    assert st.timers["deadline_ns"][1].tolist() == [D] * 5 and st.timers["flags"][1] == KEEPALIVE_NOW | NEED_ANOTHER
    assert st.timers["last_handshake_ns"][1] == D  # timersHandshakeComplete's stores are not behind timersActive
    st, outs = check(named("a_clock_that_went_back"))
    assert not outs[4]["actions"].any() and pending(st, 0) == [1, 3, 4]
    assert outs[5]["actions"][0] == 0  # resendHandshake is due at D + 5 s + jitter at the earliest

    st, (o,) = check(named("two_timers_due_resend_first"))
    assert o["actions"][2] == fired(1) | ACT_GAVE_UP | ACT_FLUSH_STAGED and o["n_ka"][0] == 0
    st, (o,) = check(named("two_timers_due_keepalive_first"))
    assert o["actions"][2] == fired(1) | fired(2) | ACT_GAVE_UP | ACT_FLUSH_STAGED | ACT_KEEPALIVE and o["ka_peer"][0] == ids[2]
    st, (o,) = check(named("two_timers_due_tied"))  # a tie goes to the lower index: resendHandshake
    assert o["actions"][2] == fired(1) | ACT_GAVE_UP | ACT_FLUSH_STAGED and pending(st, 2) == [4]
    st, (o,) = check(named("three_timers_due"))
    assert o["actions"][0] == fired(0) | fired(3) | fired(4) | ACT_ZEROED | ACT_FLUSH_STAGED | ACT_KEEPALIVE

    st, (a, b) = check(named("need_another_set"))
    assert a["actions"][1] == b["actions"][1] == fired(2) | ACT_KEEPALIVE and st.timers["flags"][1] == ACTIVE
    assert st.timers["deadline_ns"][1, 2] == D + 10 * SECOND and pending(st, 1) == []
    st, (a, b) = check(named("need_another_clear"))
    assert a["actions"][1] == fired(2) | ACT_KEEPALIVE and b["actions"][1] == 0
    st, outs = check(named("interval_0"))
    assert outs[2]["actions"].tolist() == [0, 0, 0, fired(3)] and outs[2]["n_ka"][0] == 0 and not outs[3]["actions"].any()
    assert pending(st, 2) == []  # no keepalive timer without an interval; the reply cancelled newHandshake
    st, outs = check(named("interval_25"))
    assert not outs[2]["actions"].any()  # the keepalive that was sent moved row 3's timer on by its interval
    assert outs[3]["actions"].tolist() == [0, 0, fired(3) | ACT_KEEPALIVE, fired(3) | ACT_KEEPALIVE] and pending(st, 3) == []
    assert outs[3]["ka_peer"].tolist() == [ids[2], ids[3], PEER_NONE, PEER_NONE]
    assert st.timers["deadline_ns"][2, 3] == st.timers["deadline_ns"][3, 3] == D + 24 * SECOND

    for k in (1, 2, 3):
        st, (o,) = check(named(f"zero_out_keys_with_{k}"))
        assert o["actions"][1] == fired(4) | ACT_ZEROED | ACT_FLUSH_STAGED
        for name in ("previous", "current", "next"):
            assert not st.kp[name][1].tobytes().strip(b"\0")
        assert st.kp["current"][2]["recv_key"] == 7 and st.key_peer[6] == st.key_peer[7] == ids[2]
        assert (st.key_peer[:2 * k] == PEER_NONE).all() and not st.keys[:2 * k].tobytes().strip(b"\0")
        assert st.keys[6].tobytes().strip(b"\0") and st.keys[2 * k].tobytes().strip(b"\0")
        key_of = lambda slots, index: int(slots["key"][(slots["index"] == index) & (slots["key"] != 0xFFFFFFFF)][0])  # noqa: E731
        assert [key_of(st.slots, I[j]) for j in range(4)] == [NO_KEYPAIR] * 3 + [7]
        assert key_of(st.peer_keys, ids[1]) == NO_KEYPAIR and key_of(st.peer_keys, ids[2]) == 6

    st, (o,) = check(named("a_staged_peer"))
    assert o["ka_peer"].tolist() == [ids[0], ids[3], PEER_NONE, PEER_NONE] and o["n_ka"][0] == 2
    assert o["actions"].tolist() == [fired(2) | ACT_KEEPALIVE, fired(2), 0, ACT_KEEPALIVE]
    assert st.timers["flags"].tolist() == [ACTIVE] * 4  # the staged peer's SendKeepalive is done: its packets go out
    st, (a, b, c) = check(named("n_ka_max_0"))
    assert a["actions"].tolist() == [fired(2) | ACT_DEFERRED] * 4 and b["actions"].tolist() == [ACT_DEFERRED] * 4
    assert a["n_ka"][0] == 0 and c["ka_peer"].tolist() == ids + [PEER_NONE] * 2 and c["n_ka"][0] == 4
    assert st.timers["flags"].tolist() == [ACTIVE] * 4
    st, (a, b, c) = check(named("n_ka_max_less"))
    assert a["actions"].tolist() == [fired(2) | ACT_KEEPALIVE] * 2 + [fired(2) | ACT_DEFERRED] * 2 and a["ka_peer"].tolist() == ids[:2]
    assert b["actions"].tolist() == [0, 0, ACT_KEEPALIVE, ACT_KEEPALIVE] and b["ka_peer"].tolist() == ids[2:] and c["n_ka"][0] == 0
    st, (a, b, c) = check(named("n_ka_max_more"))
    assert a["ka_peer"].tolist() == ids + [PEER_NONE] * 2 and a["ka_count"].tolist() == [1] * 4 + [0] * 2 and not b["actions"].any()

    st, outs = check(named("a_peer_id_without_a_row"))
    assert pending(st, 0) == [] and pending(st, 1) == [0, 3] and pending(st, 2) == [3, 4] and pending(st, 3) == [1, 3, 4]
    assert st.timers["flags"].tolist() == [ACTIVE, ACTIVE, ACTIVE | KEEPALIVE_NOW, ACTIVE]
    st, outs = check(named("two_data_groups_of_one_peer_in_one_call"))
    c = named("two_data_groups_of_one_peer_in_one_call")
    s1 = cases.state_of(c.world)
    cases.run_host(c.world, s1, c.steps[0])
    assert s1.timers["flags"].tolist() == [ACTIVE, ACTIVE | NEED_ANOTHER, ACTIVE, ACTIVE]
    assert pending(s1, 0) == pending(s1, 1) == [2] and s1.timers["deadline_ns"][1, 2] == D + 10 * SECOND
    assert [o["n_ka"][0] for o in outs[2:]] == [2, 2, 0]  # both re-arm once: row 0's second group came a call later

    st, outs = check(named("sent_data_and_keepalive"))
    j0, j1 = timers.jitter_ms(cases.JSEED, 0), timers.jitter_ms(cases.JSEED + 1, 1)
    assert st.timers["deadline_ns"][0, 0] == D + 15 * SECOND + j0 * 1_000_000  # not re-armed by the second call
    assert st.timers["deadline_ns"][1, 0] == D + 16 * SECOND + j1 * 1_000_000 and pending(st, 2) == []
    assert outs[2]["actions"][0] == fired(0) and st.rekey["want"].tolist() == [WANT_NEW_HANDSHAKE, 0, 0, 0]
    st, outs = check(named("initiated_fresh_and_retry"))
    c = named("initiated_fresh_and_retry")
    s1 = cases.state_of(c.world)
    cases.run_host(c.world, s1, c.steps[0])
    assert s1.timers["attempts"].tolist() == [3, 0, 5, 0] and pending(s1, 3) == []  # merged wishes count as fresh
    assert s1.timers["deadline_ns"][0, 1] == D + 5 * SECOND + timers.jitter_ms(cases.JSEED, 0) * 1_000_000
    assert st.timers["attempts"].tolist() == [4, 1, 5, 0] and st.rekey["want"].tolist() == [WANT_RETRY, WANT_RETRY, 0, 0]
    st, outs = check(named("responded"))
    both = fired(3) | fired(4) | ACT_ZEROED | ACT_FLUSH_STAGED | ACT_KEEPALIVE
    assert outs[1]["actions"].tolist() == [0, both, both, 0] and pending(st, 0) == pending(st, 1) == []
    st, outs = check(named("finished_then_a_keepalive"))
    assert st.timers["attempts"][1] == 0 and st.rekey["flags"].tolist() == [0, 0, 1, 0]
    assert st.timers["last_handshake_ns"].tolist() == [0, D, 0, 0] and pending(st, 1) == [3, 4]
    assert outs[1]["ka_peer"][0] == ids[1] and outs[1]["actions"][1] == ACT_KEEPALIVE and not outs[2]["actions"].any()
    st, outs = check(named("rotated"))
    assert st.timers["attempts"][2] == 0 and st.rekey["flags"][2] == 0 and st.timers["last_handshake_ns"][2] == D
    assert not outs[1]["actions"].any()


def random_sequence(seed: int):
    """(the world, its steps): calls over 6 peers under a clock that only moves forward, by steps between a
    second and nine minutes.  Handshakes planned ahead are begun and promoted by the rotation calls, each
    followed by the timer call that sits behind it; send batches pass the rekey gate, a send-assign that keeps
    four jobs in five, and the sent calls; receive batches leave groups; expire is followed by start and by an
    initiate that now and then fails; the host stages packets for a peer now and then; and in some sequences
    one peer's handshake is lost over and over, until its retries are used up and its keys are thrown away."""
    rng = np.random.default_rng(7000 + seed)
    n_peers, n_hs, n_keys = 6, 16, 36
    idx = [int(x) for x in rng.choice(1 << 20, n_hs, replace=False) + 1]
    plan = [(idx[h], int(rng.integers(0, n_peers)), 2 * h, 2 * h + 1, bool(rng.random() < 0.5)) for h in range(n_hs)]
    w = cases.world(n_peers, n_keys, idx, handshakes=[p[:4] for p in plan if p[4]], seed=seed,
                    keepalive_interval_s=[0, 25, 0, 3, 0, 0])
    ids = w.ids.tolist()
    steps, h, now = [], 0, NOW
    any_id = lambda: int(rng.choice(ids + ids + [11, w.n_ids + 3, PEER_NONE]))  # noqa: E731

    def expire_and_start(tickets=None):
        steps.append(("staged", (rng.random(n_peers) < 0.15).astype(np.uint32) if rng.random() < 0.5 else None))
        steps.append(("exp", int(rng.choice([0, 1, 2, 6]))))
        steps.append(("start", int(rng.integers(0, 4)) if tickets is None else tickets,
                      rng.random(6) < (0.85 if tickets is None else 2)))

    lossy = int(rng.integers(0, n_peers)) if seed % 4 == 0 else None
    for k in range(int(rng.integers(14, 24))):
        now += int(rng.choice([1, 1, 1, 3, 5, 6, 11, 16, 26, 60, 125, 541])) * SECOND + int(rng.integers(0, 1000))
        steps.append(("clock", now))
        u, sd = rng.random(), 1000 * seed + k
        if u < 0.20 and h < n_hs:
            li, row, sk, rk, initiator = plan[h]
            h += 1
            steps.append(("begin", kc.init_step([li], now=now, seed=sd) if initiator else
                          kc.resp_step([(row, li, sk, rk)], now=now, seed=sd)))
        elif u < 0.30:
            steps.append(("recv", kc.recv_step([(2 * int(rng.integers(0, max(h, 1))) + 1, 100) for _ in range(3)], seed=sd)))
        elif u < 0.55:
            steps.append(("send", [(any_id(), int(rng.choice([1, 2, 4, 0, 5])), int(rng.choice([0, 0, 0, 0, -8])),
                                    bool(rng.random() < 0.8), bool(rng.random() < 0.75))
                                   for _ in range(int(rng.integers(1, 7)))], sd))
        elif u < 0.75:
            steps.append(("rcvd", [(any_id(), int(rng.integers(-1, 5)), int(rng.integers(0, 2)))
                                   for _ in range(2 * int(rng.integers(1, 4)))], sd))
        else:
            expire_and_start()
    if lossy is not None:  # the initiation is lost 20 times running, then nothing is heard for ten minutes
        steps.append(("want", lossy))
        for k in range(21):
            steps.append(("clock", now))
            expire_and_start(tickets=6)
            now += 5 * SECOND + 400_000_000
        for wait in (541, 60):
            now += wait * SECOND
            steps.append(("clock", now))
            expire_and_start()
    return w, steps


def test_random_sequences():
    seen = Counter()
    for seed in SEEDS:
        w, steps = random_sequence(seed)
        st = cases.state_of(w)
        d = cases.device_of(w, st)
        t = {k: getattr(st, k) for k in cases.KEYPAIR_TABLES}  # the rotation's tables, in place
        now, staged, k = NOW, None, 0

        def timer_call(s):
            nonlocal k
            k += 1
            return compare((seed, k, s.kind), w, st, d, s)

        for what, *a in steps:
            if what == "clock":
                now = a[0]
            elif what == "staged":
                staged = a[0]
            elif what == "want":  # the host's own wish, a stream-ordered write
                st.rekey["want"][a[0]] |= 1
            elif what == "begin":
                s = a[0]
                if s.kind == "resp":  # respond -> responded -> begin
                    rekey.responded_host(s.resp, s.gate, now, st.rekey)
                    timer_call(cases.SimpleNamespace(kind="resp", now=now, resp=s.resp, gate=s.gate, n=s.n))
                begun = kc.run_host(w, t, s)
                assert begun.tobytes() == kc.run_ref(w, d.kd, s).tobytes()
                if s.kind == "init":  # finish -> begin -> finished
                    timer_call(cases.SimpleNamespace(kind="fin", now=now, arena=s.arena, pkts=s.pkts, gate=s.gate,
                                                     begun=begun, n=s.n))
                    seen["begun"] += int((begun == HS_BEGUN).sum())
            elif what == "recv":
                s = a[0]
                rotated = kc.run_host(w, t, s)
                assert rotated.tobytes() == kc.run_ref(w, d.kd, s).tobytes()
                timer_call(cases.SimpleNamespace(kind="rot", now=now, pkts=s.pkts, rotated=rotated, n=s.n))
                seen["rotated"] += int(rotated.sum())
            elif what == "send":
                s = cases.sent_step(a[0], now, seed=a[1], jitter_seed=a[1])
                status = np.zeros(s.n, np.int32)
                nonce = np.zeros(w.n_keys, np.uint64)
                rekey.send_gate_host(s.peer, s.count, s.status, s.max_segs, now, w.peer_rows, st.kp, nonce, LIMIT, st.rekey,
                                     status)
                s.status, s.job_key = status, np.where(status == 0, s.job_key, NO_KEY).astype(np.uint32)
                rekey.sent_host(s.peer, s.count, s.status, s.job_key, s.max_segs, now, w.peer_rows, st.kp, nonce, LIMIT,
                                st.rekey)
                timer_call(s)
            elif what == "rcvd":
                s = cases.rcvd_step(a[0], now, 2, seed=a[1])
                rekey.received_host(s.groups, 2, now, w.peer_rows, st.kp, st.rekey)
                timer_call(s)
            elif what == "exp":
                o = timer_call(cases.exp_step(now, a[0], staged))
                for bit, name in ((ACT_KEEPALIVE, "job"), (ACT_DEFERRED, "deferred"), (ACT_FLUSH_STAGED, "flush"),
                                  (ACT_ZEROED, "zeroed"), (ACT_GAVE_UP, "gave_up"), *((fired(i), n) for i, n in enumerate(ref.NAMES))):
                    seen[name] += int((o["actions"] & bit != 0).sum())
            else:  # start -> initiate (which fails now and then) -> initiated
                n_tickets, ok = a
                tickets = np.zeros(n_tickets, HS_START_DTYPE)
                o = dict(start=np.zeros(n_tickets, HS_START_DTYPE), start_peer=np.zeros(n_tickets, np.uint32),
                         count=np.zeros(1, np.uint32), status=np.zeros(w.n_peers, np.int32),
                         reasons=np.zeros(w.n_peers, np.uint32))
                rekey.start_host(now, st.rekey, np.zeros(w.n_peers, rekey.HS_PEER_DTYPE), tickets, o["start"], o["start_peer"],
                                 o["count"], o["status"], o["reasons"])
                init_status = np.where((o["start_peer"] != PEER_NONE) & ok[:n_tickets], HS_INITIATED, -1).astype(np.int32)
                timer_call(cases.SimpleNamespace(kind="init", now=now, reasons=o["reasons"], start_peer=o["start_peer"],
                                                 init_status=init_status, jitter_seed=seed, n=n_tickets))
                seen["want_new"] += int((o["reasons"] & WANT_NEW_HANDSHAKE != 0).sum())
                seen["want_retry"] += int((o["reasons"] & WANT_RETRY != 0).sum())
    # the sequences reach what they are for; the outputs counted are the restatement's too (compare)
    need = ["job", "deferred", "flush", "zeroed", "gave_up", *ref.NAMES, "want_new", "want_retry", "begun", "rotated"]
    assert all(seen[k] >= 20 for k in need), ", ".join(f"{k}: {seen[k]}" for k in need)


def test_jitter_ms():
    L = _lib.load()
    for seed in (0, 1, cases.JSEED, 0xFFFFFFFF):
        got = [L.wgcs_timers_jitter_ms(seed, r) for r in range(4096)]
        assert got == [timers.jitter_ms(seed, r) for r in range(4096)] == [ref.jitter_ms(seed, r) for r in range(4096)]
        assert all(0 <= x < 334 for x in got)
        assert len({ref.jitter_ms(seed, r) for r in range(4096)}) >= 300, seed
    assert L.wgcs_timers_jitter_ms(7, 0xFFFFFFFF) == ref.jitter_ms(7, 0xFFFFFFFF)


def test_host_forms_refuse_bad_arguments():
    c = named("a_peer_id_without_a_row")
    w, st = c.world, cases.state_of(c.world)
    sent, rcvd, init, resp, fin, rot = c.steps
    exp = cases.exp_step(D, 4, staged=[0, 0, 0, 0])
    o = cases.fresh_outputs(w, exp)
    L, bad = _lib.load(), _lib.ERR_INVALID_ARG
    p = lambda x: x.ctypes.data  # noqa: E731
    rows = lambda tm=p(st.timers), n=4: (p(w.peer_rows), w.n_ids, tm, n)  # noqa: E731
    f_sent = lambda sz=p(sent.sizes), pe=p(sent.peer), c=p(sent.count), s=p(sent.status), jk=p(sent.job_key), n=sent.n, segs=4, r=rows(): (  # noqa: E731
        L.wgcs_timers_sent_host(sz, pe, c, s, jk, n, segs, D, 1, *r))
    for kw in (dict(sz=None), dict(pe=None), dict(c=None), dict(s=None), dict(jk=None), dict(segs=0), dict(n=1 << 27),
               dict(r=rows(tm=None)), dict(r=(None, w.n_ids, p(st.timers), 4)), dict(r=rows(n=(1 << 24) + 1))):
        assert f_sent(**kw) == bad, kw
    assert L.wgcs_timers_received_host(None, 1, 1, D, *rows()) == bad
    assert L.wgcs_timers_received_host(p(rcvd.groups), 1, 1, D, *rows(tm=None)) == bad
    assert L.wgcs_timers_received_host(p(rcvd.groups), 1 << 20, 1 << 9, D, *rows()) == bad
    f_init = lambda why=p(init.reasons), sp=p(init.start_peer), s=p(init.init_status), n=init.n, tm=p(st.timers), np_=4: (  # noqa: E731
        L.wgcs_timers_initiated_host(why, sp, s, n, D, 1, tm, np_))
    for kw in (dict(why=None), dict(sp=None), dict(s=None), dict(tm=None), dict(n=(1 << 28) + 1), dict(np_=(1 << 24) + 1)):
        assert f_init(**kw) == bad, kw
    assert L.wgcs_timers_responded_host(None, p(resp.gate), 1, D, p(st.timers), 4) == bad
    assert L.wgcs_timers_responded_host(p(resp.resp), None, 1, D, p(st.timers), 4) == bad
    assert L.wgcs_timers_responded_host(p(resp.resp), p(resp.gate), 1, D, None, 4) == bad
    assert L.wgcs_timers_responded_host(p(resp.resp), p(resp.gate), (1 << 28) + 1, D, p(st.timers), 4) == bad
    f_fin = lambda a=p(fin.arena), pk=p(fin.pkts), g=p(fin.gate), b=p(fin.begun), n=fin.n, hs=p(w.hs_slots), nh=len(w.hs_slots), s=p(w.states), tm=p(st.timers), rk=p(st.rekey): (  # noqa: E731
        L.wgcs_timers_finished_host(a, pk, g, b, n, D, hs, nh, s, len(w.states), tm, rk, 4))
    for kw in (dict(a=None), dict(pk=None), dict(g=None), dict(b=None), dict(hs=None), dict(s=None), dict(tm=None),
               dict(rk=None), dict(nh=3), dict(n=(1 << 24) + 1)):
        assert f_fin(**kw) == bad, kw
    f_rot = lambda pk=p(rot.pkts), ro=p(rot.rotated), n=rot.n, kp=p(st.key_peer), r=rows()[:2], tm=p(st.timers), rk=p(st.rekey): (  # noqa: E731
        L.wgcs_timers_rotated_host(pk, ro, n, D, kp, 16, *r, tm, rk, 4))
    for kw in (dict(pk=None), dict(ro=None), dict(kp=None), dict(r=(None, w.n_ids)), dict(tm=None), dict(rk=None),
               dict(n=(1 << 28) + 1)):
        assert f_rot(**kw) == bad, kw

    def f_exp(**kw):
        a = dict(tm=p(st.timers), rk=p(st.rekey), tb=p(w.table), n=4, sg=p(exp.staged), kp=p(st.kp), sl=p(st.slots),
                 ns=len(st.slots), pk=p(st.peer_keys), nps=len(st.peer_keys), ks=p(st.keys), kpr=p(st.key_peer), nk=16, room=4,
                 kap=p(o["ka_peer"]), kac=p(o["ka_count"]), kas=p(o["ka_sizes"]), kat=p(o["ka_status"]), nka=p(o["n_ka"]),
                 act=p(o["actions"]))
        a.update(kw)
        return L.wgcs_timers_expire_host(D - SECOND, a["tm"], a["rk"], a["tb"], a["n"], a["sg"], a["kp"], a["sl"], a["ns"],
                                         a["pk"], a["nps"], a["ks"], a["kpr"], a["nk"], a["room"], a["kap"], a["kac"],
                                         a["kas"], a["kat"], a["nka"], a["act"])
    for kw in (dict(tm=None), dict(rk=None), dict(tb=None), dict(kp=None), dict(sl=None), dict(pk=None), dict(ks=None),
               dict(kpr=None), dict(kap=None), dict(kac=None), dict(kas=None), dict(kat=None), dict(nka=None), dict(act=None),
               dict(ns=3), dict(nps=6), dict(n=(1 << 24) + 1), dict(room=(1 << 24) + 1)):
        assert f_exp(**kw) == bad, kw
    # n == 0 is a no-op whatever else is given
    assert f_sent(n=0, sz=None, pe=None, c=None, s=None, jk=None) == 0
    assert L.wgcs_timers_received_host(None, 0, 8, D, *rows()) == 0 and L.wgcs_timers_received_host(None, 8, 0, D, *rows()) == 0
    assert f_init(np_=0, why=None, tm=None) == 0
    assert L.wgcs_timers_responded_host(None, None, 0, D, None, 4) == 0
    assert f_fin(n=0, a=None, pk=None, g=None, b=None) == 0 and f_rot(n=0, pk=None, ro=None) == 0
    assert all(getattr(st, k).tobytes() == getattr(w, k).tobytes() for k in cases.STATE)
    assert all(x.view(np.uint8).min() == cases.FILL == x.view(np.uint8).max() for x in o.values())
    # a NULL d_staged is "nobody has staged packets"; no peer rows: the count is zero and every job is the tail
    assert f_exp(sg=None) == 0 and o["n_ka"][0] == 0 and (o["ka_peer"] == PEER_NONE).all() and not o["actions"].any()
    o = cases.fresh_outputs(w, exp)
    assert f_exp(n=0, tm=None, rk=None, tb=None, kp=None, act=None) == 0 and o["n_ka"][0] == 0
    assert (o["ka_peer"] == PEER_NONE).all() and not o["ka_count"].any() and (o["actions"].view(np.uint8) == cases.FILL).all()


def test_layout_constants_and_start_takes_the_new_wishes():
    assert TIMERS_DTYPE.itemsize == 64 and TIMERS_DTYPE.fields["last_handshake_ns"][1] == 40
    assert [TIMERS_DTYPE.fields[k][1] for k in ("pending", "attempts", "flags", "keepalive_interval_s")] == [48, 52, 56, 60]
    assert (timers.TIMERS_ACTIVE, timers.TIMERS_NEED_ANOTHER, timers.TIMERS_CLEAR_SRC, timers.TIMERS_KEEPALIVE_NOW) == (
        ACTIVE, NEED_ANOTHER, CLEAR_SRC, KEEPALIVE_NOW)
    assert (timers.REKEY_WANT_NEW_HANDSHAKE, timers.REKEY_WANT_RETRY) == (WANT_NEW_HANDSHAKE, WANT_RETRY) == (0x80, 0x100)
    assert (timers.TIMERS_ACT_KEEPALIVE, timers.TIMERS_ACT_DEFERRED, timers.TIMERS_ACT_FLUSH_STAGED, timers.TIMERS_ACT_ZEROED,
            timers.TIMERS_ACT_GAVE_UP) == (ACT_KEEPALIVE, ACT_DEFERRED, ACT_FLUSH_STAGED, ACT_ZEROED, ACT_GAVE_UP)
    assert timers.TIMERS_MAX_ATTEMPTS == ref.MaxHandshakeAttempts == 18 and timers.TIMERS_JITTER_MAX_MS == 334
    assert timers.TIMERS_ZERO_KEYS_NS == 3 * ref.RejectAfterTime and _lib.load().wgcs_abi_version() == 2
    assert [timers.TIMER_NEW_HANDSHAKE, timers.TIMER_RESEND_HANDSHAKE, timers.TIMER_SEND_KEEPALIVE, timers.TIMER_KEEPALIVE,
            timers.TIMER_ZERO_OUT_KEYS] == list(range(5)) == [ref.NAMES.index(n) for n in ref.NAMES]
    t = timers.timers_table(3, [0, 25, 7])
    assert t["flags"].tolist() == [ACTIVE] * 3 and t["keepalive_interval_s"].tolist() == [0, 25, 7] and not t["pending"].any()
    assert not timers.timers_table(2, active=False)["flags"].any()
    # wgcs_rekey_start_batch's rule needs no change: want is copied as it stood and any bit is a wish
    rk = rekey.rekey_table(2, NOW)
    rk["want"] = [WANT_NEW_HANDSHAKE, WANT_RETRY]
    o = dict(start=np.zeros(2, HS_START_DTYPE), start_peer=np.zeros(2, np.uint32), count=np.zeros(1, np.uint32),
             status=np.zeros(2, np.int32), reasons=np.zeros(2, np.uint32))
    rekey.start_host(NOW, rk, np.zeros(2, rekey.HS_PEER_DTYPE), np.zeros(2, HS_START_DTYPE), o["start"], o["start_peer"],
                     o["count"], o["status"], o["reasons"])
    assert o["reasons"].tolist() == [WANT_NEW_HANDSHAKE, WANT_RETRY] and o["status"].tolist() == [9, 9] and not rk["want"].any()
    assert GROUP_DATA == _lib.GROUP_DATA and HS_RESPONDED == _lib.HS_RESPONDED and HS_FINISHED == _lib.HS_FINISHED
