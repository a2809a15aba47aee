"""The peer timers on the GPU (the seven wgcs_timers_*_batch calls; the kernels
of timers_kernels.hip) against the host forms of timers.cpp, byte for byte:
the wgcs_timers and wgcs_rekey tables, the keypair tables and every output of
the call.  tests/test_timers_ref.py pins the host forms to the restatement of
the reference.

Every output buffer is filled with a sentinel first and is longer than the
call's rows; every read-only input is compared with its upload afterwards."""
import numpy as np
import pytest
import torch

import timers_cases as cases
from timers_cases import D, NOW
from timers_ref import (ACT_DEFERRED, ACT_KEEPALIVE, ACTIVE, GROUP_DATA, HS_BEGUN, HS_INITIATED, HS_RESPONDED,
                        KEEPALIVE_NOW, NEED_ANOTHER, PEER_NONE, SECOND, WANT_NEW_HANDSHAKE, fired)
from wireguard_amd import _lib, keystate, timers

pytestmark = pytest.mark.gpu

SPARE = 3  # rows of every output past the call's: they keep their fill
STATE_DTYPES = dict(timers=timers.TIMERS_DTYPE, rekey=timers.REKEY_DTYPE, kp=timers.KEYPAIRS_DTYPE,
                    slots=timers.SESSION_SLOT_DTYPE, peer_keys=timers.SESSION_SLOT_DTYPE, keys=timers.AEAD_KEY_DTYPE,
                    key_peer=np.uint32)


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def inputs_of(w, s):
    """the arrays the call only reads"""
    if s.kind == "sent":
        return dict(sizes=s.sizes, peer=s.peer, count=s.count, status=s.status, job_key=s.job_key, peer_rows=w.peer_rows)
    if s.kind == "rcvd":
        return dict(groups=s.groups, peer_rows=w.peer_rows)
    if s.kind == "init":
        return dict(reasons=s.reasons, start_peer=s.start_peer, init_status=s.init_status)
    if s.kind == "resp":
        return dict(resp=s.resp, gate=s.gate)
    if s.kind == "fin":
        return dict(arena=s.arena, pkts=s.pkts, gate=s.gate, begun=s.begun, hs_slots=w.hs_slots, states=w.states)
    if s.kind == "rot":
        return dict(pkts=s.pkts, rotated=s.rotated, peer_rows=w.peer_rows)
    return dict(table=w.table, **({} if s.staged is None else dict(staged=s.staged)))


def device_step(dev, w, st, s, stream=None):
    """(the outputs whole, fills included; the state tables afterwards); st is left alone"""
    ins = inputs_of(w, s)
    di = {k: up(v) for k, v in ins.items()}
    do = {k: up(v) for k, v in cases.fresh_outputs(w, s, SPARE).items()}
    ds = {k: up(getattr(st, k)) for k in cases.STATE}
    n_peers, n_keys = w.n_peers, len(st.key_peer)
    torch.cuda.synchronize()
    if s.kind == "sent":
        timers.sent_batch(dev, di["sizes"], di["peer"], di["count"], di["status"], di["job_key"], s.max_segs, s.now,
                          s.jitter_seed, di["peer_rows"], ds["timers"], stream=stream, n_jobs=s.n, n_ids=w.n_ids,
                          n_peers=n_peers)
    elif s.kind == "rcvd":
        timers.received_batch(dev, di["groups"], s.calls_per_batch, s.now, di["peer_rows"], ds["timers"], stream=stream,
                              n_batches=s.n // s.calls_per_batch, n_ids=w.n_ids, n_peers=n_peers)
    elif s.kind == "init":
        timers.initiated_batch(dev, di["reasons"], di["start_peer"], di["init_status"], s.now, s.jitter_seed, ds["timers"],
                               stream=stream, n_tickets=s.n, n_peers=n_peers)
    elif s.kind == "resp":
        timers.responded_batch(dev, di["resp"], di["gate"], s.now, ds["timers"], stream=stream, n=s.n, n_peers=n_peers)
    elif s.kind == "fin":
        timers.finished_batch(dev, di["arena"], di["pkts"], di["gate"], di["begun"], s.now, di["hs_slots"], di["states"],
                              ds["timers"], ds["rekey"], stream=stream, n=s.n, n_hs_slots=len(w.hs_slots),
                              n_states=len(w.states), n_peers=n_peers)
    elif s.kind == "rot":
        timers.rotated_batch(dev, di["pkts"], di["rotated"], s.now, ds["key_peer"], di["peer_rows"], ds["timers"],
                             ds["rekey"], stream=stream, n=s.n, n_keys=n_keys, n_ids=w.n_ids, n_peers=n_peers)
    else:
        d_work = torch.full((keystate.work_bytes(n_peers),), 0x77, dtype=torch.uint8, device="cuda")
        timers.expire_batch(dev, s.now, ds["timers"], ds["rekey"], di["table"], di.get("staged"), ds["kp"], ds["slots"],
                            ds["peer_keys"], ds["keys"], ds["key_peer"], do["ka_peer"], do["ka_count"], do["ka_sizes"],
                            do["ka_status"], do["n_ka"], do["actions"], d_work, stream=stream, n_peers=n_peers,
                            n_slots=len(st.slots), n_peer_slots=len(st.peer_keys), n_keys=n_keys, n_ka_max=s.n_ka_max)
    torch.cuda.synchronize()
    for k, a in ins.items():
        assert di[k].cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), f"{k} was written"
    return ({k: v.cpu().numpy().view(cases.OUT_DTYPES[k]) for k, v in do.items()},
            {k: v.cpu().numpy().view(STATE_DTYPES[k]) for k, v in ds.items()})


def check_case(dev, c):
    w, st, outs = c.world, cases.state_of(c.world), []
    for k, s in enumerate(c.steps):
        got, got_state = device_step(dev, w, st, s)
        want = cases.run_host(w, st, s, spare=SPARE)  # st moves on
        where = f"{c.name} step {k} ({s.kind})"
        assert set(got) == set(want), where
        for name in want:
            assert got[name].tobytes() == want[name].tobytes(), f"{where}: {name}: got {got[name]}, want {want[name]}"
        for name in cases.STATE:
            assert got_state[name].tobytes() == getattr(st, name).tobytes(), (
                f"{where}: {name}: got {got_state[name]}, want {getattr(st, name)}")
        outs.append(got)
    return st, outs


NAMED = {c.name: c for c in cases.named()}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case_matches_the_host_form(dev, name):
    check_case(dev, NAMED[name])


def twice(dev, c):
    """the case on fresh tables, twice: the same bytes, whichever lane ran first"""
    st, outs = check_case(dev, c)
    st2, outs2 = check_case(dev, c)
    assert all(getattr(st, k).tobytes() == getattr(st2, k).tobytes() for k in cases.STATE)
    assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(outs, outs2) for k in a)
    return st, outs


def pending(st, row):
    return [i for i in range(5) if st.timers["pending"][row] >> i & 1]


def test_sent_one_peer_across_blocks(dev):
    """300 jobs x 4 slots on 40 peers, two blocks; row 17's jobs at 3, 70 and 290, the first a job of keepalives
    alone, so the atomics of one peer come from different blocks and only one lane arms newHandshake"""
    n, now = 300, NOW
    rng = np.random.default_rng(300)
    w = cases.world(40, 8, keepalive_interval_s=(np.arange(40) % 3) * 20)
    w.timers["pending"] = rng.integers(0, 32, 40)
    w.timers["pending"][17] = 0b00100
    w.timers["deadline_ns"] = now + rng.integers(1, 100, (40, 5)) * SECOND
    w.timers["flags"][::7] = 0  # not active
    ids = w.ids.tolist()
    others = [r for r in range(40) if r != 17]
    jobs = [(int(rng.choice([ids[int(rng.choice(others))], 11, w.n_ids + 7, PEER_NONE], p=[0.91, 0.03, 0.03, 0.03])),
             int(rng.choice([1, 2, 4, 0, 5], p=[0.3, 0.3, 0.3, 0.05, 0.05])), int(rng.choice([0, -8], p=[0.93, 0.07])),
             bool(rng.random() < 0.8), bool(rng.random() < 0.7)) for _ in range(n)]
    jobs[3], jobs[70], jobs[290] = (ids[17], 1, 0, True, False), (ids[17], 2, 0, True, True), (ids[17], 4, 0, True, True)
    st, _ = twice(dev, cases.case("sent_300", w, [cases.sent_step(jobs, now, seed=301, jitter_seed=77)]))
    assert pending(st, 17) == [0, 3] and st.timers["deadline_ns"][17, 3] == now + 40 * SECOND
    assert st.timers["deadline_ns"][17, 0] == now + 15 * SECOND + timers.jitter_ms(77, 17) * 1_000_000
    assert st.timers["pending"].tobytes() != w.timers["pending"].tobytes()
    assert st.timers["pending"][::7].tolist() == w.timers["pending"][::7].tolist()  # the inactive rows


def test_received_one_peer_in_both_batches(dev):
    """2 batches x 128 group rows; row 23 has a data group in both: the timer is armed and NEED_ANOTHER set"""
    now = NOW
    rng = np.random.default_rng(128)
    w = cases.world(40, 8, keepalive_interval_s=25)
    w.timers["pending"] = rng.integers(0, 32, 40)
    w.timers["pending"][23] = 0b00001
    ids = w.ids.tolist()
    others = [i for r, i in enumerate(ids) if r != 23]
    groups = [(int(rng.choice(others + [11, PEER_NONE])), int(rng.integers(-1, 200)), int(rng.integers(0, 2)))
              for _ in range(256)]
    groups[7], groups[128 + 9] = (ids[23], 4, GROUP_DATA), (ids[23], 130, GROUP_DATA)
    st, _ = twice(dev, cases.case("received_2x128", w, [cases.rcvd_step(groups, now, 128, seed=129)]))
    assert pending(st, 23) == [2, 3] and st.timers["flags"][23] == ACTIVE | NEED_ANOTHER
    assert st.timers["deadline_ns"][23, 2] == now + 10 * SECOND and st.timers["deadline_ns"][23, 3] == now + 25 * SECOND


def expire_world(rows=(3, 70, 255, 256, 290, 699), n_peers=700):
    """700 peer rows; sendKeepalive is due in the named rows, newHandshake in row 100, and row 300 owes a keepalive
    that its staged packets replace"""
    w = cases.world(n_peers, 8)
    for r in rows:
        cases.arm(w, r, 2, D - r)
    cases.arm(w, 100, 0, D)
    cases.arm(w, 500, 2, D + 1)  # not yet
    w.timers["flags"][300] |= KEEPALIVE_NOW
    return w


@pytest.mark.parametrize("room", [4, 8, 0])
def test_expire_ranks_cross_block_edges(dev, room):
    """700 peer rows, three blocks; owing rows at 3, 70, 255, 256, 290 and 699"""
    staged = np.zeros(700, np.uint32)
    staged[300] = 1
    st, (a, b) = twice(dev, cases.case(f"expire_700_{room}", expire_world(),
                                       [cases.exp_step(D, room, staged), cases.exp_step(D + 1, 8)]))
    rows, ids = [3, 70, 255, 256, 290, 699], expire_world().ids
    k = min(room, 6)
    assert a["ka_peer"][:room].tolist() == ids[rows[:k]].tolist() + [PEER_NONE] * (room - k) and a["n_ka"][0] == k
    assert a["ka_count"][:room].tolist() == [1] * k + [0] * (room - k)
    assert [int(a["actions"][r]) for r in rows] == [fired(2) | ACT_KEEPALIVE] * k + [fired(2) | ACT_DEFERRED] * (6 - k)
    assert a["actions"][100] == fired(0) and a["actions"][300] == 0 and a["actions"][500] == 0
    late = rows[k:] + [500]
    assert b["ka_peer"][:8].tolist() == ids[sorted(late)].tolist() + [PEER_NONE] * (8 - len(late)) and b["n_ka"][0] == len(late)
    assert (st.timers["flags"] & KEEPALIVE_NOW == 0).all() and st.rekey["want"][100] == WANT_NEW_HANDSHAKE
    assert np.count_nonzero(st.rekey["want"]) == 1


def test_expire_without_peer_rows(dev):
    """n_peers == 0: the count is zero and every job is the tail"""
    w = cases.world(1, 8)
    d = {k: torch.full((6,), 0x6EEEEEEE, dtype=torch.int32, device="cuda") for k in ("peer", "count", "sizes", "status", "n")}
    timers.expire_batch(dev, NOW, None, None, None, None, None, up(w.slots), up(w.peer_keys), up(w.keys), up(w.key_peer),
                        d["peer"], d["count"], d["sizes"], d["status"], d["n"], None, None, n_peers=0, n_slots=len(w.slots),
                        n_peer_slots=len(w.peer_keys), n_keys=8, n_ka_max=5, work_bytes=0)
    torch.cuda.synchronize()
    assert d["peer"].cpu().numpy().view(np.uint32).tolist() == [PEER_NONE] * 5 + [0x6EEEEEEE]
    for k in ("count", "sizes", "status"):
        assert d[k].cpu().tolist() == [0] * 5 + [0x6EEEEEEE], k
    assert d["n"].cpu().tolist() == [0] + [0x6EEEEEEE] * 5


def test_argument_errors_write_nothing(dev):
    c = NAMED["a_peer_id_without_a_row"]
    w, st = c.world, cases.state_of(c.world)
    sent, rcvd, init, resp, fin, rot = c.steps
    exp = cases.exp_step(D, 4, staged=[0, 0, 0, 0])
    d = {k: up(x) for k, x in dict(sizes=sent.sizes, peer=sent.peer, count=sent.count, status=sent.status,
                                   job_key=sent.job_key, peer_rows=w.peer_rows, groups=rcvd.groups, reasons=init.reasons,
                                   start_peer=init.start_peer, init_status=init.init_status, resp=resp.resp, gate=resp.gate,
                                   arena=fin.arena, pkts=fin.pkts, fgate=fin.gate, begun=fin.begun, hs_slots=w.hs_slots,
                                   states=w.states, rpkts=rot.pkts, rotated=rot.rotated, table=w.table, staged=exp.staged,
                                   **{k: getattr(st, k) for k in cases.STATE}).items()}
    before = {k: x.cpu().numpy().tobytes() for k, x in d.items()}
    o = {k: torch.full((8,), 12345, dtype=torch.int32, device="cuda") for k in cases.EXP_OUTS}
    d_work = torch.zeros(keystate.work_bytes(4) + 16, dtype=torch.uint8, device="cuda")
    rows = dict(peer_rows=d["peer_rows"], timers=d["timers"], n_ids=w.n_ids, n_peers=4)

    def call(fn, base):
        def f(**kw):
            a = dict(base)
            a.update(kw)
            fn(dev, **a)
        f.__name__ = fn.__name__
        return f

    f_sent = call(timers.sent_batch, dict(sizes=d["sizes"], peer=d["peer"], count=d["count"], status=d["status"],
                                          job_key=d["job_key"], max_segs=4, now_ns=D, jitter_seed=cases.JSEED, n_jobs=sent.n, **rows))
    f_rcvd = call(timers.received_batch, dict(groups=d["groups"], calls_per_batch=2, now_ns=D, n_batches=2, **rows))
    f_init = call(timers.initiated_batch, dict(reasons=d["reasons"], start_peer=d["start_peer"], init_status=d["init_status"],
                                               now_ns=D, jitter_seed=cases.JSEED, timers=d["timers"], n_tickets=init.n, n_peers=4))
    f_resp = call(timers.responded_batch, dict(resp=d["resp"], gate=d["gate"], now_ns=D, timers=d["timers"], n=resp.n,
                                               n_peers=4))
    f_fin = call(timers.finished_batch, dict(arena=d["arena"], pkts=d["pkts"], gate=d["fgate"], begun=d["begun"], now_ns=D,
                                             hs_slots=d["hs_slots"], states=d["states"], timers=d["timers"], rekey=d["rekey"],
                                             n=fin.n, n_hs_slots=len(w.hs_slots), n_states=len(w.states), n_peers=4))
    f_rot = call(timers.rotated_batch, dict(pkts=d["rpkts"], rotated=d["rotated"], now_ns=D, key_peer=d["key_peer"],
                                            rekey=d["rekey"], n=rot.n, n_keys=16, **rows))
    f_exp = call(timers.expire_batch, dict(now_ns=D - SECOND, timers=d["timers"], rekey=d["rekey"], table=d["table"],
                                           staged=d["staged"], kp=d["kp"], slots=d["slots"], peer_keys=d["peer_keys"],
                                           keys=d["keys"], key_peer=d["key_peer"], ka_peer=o["ka_peer"], ka_count=o["ka_count"],
                                           ka_sizes=o["ka_sizes"], ka_status=o["ka_status"], n_ka=o["n_ka"],
                                           actions=o["actions"], work=d_work, n_peers=4, n_slots=len(st.slots),
                                           n_peer_slots=len(st.peer_keys), n_keys=16, n_ka_max=4,
                                           work_bytes=keystate.work_bytes(4)))
    odd = lambda x, by=2: x.data_ptr() + by  # noqa: E731
    rows_bad = [dict(peer_rows=None), dict(timers=None), dict(peer_rows=odd(d["peer_rows"])), dict(timers=odd(d["timers"], 4)),
                dict(n_peers=(1 << 24) + 1)]
    calls = [(f_sent, rows_bad + [dict(sizes=None), dict(peer=None), dict(count=None), dict(status=None), dict(job_key=None),
                                  dict(max_segs=0), dict(n_jobs=1 << 27), dict(sizes=odd(d["sizes"])), dict(peer=odd(d["peer"])),
                                  dict(count=odd(d["count"])), dict(status=odd(d["status"])), dict(job_key=odd(d["job_key"]))]),
             (f_rcvd, rows_bad + [dict(groups=None), dict(n_batches=1 << 20, calls_per_batch=1 << 9),
                                  dict(groups=odd(d["groups"], 4))]),
             (f_init, [dict(reasons=None), dict(start_peer=None), dict(init_status=None), dict(timers=None),
                       dict(n_tickets=(1 << 28) + 1), dict(n_peers=(1 << 24) + 1), dict(reasons=odd(d["reasons"])),
                       dict(start_peer=odd(d["start_peer"])), dict(init_status=odd(d["init_status"])),
                       dict(timers=odd(d["timers"], 4))]),
             (f_resp, [dict(resp=None), dict(gate=None), dict(timers=None), dict(n=(1 << 28) + 1), dict(resp=odd(d["resp"])),
                       dict(gate=odd(d["gate"])), dict(timers=odd(d["timers"], 4))]),
             (f_fin, [dict(arena=None), dict(pkts=None), dict(gate=None), dict(begun=None), dict(hs_slots=None),
                      dict(states=None), dict(timers=None), dict(rekey=None), dict(n=(1 << 24) + 1), dict(n_hs_slots=3),
                      dict(pkts=odd(d["pkts"], 4)), dict(gate=odd(d["fgate"])), dict(begun=odd(d["begun"])),
                      dict(hs_slots=odd(d["hs_slots"])), dict(states=odd(d["states"])), dict(timers=odd(d["timers"], 4)),
                      dict(rekey=odd(d["rekey"], 4))]),
             (f_rot, rows_bad + [dict(pkts=None), dict(rotated=None), dict(key_peer=None), dict(rekey=None),
                                 dict(n=(1 << 28) + 1), dict(pkts=odd(d["rpkts"], 4)), dict(rotated=odd(d["rotated"])),
                                 dict(key_peer=odd(d["key_peer"])), dict(rekey=odd(d["rekey"], 4))]),
             (f_exp, [dict(timers=None), dict(rekey=None), dict(table=None), dict(kp=None), dict(slots=None),
                      dict(peer_keys=None), dict(keys=None), dict(key_peer=None), dict(ka_peer=None), dict(ka_count=None),
                      dict(ka_sizes=None), dict(ka_status=None), dict(n_ka=None), dict(actions=None), dict(work=None),
                      dict(work_bytes=64), dict(n_peers=(1 << 24) + 1), dict(n_ka_max=(1 << 24) + 1), dict(n_slots=3),
                      dict(n_peer_slots=6), dict(work=odd(d_work, 8)), dict(timers=odd(d["timers"], 4)),
                      dict(rekey=odd(d["rekey"], 4)), dict(table=odd(d["table"])), dict(staged=odd(d["staged"])),
                      dict(kp=odd(d["kp"])), dict(slots=odd(d["slots"])), dict(peer_keys=odd(d["peer_keys"])),
                      dict(keys=odd(d["keys"])), dict(key_peer=odd(d["key_peer"])), dict(ka_peer=odd(o["ka_peer"])),
                      dict(ka_count=odd(o["ka_count"])), dict(ka_sizes=odd(o["ka_sizes"])), dict(ka_status=odd(o["ka_status"])),
                      dict(n_ka=odd(o["n_ka"])), dict(actions=odd(o["actions"]))])]
    for fn, bad in calls:
        for kw in bad:
            with pytest.raises(_lib.WgcsError) as ei:
                fn(**kw)
            assert ei.value.code == _lib.ERR_INVALID_ARG, (fn.__name__, kw)
    L, p = dev.lib, lambda x: x.data_ptr()  # noqa: E731
    assert L.wgcs_timers_responded_batch(None, p(d["resp"]), p(d["gate"]), resp.n, D, p(d["timers"]), 4, None) == _lib.ERR_INVALID_ARG
    assert L.wgcs_timers_received_batch(None, p(d["groups"]), 2, 2, D, p(d["peer_rows"]), w.n_ids, p(d["timers"]), 4,
                                        None) == _lib.ERR_INVALID_ARG
    # n == 0 is a no-op, whatever else is given
    f_sent(n_jobs=0, sizes=None, peer=None, count=None, status=None, job_key=None)
    f_rcvd(n_batches=0, groups=None)
    f_rcvd(calls_per_batch=0, groups=None)
    f_init(n_peers=0, reasons=None, timers=None)
    f_resp(n=0, resp=None, gate=None)
    f_fin(n=0, arena=None, pkts=None, gate=None, begun=None)
    f_rot(n=0, pkts=None, rotated=None)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 12345).all() for t in o.values())
    assert {k: x.cpu().numpy().tobytes() for k, x in d.items()} == before
    # and the same arguments without the fault do the work
    want = cases.state_of(st)
    for s in c.steps:
        cases.run_host(w, want, s)
    f_sent(), f_rcvd(), f_init(), f_resp(), f_fin(), f_rot()
    torch.cuda.synchronize()
    assert d["timers"].cpu().numpy().tobytes() == want.timers.tobytes() and d["rekey"].cpu().numpy().tobytes() == want.rekey.tobytes()
    f_exp(now_ns=D + 30 * SECOND)
    torch.cuda.synchronize()
    h = cases.run_host(w, want, cases.exp_step(D + 30 * SECOND, 4, staged=[0, 0, 0, 0]), spare=4)
    for k in cases.EXP_OUTS:
        n = len(h[k]) - 4
        assert o[k].cpu().numpy().view(cases.OUT_DTYPES[k])[:n].tolist() == h[k][:n].tolist(), k
        assert (o[k].cpu().numpy()[n:] == 12345).all(), k
    assert all(d[k].cpu().numpy().tobytes() == getattr(want, k).tobytes() for k in cases.STATE)
    assert HS_BEGUN == _lib.HS_BEGUN and HS_INITIATED == _lib.HS_INITIATED and HS_RESPONDED == _lib.HS_RESPONDED
