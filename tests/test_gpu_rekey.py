"""Keypair expiry, the rekey rules and the start of a handshake on the GPU (the
six wgcs_rekey_*_batch calls; the kernels of rekey_kernels.hip) against the
host forms of rekey.cpp, byte for byte: the whole wgcs_rekey table and every
output of the call.  tests/test_rekey_ref.py pins the host forms to the
restatement of the reference.

Every output buffer is filled with a sentinel first and is longer than the
call's rows; every read-only input is compared with its upload afterwards."""
import numpy as np
import pytest
import torch

import rekey_cases as cases
from rekey_cases import LIMIT, NOW, T0
from rekey_ref import (ERR_BATCH_FULL, ERR_KEY_EXPIRED, HS_NONE, HS_RESPONDED, HS_STARTED, INITIATOR, LAST_MINUTE, NO_KEY,
                       PEER_NONE, SECOND, SESSION_EXPIRED, SET)
from wireguard_amd import _lib, keystate, rekey
from wireguard_amd.noise import HS_START_DTYPE
from wireguard_amd.rekey import REKEY_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

SPARE = 3  # rows of every output past the call's: they keep their fill
OUT_DTYPES = dict(pkts=AEAD_PKT_DTYPE, status_out=np.int32, status=np.int32, reasons=np.uint32, start=HS_START_DTYPE,
                  start_peer=np.uint32, count=np.uint32)


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def inputs_of(w, st, s):
    """the arrays the call only reads"""
    rows = dict(peer_rows=w.peer_rows, kp=st.kp)
    if s.kind == "recv":
        return dict(key_peer=st.key_peer, **rows)
    if s.kind == "gate":
        return dict(peer=s.peer, count=s.count, status_in=s.status_in, send_nonce=st.send_nonce, **rows)
    if s.kind == "sent":
        return dict(peer=s.peer, count=s.count, status=s.status, job_key=s.job_key, send_nonce=st.send_nonce, **rows)
    if s.kind == "rcvd":
        return dict(groups=s.groups, **rows)
    if s.kind == "resp":
        return dict(resp=s.resp, gate=s.gate)
    return dict(hs_peers=st.hs_peers, tickets=s.tickets)


def device_step(dev, w, st, s, stream=None):
    """(the outputs whole, fills included; the wgcs_rekey table afterwards); st is left alone"""
    ins = inputs_of(w, st, s)
    di = {k: up(v) for k, v in ins.items()}
    do = {k: up(v) for k, v in cases.fresh_outputs(w, s, SPARE).items()}
    d_rekey = up(st.rekey)
    n_peers, n_keys = w.n_peers, len(st.key_peer)
    torch.cuda.synchronize()
    if s.kind == "recv":
        rekey.recv_gate_batch(dev, do["pkts"], s.now, di["key_peer"], di["peer_rows"], di["kp"], stream=stream, n=s.n,
                              n_keys=n_keys, n_ids=w.n_ids, n_peers=n_peers)
    elif s.kind == "gate":
        rekey.send_gate_batch(dev, di["peer"], di["count"], di["status_in"], s.max_segs, s.now, di["peer_rows"], di["kp"],
                              di["send_nonce"], s.limit, d_rekey, do["status_out"], stream=stream, n_jobs=s.n,
                              n_ids=w.n_ids, n_peers=n_peers, n_keys=n_keys)
    elif s.kind == "sent":
        rekey.sent_batch(dev, di["peer"], di["count"], di["status"], di["job_key"], s.max_segs, s.now, di["peer_rows"],
                         di["kp"], di["send_nonce"], s.limit, d_rekey, stream=stream, n_jobs=s.n, n_ids=w.n_ids,
                         n_peers=n_peers, n_keys=n_keys)
    elif s.kind == "rcvd":
        rekey.received_batch(dev, di["groups"], s.calls_per_batch, s.now, di["peer_rows"], di["kp"], d_rekey,
                             stream=stream, n_batches=s.n // s.calls_per_batch, n_ids=w.n_ids, n_peers=n_peers)
    elif s.kind == "resp":
        rekey.responded_batch(dev, di["resp"], di["gate"], s.now, d_rekey, stream=stream, n=s.n, n_peers=n_peers)
    else:
        d_work = torch.full((keystate.work_bytes(n_peers),), 0x77, dtype=torch.uint8, device="cuda")
        rekey.start_batch(dev, s.now, d_rekey, di["hs_peers"], di["tickets"], do["start"], do["start_peer"], do["count"],
                          do["status"], do["reasons"], d_work, stream=stream, n_peers=n_peers, n_tickets=s.n_tickets)
    torch.cuda.synchronize()
    for k, a in ins.items():
        assert di[k].cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), f"{k} was written"
    return ({k: v.cpu().numpy().view(OUT_DTYPES[k]) for k, v in do.items()}, d_rekey.cpu().numpy().view(REKEY_DTYPE))


def check_case(dev, c):
    w, st, outs = c.world, cases.state_of(c.world), []
    for k, s in enumerate(c.steps):
        got, got_rekey = device_step(dev, w, st, s)
        want = cases.run_host(w, st, s, spare=SPARE)  # st.rekey moves on
        where = f"{c.name} step {k} ({s.kind})"
        assert set(got) == set(want), where
        for name in want:
            assert got[name].tobytes() == want[name].tobytes(), f"{where}: {name}: got {got[name]}, want {want[name]}"
        assert got_rekey.tobytes() == st.rekey.tobytes(), f"{where}: rekey: got {got_rekey}, want {st.rekey}"
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
    assert st.rekey.tobytes() == st2.rekey.tobytes()
    assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(outs, outs2) for k in a)
    return st, outs


def test_recv_gate_three_blocks(dev):
    """556 rows, three blocks; peer row 5's keypair is past RejectAfterTime and its packets sit at 0, 255, 256 and 555"""
    n, n_peers = 2 * 256 + 44, 12
    rng = np.random.default_rng(556)
    w = cases.world(n_peers, 4 * n_peers + 4)
    now = T0 + 181 * SECOND
    for r in range(n_peers):
        cases.put(w, r, "current", 4 * r, 4 * r + 1, T0 if r == 5 else now - 10 * SECOND, initiator=bool(r % 2))
        cases.put(w, r, "previous", 4 * r + 2, 4 * r + 3, T0 + SECOND)  # 180 s old at the call: equality passes
    keys = [int(rng.choice([4 * r + 1, 4 * r + 3, 4 * r, 4 * n_peers + int(rng.integers(0, 8))], p=[0.6, 0.2, 0.1, 0.1]))
            for r in rng.choice([r for r in range(n_peers) if r != 5], n)]
    for i in (0, 255, 256, 555):
        keys[i] = 21
    _, (o,) = twice(dev, cases.case("recv_gate_556", w, [cases.recv_step(keys, now, seed=557)]))
    got = o["pkts"]["key"]
    assert np.flatnonzero(got == SESSION_EXPIRED).tolist() == [0, 255, 256, 555]
    assert [int(k) for k in np.delete(got, [0, 255, 256, 555])] == [k for i, k in enumerate(keys) if i not in (0, 255, 256, 555)]


def send_world(now):
    """40 peers: row 17's current is 181 s old, row 23's is the initiator's and 130 s old, rows 30.. have none"""
    w = cases.world(40, 4 * 40 + 2)
    for r in range(30):
        age = {17: 181, 23: 130}.get(r, 10)
        cases.put(w, r, "current", 4 * r, 4 * r + 1, now - age * SECOND, initiator=r == 23 or r % 5 == 0)
    w.send_nonce[4 * 3] = LIMIT           # row 3 is out of nonces
    w.send_nonce[4 * 4] = (1 << 60) + 9   # row 4 is past RekeyAfterMessages
    return w


def test_send_gate_and_sent_one_peer_across_blocks(dev):
    """300 jobs x 4 slots on 40 peers, two blocks; row 17's jobs at 3, 70 and 290 and row 23's at 5, 71 and 291, so
    the atomicOrs of one peer come from different blocks"""
    n, now = 300, NOW
    rng = np.random.default_rng(300)
    w = send_world(now)
    ids = w.ids.tolist()
    others = [r for r in range(40) if r not in (17, 23)]
    jobs = [(int(rng.choice([ids[int(rng.choice(others))], 11, w.n_ids + 7, PEER_NONE], p=[0.91, 0.03, 0.03, 0.03])),
             int(rng.choice([1, 2, 4, 0, 5], p=[0.3, 0.3, 0.3, 0.05, 0.05])), int(rng.choice([0, -8], p=[0.93, 0.07])),
             bool(rng.random() < 0.8)) for _ in range(n)]
    for j in (3, 70, 290):
        jobs[j] = (ids[17], 2, 0, True)
    for j in (5, 71, 291):
        jobs[j] = (ids[23], 1 + j % 4, 0, j != 71)
    gate = cases.gate_step(jobs, now, seed=301)
    st, (o,) = twice(dev, cases.case("send_gate_300", w, [gate]))
    status = o["status_out"][:n]
    assert [int(status[j]) for j in (3, 70, 290, 5, 71, 291)] == [ERR_KEY_EXPIRED] * 3 + [0] * 3
    assert st.rekey["want"][17] == 4 and st.rekey["want"][23] == 0 and st.rekey["want"][3] == 2
    assert set(st.rekey["want"][30:].tolist()) <= {0, 1} and st.rekey["want"][30:].any()
    assert {0, -8, ERR_KEY_EXPIRED} == set(status.tolist())
    # sent over the gate's statuses, on the table the gate left
    w2 = send_world(now)
    w2.rekey = st.rekey.copy()
    sent = cases.sent_step(jobs, now, seed=301)
    sent.status = status.copy()
    sent.job_key = np.where(sent.job_key != NO_KEY, 7, NO_KEY).astype(np.uint32)
    st2, _ = twice(dev, cases.case("sent_300", w2, [sent]))
    assert st2.rekey["want"][23] == 0x10 and st2.rekey["want"][17] == 4 and st2.rekey["want"][4] in (0, 8)
    assert (st2.rekey["want"] & 0x10).sum() >= 1 and not (st2.rekey["want"][30:] & ~np.uint32(1)).any()


def test_send_gate_in_place(dev):
    """d_status_out may be d_status_in"""
    now = NOW
    w = send_world(now)
    ids = w.ids.tolist()
    gate = cases.gate_step([(ids[r % 40], 1 + r % 4, 0 if r % 7 else -8) for r in range(300)], now, seed=302)
    st = cases.state_of(w)
    status = cases.run_host(w, st, gate)["status_out"]
    n = gate.n
    d = {k: up(v) for k, v in inputs_of(w, cases.state_of(w), gate).items()}
    d_rekey = up(w.rekey)
    rekey.send_gate_batch(dev, d["peer"], d["count"], d["status_in"], gate.max_segs, now, d["peer_rows"], d["kp"],
                          d["send_nonce"], LIMIT, d_rekey, d["status_in"], n_jobs=n, n_ids=w.n_ids, n_peers=40,
                          n_keys=len(w.key_peer))
    torch.cuda.synchronize()
    assert d["status_in"].cpu().numpy().view(np.int32).tolist() == status.tolist()
    assert d_rekey.cpu().numpy().tobytes() == st.rekey.tobytes()


def test_received_one_peer_in_both_batches(dev):
    """2 batches x 128 group rows; the initiator of row 23, 170 s into its keypair, has a group in both"""
    now = NOW
    rng = np.random.default_rng(128)
    w = send_world(now - 40 * SECOND)
    ids = w.ids.tolist()
    groups = [(int(rng.choice(ids + [11, PEER_NONE])), int(rng.integers(-1, 200))) for _ in range(256)]
    groups[7], groups[128 + 9] = (ids[23], 4), (ids[23], 130)
    st, _ = twice(dev, cases.case("received_2x128", w, [cases.rcvd_step(groups, now, 128, seed=129)]))
    assert st.rekey["want"][23] == 0x20 and st.rekey["flags"][23] == LAST_MINUTE
    assert not (st.rekey["want"] & ~np.uint32(0x20)).any() and (st.rekey["flags"] == (st.rekey["want"] >> 5)).all()


def start_world(rows=(3, 70, 255, 256, 290, 699), n_peers=700):
    w = cases.world(n_peers, 8)
    for k, r in enumerate(rows):
        w.rekey["want"][r] = 1 << k
    w.rekey["want"][100], w.rekey["last_sent_ns"][100] = 0x40, NOW - SECOND  # within the timeout
    return w


def test_start_ranks_cross_block_edges(dev):
    """700 peer rows, three blocks; candidates at 3, 70, 255, 256, 290 and 699"""
    st, outs = twice(dev, cases.case("start_700", start_world(),
                                     [cases.start_step(4, NOW), cases.start_step(8, NOW + 1), cases.start_step(0, NOW + 2)]))
    a, b, c = outs
    assert [int(a["status"][r]) for r in (3, 70, 255, 256, 290, 699)] == [HS_STARTED] * 4 + [ERR_BATCH_FULL] * 2
    assert a["start_peer"][:4].tolist() == [3, 70, 255, 256] and a["count"][0] == 4 and a["status"][100] == -27
    assert a["start"]["flags"][:4].tolist() == [1, 0, 1, 0] and a["reasons"][[3, 290, 699, 100]].tolist() == [1, 16, 32, 0x40]
    assert [int(b["status"][r]) for r in (3, 70, 255, 256, 290, 699)] == [HS_NONE] * 4 + [HS_STARTED] * 2
    assert b["start_peer"][:8].tolist() == [290, 699] + [PEER_NONE] * 6 and b["count"][0] == 2
    assert (b["start"]["state_row"][2:8] == 0xFFFFFFFF).all() and not b["start"][2:8].tobytes().replace(b"\xff" * 4, b"", 6).strip(b"\0")
    assert not c["status"][:700].any() and c["count"][0] == 0 and not st.rekey["want"].any()


def test_start_commit_grid_a_block_wider_than_the_verdict_grid(dev):
    """300 peer rows, two verdict blocks, and 700 tickets, three commit blocks: the third fills tail descriptors only
    and has no word among the block counts, which lie in a d_work of exactly keystate.work_bytes(300)"""
    _, (o,) = twice(dev, cases.case("start_300_of_700", start_world(rows=(3, 299), n_peers=300), [cases.start_step(700, NOW)]))
    assert o["count"][0] == 2 and o["start_peer"][:2].tolist() == [3, 299]
    assert [int(o["status"][r]) for r in (3, 299, 100)] == [HS_STARTED, HS_STARTED, -27]
    assert (o["start"]["state_row"][2:700] == 0xFFFFFFFF).all() and (o["start_peer"][2:700] == PEER_NONE).all()


def test_start_without_peer_rows(dev):
    """n_peers == 0: the count is zero and every descriptor is the tail"""
    s = cases.start_step(5, NOW)
    d_start = torch.full((96 * 6,), 0xEE, dtype=torch.uint8, device="cuda")
    d_peer = torch.full((6,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
    d_count = torch.full((2,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
    rekey.start_batch(dev, NOW, None, None, up(s.tickets), d_start, d_peer, d_count, None, None, None, n_peers=0,
                      n_tickets=5, work_bytes=0)
    torch.cuda.synchronize()
    start, peer, count = np.full(6, 0xEE, np.uint8).repeat(96).view(HS_START_DTYPE), np.full(6, 0x6EEEEEEE, np.uint32), np.full(
        2, 0x6EEEEEEE, np.uint32)
    rekey.start_host(NOW, np.zeros(0, REKEY_DTYPE), np.zeros(0, cases.peers_of(1).dtype), s.tickets, start[:5], peer[:5],
                     count[:1], np.zeros(0, np.int32), np.zeros(0, np.uint32))
    assert d_start.cpu().numpy().tobytes() == start.tobytes() and (start["state_row"][:5] == 0xFFFFFFFF).all()
    assert d_peer.cpu().numpy().view(np.uint32).tolist() == peer.tolist() == [PEER_NONE] * 5 + [0x6EEEEEEE]
    assert d_count.cpu().numpy().view(np.uint32).tolist() == count.tolist() == [0, 0x6EEEEEEE]


def test_argument_errors_write_nothing(dev):
    c = NAMED["gate_sent_start"]
    w, st = c.world, cases.state_of(c.world)
    g, s, q = c.steps[0], c.steps[1], c.steps[2]
    r, v = cases.recv_step([1, 5], T0 + 400 * SECOND), cases.rcvd_step([(w.ids[0], 0)], T0 + 400 * SECOND, 1)
    e = cases.resp_step([(0, HS_RESPONDED)], NOW)
    d = {k: up(x) for k, x in dict(pkts=r.pkts, key_peer=st.key_peer, peer_rows=w.peer_rows, kp=st.kp, peer=g.peer,
                                   count=g.count, status=g.status_in, job_key=s.job_key, send_nonce=st.send_nonce,
                                   rekey=st.rekey, groups=v.groups, resp=e.resp, gate=e.gate, hs_peers=st.hs_peers,
                                   tickets=q.tickets).items()}
    before = {k: x.cpu().numpy().tobytes() for k, x in d.items()}
    d_out = torch.full((8,), 12345, dtype=torch.int32, device="cuda")
    d_start = torch.full((96 * 2,), 0xEE, dtype=torch.uint8, device="cuda")
    d_sp, d_count, d_reasons = (torch.full((4,), 12345, dtype=torch.int32, device="cuda") for _ in range(3))
    d_work = torch.zeros(keystate.work_bytes(4) + 16, dtype=torch.uint8, device="cuda")
    rows = dict(peer_rows=d["peer_rows"], kp=d["kp"], n_ids=w.n_ids, n_peers=4)

    def recv(**kw):
        a = dict(pkts=d["pkts"], now_ns=NOW, key_peer=d["key_peer"], n=2, n_keys=16, **rows)
        a.update(kw)
        rekey.recv_gate_batch(dev, **a)

    def gate(**kw):
        a = dict(peer=d["peer"], count=d["count"], status_in=d["status"], max_segs=4, now_ns=NOW, send_nonce=d["send_nonce"],
                 limit=LIMIT, rekey=d["rekey"], status_out=d_out, n_jobs=3, n_keys=16, **rows)
        a.update(kw)
        rekey.send_gate_batch(dev, **a)

    def sent(**kw):
        a = dict(peer=d["peer"], count=d["count"], status=d["status"], job_key=d["job_key"], max_segs=4, now_ns=NOW,
                 send_nonce=d["send_nonce"], limit=LIMIT, rekey=d["rekey"], n_jobs=3, n_keys=16, **rows)
        a.update(kw)
        rekey.sent_batch(dev, **a)

    def rcvd(**kw):
        a = dict(groups=d["groups"], calls_per_batch=1, now_ns=NOW, rekey=d["rekey"], n_batches=1, **rows)
        a.update(kw)
        rekey.received_batch(dev, **a)

    def resp(**kw):
        a = dict(resp=d["resp"], gate=d["gate"], now_ns=NOW, rekey=d["rekey"], n=1, n_peers=4)
        a.update(kw)
        rekey.responded_batch(dev, **a)

    def start(**kw):
        a = dict(now_ns=NOW, rekey=d["rekey"], hs_peers=d["hs_peers"], tickets=d["tickets"], start=d_start, start_peer=d_sp,
                 count=d_count, status=d_out, reasons=d_reasons, work=d_work, n_peers=4, n_tickets=2,
                 work_bytes=keystate.work_bytes(4))
        a.update(kw)
        rekey.start_batch(dev, **a)

    odd = lambda x, by=2: x.data_ptr() + by  # noqa: E731
    rows_bad = [dict(peer_rows=None), dict(kp=None), dict(peer_rows=odd(d["peer_rows"])), dict(kp=odd(d["kp"]))]
    jobs_bad = rows_bad + [dict(peer=None), dict(count=None), dict(send_nonce=None), dict(rekey=None), dict(max_segs=0),
                           dict(n_jobs=1 << 27), dict(peer=odd(d["peer"])), dict(count=odd(d["count"])),
                           dict(send_nonce=odd(d["send_nonce"], 4)), dict(rekey=odd(d["rekey"], 4))]
    calls = [(recv, rows_bad + [dict(pkts=None), dict(key_peer=None), dict(n=(1 << 28) + 1), dict(pkts=odd(d["pkts"], 4)),
                                dict(key_peer=odd(d["key_peer"]))]),
             (gate, jobs_bad + [dict(status_in=None), dict(status_out=None), dict(status_in=odd(d["status"])),
                                dict(status_out=odd(d_out))]),
             (sent, jobs_bad + [dict(status=None), dict(job_key=None), dict(status=odd(d["status"])),
                                dict(job_key=odd(d["job_key"]))]),
             (rcvd, rows_bad + [dict(groups=None), dict(rekey=None), dict(n_batches=1 << 20, calls_per_batch=1 << 9),
                                dict(groups=odd(d["groups"], 4)), dict(rekey=odd(d["rekey"], 4))]),
             (resp, [dict(resp=None), dict(gate=None), dict(rekey=None), dict(n=(1 << 28) + 1), dict(resp=odd(d["resp"])),
                     dict(gate=odd(d["gate"])), dict(rekey=odd(d["rekey"], 4))]),
             (start, [dict(rekey=None), dict(hs_peers=None), dict(tickets=None), dict(start=None), dict(start_peer=None),
                      dict(count=None), dict(status=None), dict(reasons=None), dict(work=None), dict(work_bytes=64),
                      dict(n_peers=(1 << 24) + 1), dict(n_tickets=(1 << 28) + 1), dict(start=d["tickets"]),
                      dict(work=odd(d_work, 8)), dict(rekey=odd(d["rekey"], 4)), dict(hs_peers=odd(d["hs_peers"])),
                      dict(tickets=odd(d["tickets"])), dict(start=odd(d_start)), dict(start_peer=odd(d_sp)),
                      dict(count=odd(d_count)), dict(status=odd(d_out)), dict(reasons=odd(d_reasons))])]
    for fn, bad in calls:
        for kw in bad:
            with pytest.raises(_lib.WgcsError) as ei:
                fn(**kw)
            assert ei.value.code == _lib.ERR_INVALID_ARG, (fn.__name__, kw)
    L, p = dev.lib, lambda x: x.data_ptr()  # noqa: E731
    assert L.wgcs_rekey_recv_gate_batch(None, p(d["pkts"]), 2, NOW, p(d["key_peer"]), 16, p(d["peer_rows"]), w.n_ids,
                                        p(d["kp"]), 4, None) == _lib.ERR_INVALID_ARG
    assert L.wgcs_rekey_start_batch(None, NOW, p(d["rekey"]), p(d["hs_peers"]), 4, p(d["tickets"]), 2, p(d_start), p(d_sp),
                                    p(d_count), p(d_out), p(d_reasons), p(d_work), keystate.work_bytes(4), None) == _lib.ERR_INVALID_ARG
    # n == 0 is a no-op, whatever else is given
    recv(n=0, pkts=None)
    gate(n_jobs=0, peer=None, count=None, status_in=None, status_out=None)
    sent(n_jobs=0, peer=None, count=None, status=None, job_key=None)
    rcvd(n_batches=0, groups=None)
    rcvd(calls_per_batch=0, groups=None)
    resp(n=0, resp=None, gate=None)
    torch.cuda.synchronize()
    for t in (d_out, d_sp, d_count, d_reasons):
        assert (t.cpu().numpy() == 12345).all()
    assert (d_start.cpu().numpy() == 0xEE).all()
    assert {k: x.cpu().numpy().tobytes() for k, x in d.items()} == before
    # and the same arguments without the fault do the work
    recv(now_ns=T0 + 400 * SECOND)
    gate(now_ns=T0 + 180 * SECOND)
    start()
    torch.cuda.synchronize()
    assert d["pkts"].cpu().numpy().view(AEAD_PKT_DTYPE)["key"].tolist() == [SESSION_EXPIRED] * 2
    assert d_out.cpu().numpy()[:4].tolist() == [HS_STARTED, HS_STARTED, ERR_BATCH_FULL, HS_NONE]
    assert d_count.cpu().numpy()[0] == 2 and d_sp.cpu().numpy()[:2].tolist() == [0, 1]
    assert SET == 1 and INITIATOR == 2
