"""Keypair rotation on the GPU (wgcs_keypairs_begin_responder_batch,
wgcs_keypairs_begin_initiator_batch, wgcs_keypairs_received_batch; the kernels
of keypairs_kernels.hip) against the host forms of keypairs.cpp, byte for byte
over whole tables: the wgcs_keypairs rows, both slot arrays, the AEAD key
table, its key -> peer id column, and the call's own output.
tests/test_keypairs_ref.py pins the host forms to the restatement of
device/noise.go:664-754.

The status / rotated buffers are filled with a sentinel first and are longer
than the call's rows; every read-only input is compared with its upload
afterwards; every claim is 0xFFFFFFFF after a call."""
import numpy as np
import pytest
import torch

import keypairs_cases as cases
from keypairs_cases import NOW, OK, TABLES
from keypairs_ref import (CLAIM_NONE, ERR_INVALID_ARG, ERR_NO_HANDSHAKE, ERR_PACKET_TOO_SHORT, HS_BEGUN, HS_NONE,
                          HS_RESPONDED, NO_KEYPAIR)
from test_gpu_cookie import up
from wireguard_amd import _lib, keypairs, keystate
from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.router import SESSION_SLOT_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE

pytestmark = pytest.mark.gpu

SPARE = 3  # rows of d_status / d_rotated past the call's: they keep their fill
FILL = 0x5A5A5A5A
VIEWS = dict(kp=KEYPAIRS_DTYPE, slots=SESSION_SLOT_DTYPE, peer_keys=SESSION_SLOT_DTYPE, keys=AEAD_KEY_DTYPE,
             key_peer=np.uint32)


def host_step(w, t, s):
    """(output with its spare rows, the tables after the step); t is left alone"""
    t = {k: v.copy() for k, v in t.items()}
    out = np.full(s.n + SPARE, FILL, np.uint32)
    out[:s.n] = cases.run_host(w, t, s).view(np.uint32)
    return out, t


def device_step(dev, w, t, s, stream=None):
    d = {k: up(v) for k, v in t.items()}
    d_out = torch.from_numpy(np.full(s.n + SPARE, FILL, np.uint32).view(np.int32)).cuda()
    if s.kind == "recv":
        ins = dict(pkts=s.pkts, verdict=s.verdict, peer_rows=w.peer_rows)
    elif s.kind == "resp":
        ins = dict(resp=s.resp, gate=s.gate, table=w.table)
    else:
        ins = dict(arena=s.arena, pkts=s.pkts, gate=s.gate, hs_slots=w.hs_slots, states=w.states, table=w.table)
    di = {k: up(v) for k, v in ins.items()}
    d_work = torch.full((keystate.work_bytes(max(s.n, 1)),), 0x77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sizes = dict(n_peers=len(w.table), n_slots=len(t["slots"]), n_peer_slots=len(t["peer_keys"]), n_keys=len(t["keys"]))
    if s.kind == "recv":
        keypairs.received_batch(dev, di["pkts"], di["verdict"], d["key_peer"], di["peer_rows"], d["kp"], d["slots"],
                                d["peer_keys"], d["keys"], d_out, stream=stream, n=s.n, n_ids=w.n_ids, **sizes)
    elif s.kind == "resp":
        keypairs.begin_responder_batch(dev, di["resp"], di["gate"], s.now, di["table"], d["kp"], d["slots"],
                                       d["peer_keys"], d["keys"], d["key_peer"], d_out, d_work, stream=stream, n=s.n,
                                       **sizes)
    else:
        keypairs.begin_initiator_batch(dev, di["arena"], di["pkts"], di["gate"], s.now, di["hs_slots"], di["states"],
                                       di["table"], d["kp"], d["slots"], d["peer_keys"], d["keys"], d["key_peer"], d_out,
                                       d_work, stream=stream, n=s.n, n_hs_slots=len(w.hs_slots), n_states=len(w.states),
                                       **sizes)
    torch.cuda.synchronize()
    for k, a in ins.items():
        assert di[k].cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), f"{k} was written"
    return d_out.cpu().numpy().view(np.uint32), {k: v.cpu().numpy().view(VIEWS[k]) for k, v in d.items()}


def check_case(dev, c):
    w, t, outs = c.world, cases.tables_of(c.world), []
    for k, s in enumerate(c.steps):
        want_out, want_t = host_step(w, t, s)
        got_out, got_t = device_step(dev, w, t, s)
        where = f"{c.name} step {k} ({s.kind})"
        bad = np.flatnonzero(got_out != want_out)
        assert len(bad) == 0, f"{where}: row {bad[0]}: got {got_out.view(np.int32)[bad[0]]}, want {want_out.view(np.int32)[bad[0]]}"
        for name in TABLES:
            assert got_t[name].tobytes() == want_t[name].tobytes(), f"{where}: {name}"
        assert (got_t["kp"]["claim"] == CLAIM_NONE).all(), where
        t = got_t
        outs.append(got_out[:s.n].view(np.int32 if s.kind != "recv" else np.uint32))
    return t, outs


NAMED = {c.name: c for c in cases.named()}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case_matches_the_host_form(dev, name):
    check_case(dev, NAMED[name])


def wide_begin(n=300, n_peers=40):
    """n responder descriptors and then n initiator rows over n_peers peers, several per peer, so a peer's run
    of the key order gathers rows of different waves and blocks of the collecting kernel; one peer's sit at
    3, 70 and 290.  Every 23rd descriptor is gated off, every 31st names a key row past the table, every 37th
    an index nobody registered."""
    rng = np.random.default_rng(300)
    idx = [int(x) for x in rng.choice(1 << 24, 2 * n, replace=False) + 1]
    special, others = 17, [r for r in range(n_peers) if r != 17]
    n_keys = 4 * n + 2

    def peer_of(j):
        return special if j in (3, 70, 290) else others[int(rng.integers(0, len(others)))]

    hs = [(idx[n + q], peer_of(q), 2 * (n + q), 2 * (n + q) + 1 if q % 31 else n_keys) for q in range(n)]
    w = cases.world(n_peers, n_keys, [x for k, x in enumerate(idx) if k % 37 != 36], handshakes=hs, seed=301)
    descs = [(peer_of(j), idx[j], 2 * j if j % 31 else n_keys + 7, 2 * j + 1, HS_RESPONDED if j % 23 else int(rng.integers(-24, 4)))
             for j in range(n)]
    rows = [(idx[n + q], cases.HS_FINISHED if q % 23 else int(rng.integers(-24, 6))) for q in range(n)]
    return cases.case("wide_begin", w, [cases.resp_step(descs, seed=302), cases.init_step(rows, now=NOW + 7, seed=303)])


def test_begin_runs_of_one_peer_across_waves_and_blocks(dev):
    c = wide_begin()
    t, (resp_status, init_status) = check_case(dev, c)
    for st in (resp_status, init_status):
        assert {HS_NONE, HS_BEGUN, ERR_INVALID_ARG, ERR_NO_HANDSHAKE} <= set(st.tolist())
        assert [st[q] for q in (3, 70, 290)] == [HS_BEGUN] * 3
    # the special peer: its responder descriptors left 290's in next, and then three initiator begins in row order
    k = t["kp"][17]
    assert (int(k["current"]["send_key"]), int(k["previous"]["send_key"])) == (2 * (300 + 290), 2 * (300 + 70))
    assert k["next"]["flags"] == 0 and not t["keys"][[2 * 3, 2 * 70, 2 * 290, 2 * 303]].view(np.uint8).any()
    # the same calls again on fresh tables: the same bytes, whichever lane ran first
    t2, _ = check_case(dev, c)
    assert all(t[k].tobytes() == t2[k].tobytes() for k in TABLES)


@pytest.mark.parametrize("place", ["highest_row_ends_at_n", "lowest_row_ends_at_a_key_change"])
@pytest.mark.parametrize("k", [1, 2, 65])
def test_begin_responder_run_lengths_and_ends(dev, k, place):
    """k descriptors for one peer, which its lane takes in descriptor order: the peer's run of the key order ends
    at n (the highest row, every descriptor taking part) or at the short run of another peer behind it."""
    n, n_peers = k + 3, 5
    rng = np.random.default_rng(650 + k)
    idx = [int(x) for x in rng.choice(1 << 24, n, replace=False) + 1]
    if place == "highest_row_ends_at_n":
        row, peers = 4, [1] + [4] * k + [2, 1]
    else:
        row, peers = 0, [2] + [0] * k + [2, 2]
    w = cases.world(n_peers, 2 * n + 2, idx, seed=651)
    descs = [(p, idx[j], 2 * j, 2 * j + 1) for j, p in enumerate(peers)]
    t, (status,) = check_case(dev, cases.case("run_of_%d" % k, w, [cases.resp_step(descs, seed=652)]))
    assert status.tolist() == [HS_BEGUN] * n
    assert int(t["kp"]["next"]["send_key"][row]) == 2 * k  # the run's last descriptor is the one that stays


def wide_received(n=2 * 256 + 44, n_peers=12):
    """n rows; peer row 5's candidates at 3, 70 and 290, peer row 9's only in the last block (530 and 550), a
    third peer's candidate carries WGCS_ERR_REPLAY; the other rows run under current keys, keys of nobody and
    keys past the table."""
    rng = np.random.default_rng(556)
    idx = [0x2000 + 3 * i for i in range(2 * n_peers + 1)]
    spare = 4 * n_peers  # two key rows and an index for a previous keypair that no call leaves beside a next one
    w = cases.world(n_peers, 4 * n_peers + 6, idx, seed=557)
    t = cases.tables_of(w)
    # every peer: a current keypair (keys 4r, 4r + 1) by begin + received, then the odd ones a next one (4r + 2, 4r + 3)
    cases.run_host(w, t, cases.resp_step([(r, idx[2 * r], 4 * r, 4 * r + 1) for r in range(n_peers)]))
    cases.run_host(w, t, cases.recv_step([(4 * r + 1, OK) for r in range(n_peers)]))
    cases.run_host(w, t, cases.resp_step([(r, idx[2 * r + 1], 4 * r + 2, 4 * r + 3) for r in range(n_peers) if r % 2],
                                         now=NOW + 1))
    assert (t["kp"]["next"]["flags"][1::2] == 1).all() and (t["kp"]["current"]["flags"] == 1).all()
    # A responder's begin clears previous, so DeleteSession(previous) of :750 finds nil in every state the calls
    # reach.  The host may write the table too: peer row 5 gets a previous keypair by hand.
    t["kp"]["previous"][5] = (spare, spare + 1, idx[-1], 1, 5)
    t["key_peer"][spare:spare + 2] = w.table["peer"][5]
    t["slots"]["key"][t["slots"]["index"] == idx[-1]] = spare + 1
    for k, v in t.items():
        setattr(w, k, v)
    rows = []
    for i in range(n):
        r = int(rng.integers(0, n_peers))
        u = rng.random()
        if r in (5, 9, 7) or u < 0.7:
            key = 4 * (r if r not in (5, 9, 7) else 0) + 1               # under a current keypair
        elif u < 0.8:
            key = spare + int(rng.integers(0, 8))                        # row 5's previous, stray rows, past the table
        else:
            key = 4 * r + 3 if r % 2 and r not in (5, 9, 7) else 4 * r + 1  # other peers' next, anywhere
        rows.append((key, int(rng.choice([OK, OK, 0, ERR_PACKET_TOO_SHORT, -18, -20]))))
    for i, r in ((3, 5), (70, 5), (290, 5), (530, 9), (550, 9)):
        rows[i] = (4 * r + 3, OK)
    rows[1] = (4 * 5 + 3, -20)   # in front of row 3, but the filter refused it
    rows[100] = (4 * 7 + 3, -20)
    rows[200] = (4 * 7 + 3, -18)
    return cases.case("wide_received", w, [cases.recv_step(rows, seed=558)])


def test_received_lowest_row_wins_across_blocks(dev):
    c = wide_received()
    t, (rotated,) = check_case(dev, c)
    assert [int(rotated[i]) for i in (1, 3, 70, 290, 530, 550, 100, 200)] == [0, 1, 0, 0, 1, 0, 0, 0]
    assert t["kp"]["next"]["flags"][[5, 9, 7]].tolist() == [0, 0, 1] and rotated.sum() >= 3
    assert not t["keys"][[48, 49]].view(np.uint8).any() and t["key_peer"][48] == 0xFFFFFFFF  # row 5's old previous is gone
    assert tuple(t["kp"]["previous"][5])[:2] == (20, 21) and tuple(t["kp"]["current"][5])[:2] == (22, 23)
    # run twice on fresh tables: the same bytes both times
    t2, (rotated2,) = check_case(dev, c)
    assert rotated.tobytes() == rotated2.tobytes() and all(t[k].tobytes() == t2[k].tobytes() for k in TABLES)


def test_argument_errors_write_nothing(dev):
    c = NAMED["initiator_with_a_staged_next"]
    w, t = c.world, cases.tables_of(c.world)
    s, q, r = cases.resp_step([(0, cases.I[0], 0, 1)]), cases.init_step([cases.I[6]]), cases.recv_step([(1, OK)])
    d = {k: up(v) for k, v in t.items()}
    di = {k: up(v) for k, v in dict(resp=s.resp, gate=s.gate, table=w.table, arena=q.arena, ipkts=q.pkts, igate=q.gate,
                                    hs_slots=w.hs_slots, states=w.states, rpkts=r.pkts, verdict=r.verdict,
                                    peer_rows=w.peer_rows).items()}
    d_out = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
    d_work = torch.zeros(keystate.work_bytes(1), dtype=torch.uint8, device="cuda")
    sizes = dict(n_peers=4, n_slots=len(t["slots"]), n_peer_slots=len(t["peer_keys"]), n_keys=16)

    def resp(**kw):
        a = dict(resp=di["resp"], gate=di["gate"], now_ns=NOW, table=di["table"], kp=d["kp"], slots=d["slots"],
                 peer_keys=d["peer_keys"], keys=d["keys"], key_peer=d["key_peer"], status=d_out, work=d_work, n=1, **sizes)
        a.update(kw)
        keypairs.begin_responder_batch(dev, **a)

    def init(**kw):
        a = dict(arena=di["arena"], pkts=di["ipkts"], gate=di["igate"], now_ns=NOW, hs_slots=di["hs_slots"],
                 states=di["states"], table=di["table"], kp=d["kp"], slots=d["slots"], peer_keys=d["peer_keys"],
                 keys=d["keys"], key_peer=d["key_peer"], status=d_out, work=d_work, n=1, n_hs_slots=len(w.hs_slots),
                 n_states=len(w.states), **sizes)
        a.update(kw)
        keypairs.begin_initiator_batch(dev, **a)

    def recv(**kw):
        a = dict(pkts=di["rpkts"], verdict=di["verdict"], key_peer=d["key_peer"], peer_rows=di["peer_rows"], kp=d["kp"],
                 slots=d["slots"], peer_keys=d["peer_keys"], keys=d["keys"], rotated=d_out, n=1, n_ids=w.n_ids, **sizes)
        a.update(kw)
        keypairs.received_batch(dev, **a)

    odd = lambda x, by=2: x.data_ptr() + by  # noqa: E731
    tail_bad = [dict(gate=None), dict(status=None), dict(table=None), dict(kp=None), dict(slots=None), dict(peer_keys=None),
                dict(keys=None), dict(key_peer=None), dict(work=None), dict(status=di["gate"]), dict(n=(1 << 24) + 1),
                dict(n_peers=(1 << 24) + 1), dict(n_slots=24), dict(n_peer_slots=6), dict(work_bytes=64),
                dict(work=odd(d_work, 8), work_bytes=keystate.work_bytes(1) - 8), dict(gate=odd(di["gate"])),
                dict(status=odd(d_out)), dict(table=odd(di["table"])), dict(kp=odd(d["kp"])), dict(slots=odd(d["slots"])),
                dict(peer_keys=odd(d["peer_keys"])), dict(keys=odd(d["keys"])), dict(key_peer=odd(d["key_peer"]))]
    calls = [(resp, tail_bad + [dict(resp=None), dict(resp=odd(di["resp"]))]),
             (init, [kw for kw in tail_bad if kw.get("status") is not di["gate"]] +
              [dict(status=di["igate"]), dict(arena=None), dict(pkts=None), dict(hs_slots=None), dict(states=None),
               dict(n_hs_slots=12), dict(pkts=odd(di["ipkts"], 4)), dict(hs_slots=odd(di["hs_slots"])),
               dict(states=odd(di["states"]))]),
             (recv, [dict(pkts=None), dict(verdict=None), dict(rotated=None), dict(key_peer=None), dict(keys=None),
                     dict(peer_rows=None), dict(kp=None), dict(slots=None), dict(peer_keys=None), dict(n=(1 << 28) + 1),
                     dict(n_slots=24), dict(n_peer_slots=6), dict(pkts=odd(di["rpkts"], 4)), dict(verdict=odd(di["verdict"])),
                     dict(rotated=odd(d_out)), dict(key_peer=odd(d["key_peer"])), dict(keys=odd(d["keys"])),
                     dict(peer_rows=odd(di["peer_rows"])), dict(kp=odd(d["kp"])), dict(slots=odd(d["slots"])),
                     dict(peer_keys=odd(d["peer_keys"]))])]
    for fn, bad in calls:
        for kw in bad:
            with pytest.raises(_lib.WgcsError) as ei:
                fn(**kw)
            assert ei.value.code == ERR_INVALID_ARG, (fn.__name__, kw)
    L, p = dev.lib, lambda x: x.data_ptr()  # noqa: E731
    assert L.wgcs_keypairs_received_batch(None, p(di["rpkts"]), p(di["verdict"]), 1, p(d["key_peer"]), 16, p(di["peer_rows"]),
                                          w.n_ids, p(d["kp"]), 4, p(d["slots"]), sizes["n_slots"], p(d["peer_keys"]),
                                          sizes["n_peer_slots"], p(d["keys"]), p(d_out), None) == ERR_INVALID_ARG
    # n == 0 is a no-op, whatever else is given
    resp(n=0, resp=None, gate=None, status=None, work=None, work_bytes=0)
    init(n=0, arena=None, pkts=None, gate=None, status=None, work=None, work_bytes=0)
    recv(n=0, pkts=None, verdict=None, rotated=None)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 12345).all()
    for k in TABLES:
        assert d[k].cpu().numpy().tobytes() == t[k].tobytes(), k
    # and the same arguments without the fault do the work
    resp()
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tolist() == [HS_BEGUN, 12345, 12345, 12345]
    slots = d["slots"].cpu().numpy().view(SESSION_SLOT_DTYPE)
    assert {int(x["index"]): int(x["key"]) for x in slots if x["key"] != 0xFFFFFFFF}[cases.I[0]] == 1
    assert NO_KEYPAIR in slots["key"]
