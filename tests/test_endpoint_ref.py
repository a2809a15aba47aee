"""The host forms of the peer endpoints (wgcs_endpoint_recv_host, the three
_set_*_host and the three _dst_*_host; wireguard_amd/csrc/endpoint.cpp over
wgcs_endpoint.h) against tests/endpoint_ref.py, the literal restatement of
getSrcFromControl, of the tail of ReceiveIPvX and of a Peer whose endpoint is
set, marked and sent to message by message (CPU only).

The set forms decide the rows of one peer by a claim and a commit and the dst
forms read before they clear; the restatement knows neither.  Every comparison
here is therefore also the proof that those passes leave what taking the rows in
turn leaves.  Every table and every output is compared whole."""
import struct

import numpy as np
import pytest

import endpoint_ref as ref
from endpoint_cases import (ADDRS, CLEAR_SRC, GRO, OOB_STRIDE, PKTINFO4, PKTINFO6, World, addr_row, control_cases, ep_row,
                            ep_rows, finished_rows, oob_of, random_endpoints, recv_ref)
from wireguard_amd import _lib, endpoint as ep, keypairs, noise, rekey, router, timers as tm
from wireguard_amd._lib import (ERR_INVALID_ARG, ERR_NO_ENDPOINT, HS_FINISHED, HS_INITIATED, HS_NONE, HS_RESPONDED,
                                PEER_NONE)
from wireguard_amd.cookie import SRC_ADDR_DTYPE

SECOND = 1_000_000_000
NOW = 1000 * SECOND


def same(a, b):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def recv(addrs, src_from, sizes, controls, n_msgs):
    """One recv call on the host form and on the restatement, outputs compared whole over a sentinel."""
    n = len(sizes)
    oob, nn = oob_of(controls)
    a = np.concatenate([addr_row(x) for x in addrs])
    got = np.full(n, 0xEE, np.uint8).repeat(64).view(ep.ENDPOINT_DTYPE)
    out = np.full(n, 0xEE, np.uint8).repeat(20).view(SRC_ADDR_DTYPE)
    ep.recv_host(a, src_from, sizes, oob, OOB_STRIDE, nn, n_msgs, n // n_msgs, ep=got, addr_out=out)
    want = recv_ref(addrs, src_from, sizes, controls, n_msgs)
    same(got, ep_rows(want))
    same(out, ep_rows(want)["dst"].copy())
    return want


# ---------------------------------------------------------------- layout
def test_constants_symbols_and_layout():
    assert ERR_NO_ENDPOINT == ref.ERR_NO_ENDPOINT == -30 and CLEAR_SRC == 4
    f = ep.ENDPOINT_DTYPE.fields
    assert [f[k][1] for k in ("dst", "src_len", "pad", "src")] == [0, 20, 21, 24] and ep.ENDPOINT_DTYPE.itemsize == 64
    L = _lib.load()
    for name in ("recv", "set_received", "set_accepted", "set_finished", "dst_jobs", "dst_initiated", "dst_responded"):
        for form in ("batch", "host"):
            assert f"wgcs_endpoint_{name}_{form}" in _lib.declared_symbols() and hasattr(L, f"wgcs_endpoint_{name}_{form}")
    assert "wgcs_coalesce_messages_dst_batch" in _lib.declared_symbols() and hasattr(L, "wgcs_coalesce_messages_dst_batch")
    r = ep.row("2001:db8::9", 7, PKTINFO6)[0]
    assert r["dst"]["len"] == 18 and r["src_len"] == 40 and bytes(r["src"][:36]) == PKTINFO6[:36]


# ---------------------------------------------------------------- getSrcFromControl
def test_get_src_from_control_named_cases():
    cases = control_cases()
    names = list(cases)
    want = recv([ADDRS[i % 4] for i in range(len(names))], None, [148] * len(names), [cases[k] for k in names], len(names))
    src = {k: want[i][1] for i, k in enumerate(names)}
    assert src["no control"] == b"" and src["exactly 16 bytes"] == b"" and src["len beyond the buffer"] == b""
    assert src["bad len then pktinfo"] == b""
    assert src["pktinfo4"] == src["pktinfo4 before gro"] == src["pktinfo4 after gro"] == PKTINFO4[:28] + bytes(4)
    assert src["pktinfo6"] == src["unknown in front"] == src["two pktinfo"] == PKTINFO6[:36] + bytes(4)
    data = bytes(range(0x11, 0x41))
    for length, kept in ((16, 0), (20, 4), (28, 12), (29, 13), (64, 16)):
        hdr = struct.pack("<Qii", length, 0, 8)  # the header as received, Len included
        assert src[f"len {length}"] == hdr + data[:kept] + bytes(16 - kept)
    assert src["pktinfo6 len 64"] == struct.pack("<Qii", 64, 41, 50) + bytes(range(0x40, 0x58))


def test_get_gso_size_walks_the_same_messages():
    import ctypes as C
    L = _lib.load()
    for name, control in control_cases().items():
        g = C.c_int(-7)
        rc = L.wgcs_get_gso_size(control, len(control), C.byref(g))
        # the restatement's walk: the first UDP_GRO message with two bytes of data, an error for a bad Len
        want, err, rest = 0, 0, control
        while len(rest) > 16:
            parsed = ref.parse_one_socket_control_message(rest)
            if parsed is None:
                err = -16
                break
            _, (_, level, typ), data, rest = parsed
            if level == ref.SOL_UDP and typ == ref.UDP_GRO and len(data) >= 2:
                want = struct.unpack("<H", data[:2])[0]
                break
        assert (rc, g.value) == (err, want), name
    assert GRO in control_cases()["pktinfo4 after gro"]


# ---------------------------------------------------------------- bind.go:308-319
def test_a_split_packet_takes_its_neighbours_addr_and_its_own_control():
    # 2 batches x 4 slots; messages land at slots 2 and 3, the split spreads message 2 over slots 0..2
    addrs = [ADDRS[0], ADDRS[0], ADDRS[1], ADDRS[2]] * 2
    src_from = [2, 2, -1, -1, 3, -1, 2, 0]
    sizes = [100, 100, 40, 0, 60, 0, 9, 9]
    controls = [b"", PKTINFO4, PKTINFO6 + GRO, PKTINFO4, b"", PKTINFO6, GRO, PKTINFO4]
    want = recv(addrs, src_from, sizes, controls, 4)
    assert want[0] == (ADDRS[1], b"") and want[1] == (ADDRS[1], PKTINFO4[:28] + bytes(4))  # slot 1's own control buffer
    assert want[2] == (ADDRS[1], PKTINFO6[:36] + bytes(4)) and want[3] is None and want[5] is None
    assert want[4] == (ADDRS[2], b"") and want[6][0] == ADDRS[1] and want[7][0] == ADDRS[0]


def test_from_out_of_range_and_nn_out_of_range():
    addrs, controls = [ADDRS[0]] * 4, [PKTINFO4] * 4
    want = recv(addrs, [4, -2, 3, 2**31 - 1], [9, 9, 9, 9], controls, 4)
    assert [w is None for w in want] == [True, True, False, True]
    oob, nn = oob_of(controls)
    nn[:] = [-1, OOB_STRIDE + 1, OOB_STRIDE, 32]
    got, _ = ep.recv_host(np.concatenate([addr_row(a) for a in addrs]), None, [9] * 4, oob, OOB_STRIDE, nn, 4, 1)
    assert got["src_len"].tolist() == [0, 0, 32, 32]  # a length outside [0, oob_stride] reads as no control


# ---------------------------------------------------------------- SetEndpointFromPacket
def set_received(w: World, rows, endpoints, calls_per_batch=None):
    g = w.groups(rows)
    ep.set_received_host(g, calls_per_batch or max(len(rows), 1), ep_rows(endpoints), w.peer_rows, w.table, w.claim, w.timers)
    w.ref_set([(w.row_of_id(peer) if tail >= 0 else None, tail) for peer, tail in rows], endpoints)
    w.check()


def set_accepted(w: World, desc, endpoints):
    d = np.zeros(len(desc), noise.HS_RESP_DTYPE)
    d["init_row"], d["peer_row"] = [i for i, _ in desc], [r for _, r in desc]
    ep.set_accepted_host(d, ep_rows(endpoints), w.table, w.claim, w.timers)
    w.ref_set([(r if r < w.n_peers else None, i) for i, r in desc], endpoints)
    w.check()
    return d


def set_finished(w: World, peer_rows, gates, endpoints):
    arena, pkts, gate, hs_slots, states = finished_rows(w.rng, w, peer_rows, gates)
    ep.set_finished_host(arena, pkts, gate, hs_slots, states, ep_rows(endpoints), w.table, w.claim, w.timers)
    w.ref_set([(r if r is not None and r < w.n_peers and g == HS_FINISHED else None, q)
               for q, (r, g) in enumerate(zip(peer_rows, gates))], endpoints)
    w.check()


A, B, C6 = (ADDRS[0], PKTINFO4[:28] + bytes(4)), (ADDRS[2], b""), (ADDRS[1], PKTINFO6[:36] + bytes(4))


def test_two_groups_of_one_peer_in_one_call_and_in_two_batches():
    w = World(np.random.default_rng(1))
    p0, p1 = w.ids[0], w.ids[1]
    eps = [A, B, C6, None, A]
    set_received(w, [(p0, 0), (p1, 2), (p0, 1)], eps)  # one batch: the higher group row wins
    assert w.ref[0].val == B and w.ref[1].val == C6
    set_received(w, [(p0, 1), (PEER_NONE, -1), (p1, 0), (p0, 2)], eps, calls_per_batch=2)  # the later batch wins
    assert w.ref[0].val == C6 and w.ref[1].val == A


def test_a_tail_row_with_a_zero_endpoint_tails_out_of_range_and_unknown_peers():
    w = World(np.random.default_rng(2))
    p0 = w.ids[0]
    set_received(w, [(p0, 0)], [A])
    set_received(w, [(p0, 1), (p0, 3), (p0, 2), (0, 0), (w.n_ids - 1, 0), (w.n_ids + 5, 0), (PEER_NONE, -1)], [B, None, A])
    assert w.ref[0].val == A  # row 1 is a slot of size 0, tail 3 is past the rows: both are passed by
    bad = ep_row(A)
    bad["dst"]["len"] = 7
    ep.set_received_host(w.groups([(p0, 0)]), 1, bad, w.peer_rows, w.table, w.claim, w.timers)
    w.check()  # a source row whose dst.len is neither 6 nor 18 is no candidate


def test_accepted_with_respond_refusing_and_tail_descriptors():
    w = World(np.random.default_rng(3))
    # descriptor 1's response will be refused (say a low-order point): :314 ran before it was built
    set_accepted(w, [(0, 2), (1, 3), (2, 2), (0xFFFFFFFF, 0), (1, w.n_peers), (5, 1)], [A, B, C6])
    assert w.ref[2].val == C6 and w.ref[3].val == B and w.ref[0].val is None and w.ref[1].val is None


def test_finished_with_begin_refusing_and_a_duplicate_response():
    w = World(np.random.default_rng(4))
    # rows 0 and 3 are two authentic responses for peer 1's handshakes: the later one stands, whatever begin said
    set_finished(w, [1, 2, None, 1, 9], [HS_FINISHED, HS_NONE, HS_FINISHED, HS_FINISHED, HS_FINISHED], [A, B, C6, B, A])
    assert w.ref[1].val == B and w.ref[2].val is None and [p.val for p in w.ref].count(None) == 4


# ---------------------------------------------------------------- Peer.Send
def dst_jobs(w: World, jobs, max_segs=3):
    """jobs: (peer id, count, status, kept, lens).  One dst_jobs call on the host form and the restatement."""
    n = len(jobs)
    peer, lens = np.full(n * max_segs, PEER_NONE, np.uint32), np.full(n * max_segs, -9, np.int32)
    count, status, key, nbufs = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.int32))
    for j, (pid, c, st, kept, ln) in enumerate(jobs):
        peer[j * max_segs] = pid
        count[j], status[j], key[j] = c, st, (7 if kept else 0xFFFFFFFF)
        nbufs[j] = c if kept and st == 0 and 1 <= c <= max_segs else 0
        lens[j * max_segs:j * max_segs + len(ln)] = ln
    want_nbufs = nbufs.copy()
    rows, want = [], []
    for j, (pid, c, st, kept, ln) in enumerate(jobs):
        r = w.row_of_id(pid) if kept and st == 0 and 1 <= c <= max_segs else None
        rows.append(r)
        d, v6, s = w.ref_send(r)
        tx = 0
        if s == ERR_NO_ENDPOINT:
            want_nbufs[j] = 0
        elif r is not None:
            tx = sum(ln[:c])  # peer.go:213-218, for the host to add once its send succeeded
        want.append((d, v6, s, tx))
    dst, v6, ds, tx = ep.dst_jobs_host(peer, count, status, key, max_segs, lens, nbufs, w.peer_rows, w.table, w.timers)
    same(dst, np.concatenate([x[0] for x in want]) if n else dst)
    assert (v6.tolist(), ds.tolist(), tx.tolist()) == ([x[1] for x in want], [x[2] for x in want], [x[3] for x in want])
    assert nbufs.tolist() == want_nbufs.tolist()
    w.check()
    return rows, ds.tolist()


def mark(w: World, rows):
    """markEndpointSrcForClearing: the expire call's flag, set here as the host's route listener sets it."""
    for r in rows:
        w.timers["flags"][r] |= CLEAR_SRC
    w.ref_mark(rows)


def test_send_with_no_endpoint_and_the_flag_set_the_flag_stays():
    w = World(np.random.default_rng(5))
    p0 = w.ids[0]
    mark(w, [0])
    _, ds = dst_jobs(w, [(p0, 2, 0, True, [48, 64])])
    assert ds == [ERR_NO_ENDPOINT] and w.timers["flags"][0] & CLEAR_SRC
    set_received(w, [(p0, 0)], [A])  # SetEndpointFromPacket puts clearSrcOnTx back to false
    assert not w.timers["flags"][0] & CLEAR_SRC
    dst_jobs(w, [(p0, 2, 0, True, [48, 64])])
    assert w.ref[0].val == A


def test_send_with_the_flag_set_and_three_jobs_of_the_peer_then_set_restores_the_source():
    w = World(np.random.default_rng(6))
    p0, p1 = w.ids[0], w.ids[1]
    set_received(w, [(p0, 0), (p1, 1)], [A, C6])
    mark(w, [0])
    dst_jobs(w, [(p0, 1, 0, True, [100]), (p1, 3, 0, True, [32, 32, 32]), (p0, 2, 0, True, [1, 2]), (p0, 1, 0, True, [5]),
                 (p0, 1, 0, False, [5]), (p0, 0, 0, True, []), (p0, 4, 0, True, [1, 1, 1]), (p1, 1, -5, True, [7]),
                 (0, 1, 0, True, [7])])
    assert w.ref[0].val == (A[0], b"") and w.ref[1].val == C6 and not w.timers["flags"][0] & CLEAR_SRC
    set_received(w, [(p0, 0)], [A])  # set after clear
    assert w.ref[0].val == A


def test_dst_of_initiations_and_responses():
    w = World(np.random.default_rng(7))
    set_accepted(w, [(0, 1), (1, 2)], [A, C6])
    mark(w, [1, 3])
    for kind, dtype, ok, fn in (("init", noise.HS_START_DTYPE, HS_INITIATED, ep.dst_initiated_host),
                                ("resp", noise.HS_RESP_DTYPE, HS_RESPONDED, ep.dst_responded_host)):
        d = np.zeros(6, dtype)
        d["peer_row"] = [1, 2, 3, 1, w.n_peers, 2]
        status = np.array([ok, ok, ok, ok, ok, HS_NONE], np.int32)
        want = [w.ref_send(r if r < w.n_peers and s == ok else None) for r, s in zip(d["peer_row"].tolist(), status.tolist())]
        dst, v6, ds = fn(d, status, w.table, w.timers)
        same(dst, np.concatenate([x[0] for x in want]))
        assert (v6.tolist(), ds.tolist()) == ([x[1] for x in want], [x[2] for x in want])
        assert ds.tolist() == [0, 0, ERR_NO_ENDPOINT, 0, 0, 0] and v6.tolist() == [0, 1, 0, 0, 0, 0]
        w.check()
    assert w.timers["flags"][3] & CLEAR_SRC and not w.timers["flags"][1] & CLEAR_SRC


# ---------------------------------------------------------------- argument checks of the host forms
def test_host_forms_refuse_bad_arguments():
    L = _lib.load()
    w = World(np.random.default_rng(8))
    t, c, m = w.table.ctypes.data, w.claim.ctypes.data, w.timers.ctypes.data
    e, g = ep_rows([A, B]), w.groups([(w.ids[0], 0)])
    ok = [g.ctypes.data, 1, 1, e.ctypes.data, 2, w.peer_rows.ctypes.data, w.n_ids, t, c, m, w.n_peers]
    assert L.wgcs_endpoint_set_received_host(*ok) == 0
    w.ref[0].set_endpoint_from_packet(A)
    for i, bad in ((0, None), (3, None), (5, None), (7, None), (8, None), (9, None), (3, e.ctypes.data + 2), (7, t + 1),
                   (9, m + 4), (3, t), (8, t), (10, (1 << 24) + 1), (1, (1 << 28) + 1)):
        assert L.wgcs_endpoint_set_received_host(*(ok[:i] + [bad] + ok[i + 1:])) == ERR_INVALID_ARG, i
    assert L.wgcs_endpoint_set_received_host(None, 0, 1, None, 0, None, 0, None, None, None, 0) == 0
    d, st = np.zeros(2, noise.HS_RESP_DTYPE), np.zeros(2, np.int32)
    out, v6, ds = np.zeros(2, ep.ENDPOINT_DTYPE), np.zeros(2, np.int32), np.zeros(2, np.int32)
    ok = [d.ctypes.data, st.ctypes.data, 2, t, m, w.n_peers, out.ctypes.data, v6.ctypes.data, ds.ctypes.data]
    assert L.wgcs_endpoint_dst_responded_host(*ok) == 0
    for i, bad in ((0, None), (1, None), (3, None), (4, None), (6, None), (7, None), (8, None), (6, t), (7, v6.ctypes.data + 2),
                   (8, v6.ctypes.data), (4, m + 4)):
        assert L.wgcs_endpoint_dst_responded_host(*(ok[:i] + [bad] + ok[i + 1:])) == ERR_INVALID_ARG, i
    a, sz, nn, oob = np.zeros(2, SRC_ADDR_DTYPE), np.ones(2, np.int32), np.zeros(2, np.int32), np.zeros(16, np.uint8)
    ok = [a.ctypes.data, None, sz.ctypes.data, oob.ctypes.data, 8, nn.ctypes.data, 2, 1, out.ctypes.data, None]
    assert L.wgcs_endpoint_recv_host(*ok) == 0
    for i, bad in ((0, None), (2, None), (3, None), (5, None), (8, None), (4, 6), (8, out.ctypes.data + 1), (8, a.ctypes.data),
                   (9, out.ctypes.data)):
        assert L.wgcs_endpoint_recv_host(*(ok[:i] + [bad] + ok[i + 1:])) == ERR_INVALID_ARG, i
    w.check()


# ---------------------------------------------------------------- random sequences
def expire(w: World, rng, now: int):
    """wgcs_timers_expire_host with the newHandshake timer due for some peers: its body marks the source."""
    due = [r for r in range(w.n_peers) if rng.random() < 0.4]
    for r in due:
        w.timers["pending"][r] |= 1 << tm.TIMER_NEW_HANDSHAKE
        w.timers["deadline_ns"][r, tm.TIMER_NEW_HANDSHAKE] = now - 1
    n = w.n_peers
    table = np.zeros(n, noise.PEER_KEY_DTYPE)
    table["peer"] = w.ids
    empty = np.zeros(0, router.SESSION_SLOT_DTYPE)
    ka = [np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    tm.expire_host(now, w.timers, rekey.rekey_table(n, now), table, None, np.zeros(n, keypairs.KEYPAIRS_DTYPE), empty,
                   empty.copy(), np.zeros(0, tm.AEAD_KEY_DTYPE), np.zeros(0, np.uint32), *ka, np.zeros(1, np.uint32),
                   np.zeros(n, np.uint32))
    assert all(w.timers["flags"][r] & CLEAR_SRC for r in due)
    w.ref_mark(due)
    w.check()


def test_random_sequences():
    multi = cleared = no_endpoint = split_carried = 0
    for seed in range(200):
        rng = np.random.default_rng(3000 + seed)
        w = World(rng)
        now = NOW + seed
        for _ in range(int(rng.integers(6, 13))):
            now += SECOND
            what = rng.choice(["recv+received", "accepted", "finished", "jobs", "init", "resp", "expire"],
                              p=[.3, .1, .1, .25, .05, .05, .15])
            if what == "recv+received":
                n_msgs, nb = 6, 2
                n = n_msgs * nb
                addrs = [ADDRS[int(rng.integers(0, 4))] for _ in range(n)]
                src_from = [int(rng.choice([-1, -1, int(rng.integers(0, n_msgs)), 9])) for _ in range(n)]
                sizes = [int(rng.choice([0, 32, 148])) for _ in range(n)]
                cases = list(control_cases().values())
                controls = [cases[int(rng.integers(0, len(cases)))] for _ in range(n)]
                eps = recv(addrs, src_from, sizes, controls, n_msgs)
                split_carried += sum(e is not None and 0 <= f < n_msgs for e, f in zip(eps, src_from))
                rows = [(int(rng.choice(w.ids + [0, PEER_NONE])), int(rng.integers(-1, n + 1))) for _ in range(8)]
                hit = [w.row_of_id(p) for p, t in rows if 0 <= t < n and eps[t] is not None and w.row_of_id(p) is not None]
                multi += len(hit) != len(set(hit))
                set_received(w, rows, eps, calls_per_batch=4)
            elif what == "accepted":
                eps = random_endpoints(rng, 6)
                set_accepted(w, [(int(rng.integers(0, 8)), int(rng.integers(0, w.n_peers + 1))) for _ in range(5)], eps)
            elif what == "finished":
                eps = random_endpoints(rng, 5)
                set_finished(w, [rng.choice([None, 0, 1, 2, 3, 4, 9]) for _ in range(5)],
                             [int(rng.choice([HS_FINISHED, HS_NONE, -18], p=[.8, .1, .1])) for _ in range(5)], eps)
            elif what == "jobs":
                jobs = [(int(rng.choice(w.ids + [0])), int(rng.integers(0, 5)), int(rng.choice([0, 0, 0, -26])),
                         bool(rng.random() < 0.9), [int(x) for x in rng.integers(32, 1500, 3)]) for _ in range(6)]
                before = [p.clear_src_on_tx and p.val is not None and p.val[1] != b"" for p in w.ref]
                rows, ds = dst_jobs(w, jobs)
                no_endpoint += ds.count(ERR_NO_ENDPOINT)
                cleared += sum(before[r] for r in set(rows) if r is not None)
            elif what in ("init", "resp"):
                dtype, ok, fn = ((noise.HS_START_DTYPE, HS_INITIATED, ep.dst_initiated_host) if what == "init" else
                                 (noise.HS_RESP_DTYPE, HS_RESPONDED, ep.dst_responded_host))
                d = np.zeros(4, dtype)
                d["peer_row"] = rng.integers(0, w.n_peers + 1, 4)
                status = rng.choice([ok, HS_NONE], 4, p=[.8, .2]).astype(np.int32)
                want = [w.ref_send(r if r < w.n_peers and s == ok else None) for r, s in zip(d["peer_row"].tolist(), status.tolist())]
                dst, v6, ds = fn(d, status, w.table, w.timers)
                same(dst, np.concatenate([x[0] for x in want]))
                assert (v6.tolist(), ds.tolist()) == ([x[1] for x in want], [x[2] for x in want])
                w.check()
            else:
                expire(w, rng, now)
    # conditions on the generator, which the restatement alone reaches
    assert multi > 0 and cleared > 0 and no_endpoint > 0 and split_carried > 0
    assert min(multi, cleared, no_endpoint, split_carried) >= 20
