"""wgcs_handshake_accept_host and wgcs_peer_rows_build (noise.cpp, the row
functions of wgcs_noise.h) against tests/noise_accept_ref.py, the sequential
restatement of device/noise.go:458-491 under a fixed clock (CPU only).

Every step of every case is compared whole: each verdict, the whole peer table,
the whole descriptor array and the count.  The host form writes into buffers
filled with a sentinel, so what it must write and what it must leave is both in
the comparison."""
import os
import subprocess

import numpy as np
import pytest

import noise_accept_cases as cases
import noise_accept_ref as ref
from noise_accept_cases import CLAIM_NONE, FILL, MS, NOW, T
from noise_accept_ref import ERR_BATCH_FULL, ERR_FLOOD, ERR_NO_PEER, ERR_REPLAY, HS_ACCEPTED, HS_CONSUMED
from wireguard_amd import _lib, noise
from wireguard_amd.noise import HS_PEER_DTYPE, HS_RESP_DTYPE, HS_TICKET_DTYPE

SPARE = 2  # verdict rows past the batch: they keep their fill


def host(c, s, peers):
    """(verdict with its spare rows, peers, resp, count) of the host form for step s on a copy of peers."""
    p = peers.copy()
    verdict = np.full(len(s.init) + SPARE, 12345, np.int32)
    resp = np.full(80 * len(s.tickets), FILL, np.uint8).view(HS_RESP_DTYPE)
    count = np.full(1, 0xEEEEEEEE, np.uint32)
    noise.accept_host(s.init, s.gate, s.now, c.table, c.peer_rows, p, s.tickets, resp, count, verdict)
    return verdict, p, resp, int(count[0])


def run(c):
    """Every step of c through the host form and the restatement, compared; the restatement's verdicts per step."""
    peers, out = c.peers, []
    for k, s in enumerate(c.steps):
        want_v, want_p, want_r, want_n = ref.accept(s.init, s.gate, s.now, c.table, c.peer_rows, peers, s.tickets)
        v, p, r, n = host(c, s, peers)
        where = f"{c.name} step {k}"
        assert v[:len(s.init)].tolist() == want_v.tolist(), where
        assert (v[len(s.init):] == 12345).all(), where
        assert n == want_n, where
        assert r.tobytes() == want_r.tobytes(), where
        assert p.tobytes() == want_p.tobytes(), where
        assert (p["claim"] == CLAIM_NONE).all(), where
        peers = p
        out.append(want_v.tolist())
    return out, peers


NAMED = {c.name: c for c in cases.named()}
A, R, F, NP, FULL = HS_ACCEPTED, ERR_REPLAY, ERR_FLOOD, ERR_NO_PEER, ERR_BATCH_FULL
# what the rules give, worked out by hand from noise.go:458-491: the restatement is checked too
WANT = {
    "n_1": [[A]],
    "fresh_peers": [[A, A, R, A]],
    "flooding_at_exactly_20_ms": [[F, A]],
    "clock_went_back": [[F, R, A]],
    "three_rising": [[A, F, F]],
    "equal_to_the_winner": [[A, R, R, F]],
    "old_row_in_front_of_the_winner": [[R, R, A, F, R]],
    "ids_without_a_peer": [[NP, NP, NP, NP, NP, NP, A, NP]],
    "gated_rows_are_not_read": [[0, A, -18, 7, A, F, 1, -23, R]],
    "fewer_tickets_than_winners": [[A, A, FULL, R, FULL, R, R, F, F], [A, A, F]],
    "no_tickets": [[FULL, FULL, F]],
    "more_tickets_than_rows": [[A, R]],
    "no_rows": [[]],
    "second_call_later": [[A, A, F], [R, A, R, A, A]],
    "the_same_call_again_within_20_ms": [[A, A, F, A], [R, R, F, R], [R, R, A, R]],
}


def test_every_named_case_is_listed():
    assert sorted(NAMED) == sorted(WANT)


@pytest.mark.parametrize("name", sorted(WANT))
def test_named_case(name):
    got, _ = run(NAMED[name])
    assert got == WANT[name]


def test_a_committed_winner_writes_the_state_and_its_descriptor():
    c = NAMED["fewer_tickets_than_winners"]
    s = c.steps[0]
    v, p, r, n = host(c, s, c.peers)
    assert n == 2 and r["init_row"].tolist() == [0, 1] and r["peer_row"].tolist() == [0, 2]
    for j, (q, row) in enumerate(((0, 0), (1, 2))):
        assert p["last_timestamp"][row].tobytes() == s.init["timestamp"][q].tobytes()
        assert p["last_consumption_ns"][row] == s.now and p["remote_index"][row] == s.init["sender"][q]
        assert p["state"][row] == noise.HS_PEER_CONSUMED and p["flags"][row] & noise.HS_PEER_SEEN
        for f in ("local_index", "send_key", "recv_key"):
            assert r[f][j] == s.tickets[f][j]
        assert r["ephemeral_private"][j].tobytes() == s.tickets["ephemeral_private"][j].tobytes()
        has = bool(c.peers["flags"][row] & noise.HS_PEER_COOKIE)
        assert r["flags"][j] == int(has) and r["cookie"][j].tobytes() == (c.peers["cookie"][row].tobytes() if has else bytes(16))
        assert not r["pad"][j].any()
    assert {bool(c.peers["flags"][row] & noise.HS_PEER_COOKIE) for row in (0, 2)} == {True, False}
    # the winners without a ticket left their peers as they were
    for row in (1, 4):
        assert p[row].tobytes() == c.peers[row].tobytes()


def test_the_tail_descriptors_hold_no_ticket_secret():
    c = NAMED["more_tickets_than_rows"]
    _, _, r, n = host(c, c.steps[0], c.peers)
    assert n == 1
    tail = np.zeros(4, HS_RESP_DTYPE)
    tail["init_row"] = 0xFFFFFFFF
    assert r[1:].tobytes() == tail.tobytes()
    c = NAMED["no_rows"]
    _, p, r, n = host(c, c.steps[0], c.peers)
    assert n == 0 and r.tobytes() == tail[:3].tobytes() and p.tobytes() == c.peers.tobytes()


def test_the_same_call_again_moves_nothing():
    c = NAMED["the_same_call_again_within_20_ms"]
    s0, s1 = c.steps[0], c.steps[1]
    _, p0, _, _ = host(c, s0, c.peers)
    v, p1, r, n = host(c, s1, p0)
    assert n == 0 and p1.tobytes() == p0.tobytes() and HS_ACCEPTED not in v.tolist()
    assert (r["init_row"] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("block", range(10))
def test_random_batches(block):
    for seed in range(20 * block, 20 * block + 20):  # 200 in all
        run(cases.random_case(seed))


def test_random_batches_meet_every_verdict():
    seen = set()
    for seed in range(200):
        c = cases.random_case(seed)
        peers = c.peers
        for s in c.steps:
            v, peers, _, _ = ref.accept(s.init, s.gate, s.now, c.table, c.peer_rows, peers, s.tickets)
            seen.update(int(x) for x, g in zip(v, s.gate) if g == HS_CONSUMED)
    assert seen == {A, R, F, NP, FULL}


def test_the_wide_batch():
    c = cases.wide()
    got, _ = run(c)
    assert [got[0][q] for q in (3, 70, 290)] == [R, A, F]


def test_peer_rows_build():
    table, rows, n_ids = cases.table_of(5)
    assert len(rows) == n_ids
    for r in range(5):
        assert rows[table["peer"][r]] == r
    assert (rows == ref.PEER_NONE).sum() == n_ids - 5
    with pytest.raises(_lib.WgcsError) as ei:
        noise.peer_rows_build(table, int(table["peer"].max()))
    assert ei.value.code == -1
    assert len(noise.peer_rows_build(table[:0], 0)) == 0
    assert (noise.peer_rows_build(table[:0], 3) == ref.PEER_NONE).all()
    L = _lib.load()
    assert L.wgcs_peer_rows_build(None, 1, rows.ctypes.data, n_ids) == -1
    assert L.wgcs_peer_rows_build(table.ctypes.data, 5, None, n_ids) == -1


def test_accept_host_arguments():
    c = NAMED["three_rising"]
    s = c.steps[0]
    L = _lib.load()
    n = len(s.init)
    p = c.peers.copy()
    resp = np.zeros(len(s.tickets), HS_RESP_DTYPE)
    count, verdict = np.zeros(1, np.uint32), np.zeros(n, np.int32)
    args = [s.init.ctypes.data, s.gate.ctypes.data, n, s.now, c.table.ctypes.data, c.peer_rows.ctypes.data, c.n_ids,
            p.ctypes.data, len(p), s.tickets.ctypes.data, len(s.tickets), resp.ctypes.data, count.ctypes.data,
            verdict.ctypes.data]
    assert L.wgcs_handshake_accept_host(*args) == 0
    for k in (0, 1, 4, 5, 7, 9, 11, 12, 13):
        bad = list(args)
        bad[k] = None
        assert L.wgcs_handshake_accept_host(*bad) == -1, k
    bad = list(args)
    bad[13] = args[1]  # verdict == gate
    assert L.wgcs_handshake_accept_host(*bad) == -1
    bad = list(args)
    bad[2] = (1 << 28) + 1
    assert L.wgcs_handshake_accept_host(*bad) == -1


def test_header_layouts(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "wgcsum.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(wgcs_hs_peer) == 64 && _Alignof(wgcs_hs_peer) == 4, "peer");\n'
                   '_Static_assert(offsetof(wgcs_hs_peer, state) == 12 && offsetof(wgcs_hs_peer, last_consumption_ns) == 16 && '
                   'offsetof(wgcs_hs_peer, flags) == 24 && offsetof(wgcs_hs_peer, remote_index) == 28 && '
                   'offsetof(wgcs_hs_peer, claim) == 32 && offsetof(wgcs_hs_peer, cookie) == 36 && '
                   'offsetof(wgcs_hs_peer, pad) == 52, "peer fields");\n'
                   '_Static_assert(sizeof(wgcs_hs_ticket) == 48 && offsetof(wgcs_hs_ticket, ephemeral_private) == 16, "ticket");\n'
                   '_Static_assert(WGCS_HS_ACCEPTED == 7 && WGCS_ERR_FLOOD == -25 && WGCS_HS_PEER_ZEROED == 0 && '
                   'WGCS_HS_PEER_CONSUMED == 1, "codes");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o",
                    str(tmp_path / "t")], check=True)
    for f, off in (("state", 12), ("last_consumption_ns", 16), ("flags", 24), ("remote_index", 28), ("claim", 32),
                   ("cookie", 36), ("pad", 52)):
        assert HS_PEER_DTYPE.fields[f][1] == off
    assert HS_TICKET_DTYPE.fields["ephemeral_private"][1] == 16
    assert (_lib.HS_ACCEPTED, _lib.ERR_FLOOD) == (7, -25) and NOW > 0 and MS and T
