"""The one-lane-per-entry kernel (wireguard_amd/csrc/wgcs_each.h) at its edges:
one call of every family that runs through it -- timers received, the rekey
send gate writing its status in place, the cookie generator's responded and the
endpoints' set_received -- over 1, 255, 256, 257 and 513 entries against a
peer table of three rows, so every peer recurs on both sides of a block of 256.

What the row rules compute is pinned elsewhere (tests/test_*_ref.py and the
test_gpu_* file of each family); here the grid's edge and the passing of a body
by value are what can go wrong.  Every table and every output on the device
has 64 rows of 0xEE behind its last row, which must keep their fill, and its
rows are compared byte for byte with the host form's.  The CPU tests run first
in file order and pin the host forms of these shapes to the restatements of the
reference."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rekey_cases
import timers_cases
from cookiegen_cases import World as CookieWorld, sent_arrays
from endpoint_cases import CLEAR_SRC, World as EndpointWorld, ep_rows, random_endpoints
from rekey_ref import HS_RESPONDED, PEER_NONE, SECOND
from timers_ref import GROUP_DATA
from wireguard_amd import cookiegen as cg, endpoint as ep, rekey, timers

NS = (1, 255, 256, 257, 513)
SPARE, FILL = 64, 0xEE
NOW = timers_cases.NOW
N_PEERS = 3


def up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def up_spare(a) -> torch.Tensor:
    """a on the device with SPARE rows of fill behind it"""
    a = np.ascontiguousarray(a)
    return up(np.concatenate([a.view(np.uint8).reshape(-1), np.full(SPARE * a.dtype.itemsize, FILL, np.uint8)]))


def rows_of(t: torch.Tensor, like: np.ndarray) -> bytes:
    """the bytes of the rows in front of the spare ones, which must have kept their fill"""
    b, n = t.cpu().numpy(), like.nbytes
    assert len(b) == n + SPARE * like.dtype.itemsize and (b[n:] == FILL).all(), "rows past the call's were written"
    return b[:n].tobytes()


def peer_of(ids, c: int) -> int:
    """entry c's peer id: the three peers in turn, now and then an id without a row or no id at all"""
    return 11 if c % 13 == 5 else PEER_NONE if c % 17 == 9 else int(ids[c % N_PEERS])


# ---------------------------------------------------------------- the shapes, host form and restatement
@functools.lru_cache(maxsize=None)
def timers_received(n: int):
    """(world, step, the timers table the host form leaves), the restatement agreeing"""
    w = timers_cases.world(N_PEERS, 8, keepalive_interval_s=25)
    w.timers["flags"][1] = 0  # not active
    groups = [(peer_of(w.ids, c), -1 if c % 7 == 3 else c % 5, GROUP_DATA if c % 3 else 0) for c in range(n)]
    s = timers_cases.rcvd_step(groups, NOW, 1, seed=n)
    st = timers_cases.state_of(w)
    d = timers_cases.device_of(w, st)
    timers_cases.run_ref(d, w, s, st.rekey.copy(), st.key_peer.copy())
    timers_cases.run_host(w, st, s)
    assert st.timers.tobytes() == d.render().tobytes()
    return w, s, st.timers


@functools.lru_cache(maxsize=None)
def rekey_send_gate(n: int):
    """(world, step, status_out and the rekey table of the host form), the restatement agreeing"""
    w = rekey_cases.world(N_PEERS, 8)
    rekey_cases.put(w, 0, "current", 1, 2, NOW - 200 * SECOND)  # past RejectAfterTime
    rekey_cases.put(w, 1, "current", 3, 4, NOW - 10 * SECOND)   # good; row 2 has no keypair
    jobs = [(peer_of(w.ids, j), (1, 2, 4, 0, 5, 3)[j % 6], -8 if j % 19 == 7 else 0) for j in range(n)]
    s = rekey_cases.gate_step(jobs, NOW, seed=n)
    st = rekey_cases.state_of(w)
    d = rekey_cases.device_of(w, st)
    want = rekey_cases.run_ref(d, st, s)["status_out"]
    got = rekey_cases.run_host(w, st, s)["status_out"]
    assert got.tobytes() == want.tobytes() and st.rekey.tobytes() == d.render().tobytes()
    return w, s, got, st.rekey


@functools.lru_cache(maxsize=None)
def cookie_responded(n: int):
    """(the gen table before, descriptors, status, msgs, the gen table of the host form), the restatement agreeing"""
    rng = np.random.default_rng(n)
    w = CookieWorld(rng, n_peers=N_PEERS).finish()
    peer_row = np.array([N_PEERS if j % 13 == 5 else 0xFFFFFFFF if j % 17 == 9 else j % N_PEERS for j in range(n)],
                        np.uint32)
    status = [HS_RESPONDED if j % 7 != 3 else 0 for j in range(n)]
    d, st, msgs, mac1s = sent_arrays(rng, "resp", peer_row, status)
    gen = w.gen.copy()
    cg.responded_host(d, st, msgs, gen)
    w.ref_sent(peer_row, st, HS_RESPONDED, mac1s)
    assert gen.tobytes() == w.want_gen().tobytes()
    return w.gen, d, st, msgs, gen


@functools.lru_cache(maxsize=None)
def endpoint_set_received(n: int):
    """(the tables before, groups, source rows, peer_rows, the tables the host form leaves), the restatement agreeing"""
    rng = np.random.default_rng(n)
    w = EndpointWorld(rng, n_peers=N_PEERS, n_ids=16)
    w.timers["flags"] |= CLEAR_SRC
    n_rows = 9
    endpoints = random_endpoints(rng, n_rows)
    # a tail may lie past the rows
    rows = [(peer_of(w.ids, c), -1 if c % 7 == 3 else c % (n_rows + 2)) for c in range(n)]
    g, eps = w.groups(rows), ep_rows(endpoints)
    before = SimpleNamespace(table=w.table.copy(), claim=w.claim.copy(), timers=w.timers.copy())
    ep.set_received_host(g, 1, eps, w.peer_rows, w.table, w.claim, w.timers)
    w.ref_set([(w.row_of_id(peer) if tail >= 0 else None, tail) for peer, tail in rows], endpoints)
    w.check()
    return before, g, eps, w.peer_rows, w


@pytest.mark.parametrize("n", NS)
def test_host_forms_agree_with_the_restatements(n):
    timers_received(n), rekey_send_gate(n), cookie_responded(n), endpoint_set_received(n)
    if n > 256:  # the peers behind the first block have entries in it too: all three of them at 513
        w, s, _ = timers_received(n)
        first, rest = ({int(p) for p in s.groups["peer"][a:b]} & set(w.ids.tolist()) for a, b in ((0, 256), (256, n)))
        assert rest and rest <= first and (n < 513 or len(rest) == N_PEERS)


# ---------------------------------------------------------------- the device forms
@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_timers_received(dev, n):
    w, s, want = timers_received(n)
    d_groups, d_rows, d_timers = up(s.groups), up(w.peer_rows), up_spare(w.timers)
    timers.received_batch(dev, d_groups, 1, s.now, d_rows, d_timers, n_batches=n, n_ids=w.n_ids, n_peers=N_PEERS)
    torch.cuda.synchronize()
    assert rows_of(d_timers, want) == want.tobytes()
    assert d_groups.cpu().numpy().tobytes() == s.groups.tobytes()
    assert d_rows.cpu().numpy().tobytes() == w.peer_rows.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_rekey_send_gate_in_place(dev, n):
    w, s, want_status, want_rekey = rekey_send_gate(n)
    d_status, d_rekey = up_spare(s.status_in), up_spare(w.rekey)  # d_status_out is d_status_in
    d_kp = up(w.kp)
    rekey.send_gate_batch(dev, up(s.peer), up(s.count), d_status, s.max_segs, s.now, up(w.peer_rows), d_kp,
                          up(w.send_nonce), s.limit, d_rekey, d_status, n_jobs=n, n_ids=w.n_ids, n_peers=N_PEERS,
                          n_keys=w.n_keys)
    torch.cuda.synchronize()
    assert rows_of(d_status, want_status) == want_status.tobytes()
    assert rows_of(d_rekey, want_rekey) == want_rekey.tobytes()
    assert d_kp.cpu().numpy().tobytes() == w.kp.tobytes()
    assert want_status.tobytes() != s.status_in.tobytes() or n == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_cookie_responded(dev, n):
    before, d, st, msgs, want = cookie_responded(n)
    d_gen, d_msgs = up_spare(before), up(msgs)
    cg.responded_batch(dev, up(d), up(st), d_msgs, d_gen, n=n, n_peers=N_PEERS)
    torch.cuda.synchronize()
    assert rows_of(d_gen, want) == want.tobytes()
    assert d_msgs.cpu().numpy().tobytes() == msgs.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_endpoint_set_received(dev, n):
    before, g, eps, peer_rows, w = endpoint_set_received(n)
    d_table, d_claim, d_timers = up_spare(before.table), up_spare(before.claim), up_spare(before.timers)
    d_eps = up(eps)
    ep.set_received_batch(dev, up(g), 1, d_eps, up(peer_rows), d_table, d_claim, d_timers, n_batches=n, n_rows=len(eps),
                          n_ids=len(peer_rows), n_peers=N_PEERS)
    torch.cuda.synchronize()
    assert rows_of(d_table, w.table) == w.table.tobytes()
    assert rows_of(d_claim, w.claim) == w.claim.tobytes() and not w.claim.any()
    assert rows_of(d_timers, w.timers) == w.timers.tobytes()
    assert d_eps.cpu().numpy().tobytes() == eps.tobytes()
