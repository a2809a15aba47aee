"""The peer endpoints on the GPU (wgcs_endpoint_recv_batch, the three _set_*_batch,
the three _dst_*_batch and wgcs_coalesce_messages_dst_batch; the kernels of
endpoint_kernels.hip and udp_msgs_kernels.hip) against the host forms of
endpoint.cpp: every output and every table compared whole.
tests/test_endpoint_ref.py pins the host forms to the restatement of the
reference.

Every output sits between sentinel bytes that must keep their fill, and every
read-only input is compared with its upload afterwards.  The set and dst calls
run 3 peers over 600 rows, so one peer's rows lie in different waves and in
different blocks of 256: a commit or a clear that depended on their order would
show."""
import numpy as np
import pytest
import torch

import oracle
from conn_cases import Msg
from endpoint_cases import (ADDRS, CLEAR_SRC, OOB_STRIDE, World, addr_row, control_cases, ep_rows, finished_rows, oob_of,
                            random_endpoints)
from wireguard_amd import endpoint as ep, noise, timers as tm
from wireguard_amd._lib import (ERR_INVALID_ARG, ERR_NO_ENDPOINT, HS_FINISHED, HS_INITIATED, HS_NONE, HS_RESPONDED,
                                PEER_NONE, WgcsError)
from wireguard_amd.cookie import SRC_ADDR_DTYPE

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
N = 600


class Guarded:
    """A device buffer with GUARD sentinel bytes in front of and behind its payload."""

    def __init__(self, payload):
        b = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.n = len(b)
        self.whole = torch.from_numpy(np.concatenate([np.full(GUARD, FILL, np.uint8), b, np.full(GUARD, FILL, np.uint8)])).cuda()
        self.t = self.whole[GUARD:GUARD + self.n]

    def get(self, dtype) -> np.ndarray:
        a = self.whole.cpu().numpy()
        assert (a[:GUARD] == FILL).all() and (a[GUARD + self.n:] == FILL).all(), "sentinel bytes were written"
        return a[GUARD:GUARD + self.n].copy().view(dtype)


def up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def same(a, b):
    assert a.tobytes() == b.tobytes()


def filled(n: int, dtype, byte: int = 0xEE) -> np.ndarray:
    return np.full(n * np.dtype(dtype).itemsize, byte, np.uint8).view(dtype)


class Tables:
    """A world's three tables on the device, guarded."""

    def __init__(self, w: World):
        self.w = w
        self.table, self.claim, self.timers = Guarded(w.table), Guarded(w.claim), Guarded(w.timers)
        self.peer_rows = up(w.peer_rows)

    def check(self):
        """The device tables are the world's, which the host forms have written."""
        same(self.table.get(ep.ENDPOINT_DTYPE), self.w.table)
        same(self.timers.get(tm.TIMERS_DTYPE), self.w.timers)
        assert not self.claim.get(np.uint32).any() and not self.w.claim.any()
        same(self.peer_rows.cpu().numpy(), self.w.peer_rows)


def world3(seed: int, endpoints=True) -> World:
    """Three peers; peers 0 and 1 have an endpoint unless told otherwise, peer 2 never has one."""
    w = World(np.random.default_rng(seed), n_peers=3, n_ids=8)
    if endpoints:
        w.table[0] = ep.row(ADDRS[0][:4], 40001, control_cases()["pktinfo4"])[0]
        w.table[1] = ep.row(ADDRS[1][:16], 7, control_cases()["pktinfo6"])[0]
    return w


# ---------------------------------------------------------------- recv
def test_recv_three_batches_of_eight_with_every_control_case(dev):
    rng = np.random.default_rng(10)
    n_msgs, nb = 8, 3
    n = n_msgs * nb
    cases = list(control_cases().values())
    controls = [cases[q % len(cases)] for q in range(n)]
    assert len(cases) <= n
    addrs = np.concatenate([addr_row(ADDRS[int(rng.integers(0, 4))]) for _ in range(n)])
    # slots 0..15 meet every control case live and split-carried (the address of another slot of the batch, the
    # slot's own control); the last batch has the slots of size 0, the d_from out of range and the slots of their own
    src_from = np.array([(3 * q + 1) % n_msgs for q in range(16)] + [-1, 8, -2, -1, 7, 100, -1, 0], np.int32)
    size = np.array([148, 92, 32, 64, 9, 1, 1500, 33] * 2 + [0, 9, 9, 32, 0, 9, 1, 64], np.int32)
    assert all(src_from[q] != q % n_msgs for q in range(16)) and len(cases) == 16
    oob, nn = oob_of(controls)
    nn[19], nn[22] = -1, OOB_STRIDE + 4  # outside [0, oob_stride]: no control
    for frm in (src_from, None):
        want_ep, want_addr = ep.recv_host(addrs, frm, size, oob, OOB_STRIDE, nn, n_msgs, nb)
        d_in = [up(addrs), None if frm is None else up(frm), up(size), up(oob), up(nn)]
        d_ep, d_out = Guarded(filled(n, ep.ENDPOINT_DTYPE)), Guarded(filled(n, SRC_ADDR_DTYPE))
        ep.recv_batch(dev, d_in[0], d_in[1], d_in[2], d_in[3], OOB_STRIDE, d_in[4], n_msgs, nb, d_ep.t, d_out.t)
        torch.cuda.synchronize()
        same(d_ep.get(ep.ENDPOINT_DTYPE), want_ep), same(d_out.get(SRC_ADDR_DTYPE), want_addr)
        for t, h in zip(d_in, (addrs, frm, size, oob, nn)):
            if t is not None:
                same(t.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8))
        assert set(want_ep["src_len"].tolist()) == {0, 32, 40} and (want_ep["dst"]["len"] == 0).any()
    # without the dense table, and over more than a block of slots
    big = 300
    addrs = np.concatenate([addr_row(ADDRS[q % 4]) for q in range(big)])
    oob, nn = oob_of([cases[q % len(cases)] for q in range(big)])
    size = np.ones(big, np.int32)
    want_ep, _ = ep.recv_host(addrs, None, size, oob, OOB_STRIDE, nn, big, 1)
    d_ep = Guarded(filled(big, ep.ENDPOINT_DTYPE))
    ep.recv_batch(dev, up(addrs), None, up(size), up(oob), OOB_STRIDE, up(nn), big, 1, d_ep.t, None)
    torch.cuda.synchronize()
    same(d_ep.get(ep.ENDPOINT_DTYPE), want_ep)


# ---------------------------------------------------------------- set
def test_set_calls_three_peers_over_600_candidate_rows(dev):
    rng = np.random.default_rng(20)
    w = world3(21, endpoints=False)
    w.timers["flags"] |= CLEAR_SRC
    tb = Tables(w)
    eps = ep_rows(random_endpoints(rng, N))
    eps["dst"]["len"][17] = 5  # not an address: no candidate
    d_eps = up(eps)

    # received: 150 batches of 4 group rows; peers 0 and 1 in every block, unused rows and unknown ids between them
    groups = w.groups([(int(rng.choice(w.ids[:2] + [0, PEER_NONE])), int(rng.integers(-1, N + 2))) for _ in range(N)])
    ep.set_received_host(groups, 4, eps, w.peer_rows, w.table, w.claim, w.timers)
    d_groups = up(groups)
    ep.set_received_batch(dev, d_groups, 4, d_eps, tb.peer_rows, tb.table.t, tb.claim.t, tb.timers.t, n_batches=N // 4,
                          n_rows=N, n_ids=w.n_ids, n_peers=3)
    torch.cuda.synchronize()
    tb.check()
    same(d_groups.cpu().numpy(), groups.view(np.uint8))
    assert (w.table["dst"]["len"][:2] != 0).all() and w.table["dst"]["len"][2] == 0
    assert (w.timers["flags"] & CLEAR_SRC).tolist() == [0, 0, CLEAR_SRC]

    # accepted: descriptors of all three peers, tail rows and rows past the tables
    d = np.zeros(N, noise.HS_RESP_DTYPE)
    d["init_row"] = rng.choice([0, 5, 17, 300, 599, 600, 0xFFFFFFFF], N)
    d["peer_row"] = rng.choice([0, 1, 2, 3], N)
    ep.set_accepted_host(d, eps, w.table, w.claim, w.timers)
    d_d = up(d)
    ep.set_accepted_batch(dev, d_d, d_eps, tb.table.t, tb.claim.t, tb.timers.t, n_tickets=N, n_rows=N, n_peers=3)
    torch.cuda.synchronize()
    tb.check()
    same(d_d.cpu().numpy(), d.view(np.uint8))
    assert w.table["dst"]["len"][2] != 0

    # finished: responses for handshakes of the three peers, refused rows and unknown receivers among them
    peer_rows = [rng.choice([None, 0, 1, 2, 7]) for _ in range(N)]
    gates = [int(rng.choice([HS_FINISHED, HS_NONE, -18], p=[.8, .1, .1])) for _ in range(N)]
    arena, pkts, gate, hs_slots, states = finished_rows(rng, w, peer_rows, gates)
    before = w.table.copy()
    ep.set_finished_host(arena, pkts, gate, hs_slots, states, eps, w.table, w.claim, w.timers)
    ro = [up(arena), up(pkts), up(gate), up(hs_slots), up(states)]
    ep.set_finished_batch(dev, ro[0], ro[1], ro[2], ro[3], ro[4], d_eps, tb.table.t, tb.claim.t, tb.timers.t, n=N,
                          n_hs_slots=len(hs_slots), n_states=len(states), n_peers=3)
    torch.cuda.synchronize()
    tb.check()
    for t, h in zip(ro, (arena, pkts, gate, hs_slots, states)):
        same(t.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8))
    same(d_eps.cpu().numpy(), eps.view(np.uint8))
    assert w.table.tobytes() != before.tobytes()


# ---------------------------------------------------------------- dst
def test_dst_calls_three_peers_over_600_entries(dev):
    rng = np.random.default_rng(30)
    max_segs = 3
    for flags in ([CLEAR_SRC, 0, CLEAR_SRC], [0, CLEAR_SRC, 0]):
        w = world3(31)
        w.timers["flags"] |= np.array(flags, np.uint32)
        tb = Tables(w)
        peer = np.full(N * max_segs, PEER_NONE, np.uint32)
        peer[::max_segs] = rng.choice(w.ids + [0], N)
        count = rng.choice([0, 1, 2, 3, 4], N, p=[.05, .3, .3, .3, .05]).astype(np.int32)
        status = rng.choice([0, -26], N, p=[.9, .1]).astype(np.int32)
        key = rng.choice([3, 0xFFFFFFFF], N, p=[.9, .1]).astype(np.uint32)
        lens = rng.integers(-5, 1500, N * max_segs).astype(np.int32)
        nbufs = np.where((status == 0) & (key != 0xFFFFFFFF) & (count >= 1) & (count <= max_segs), count, 0).astype(np.int32)
        d_nbufs = Guarded(nbufs)
        ro = [up(peer), up(count), up(status), up(key), up(lens)]
        want = ep.dst_jobs_host(peer, count, status, key, max_segs, lens, nbufs, w.peer_rows, w.table, w.timers)
        out = [Guarded(filled(N, ep.ENDPOINT_DTYPE)), Guarded(filled(N, np.int32)), Guarded(filled(N, np.int32)),
               Guarded(filled(N, np.uint64))]
        ep.dst_jobs_batch(dev, ro[0], ro[1], ro[2], ro[3], max_segs, ro[4], d_nbufs.t, tb.peer_rows, tb.table.t, tb.timers.t,
                          out[0].t, out[1].t, out[2].t, out[3].t, n_jobs=N, n_ids=w.n_ids, n_peers=3)
        torch.cuda.synchronize()
        for o, h, dt in zip(out, want, (ep.ENDPOINT_DTYPE, np.int32, np.int32, np.uint64)):
            same(o.get(dt), h)
        same(d_nbufs.get(np.int32), nbufs)
        tb.check()
        for t, h in zip(ro, (peer, count, status, key, lens)):
            same(t.cpu().numpy(), h.view(np.uint8))
        assert (want[2] == ERR_NO_ENDPOINT).sum() > 50 and want[1].sum() > 50 and want[3].max() > 0
        assert (w.timers["flags"] & CLEAR_SRC).tolist() == [0, 0, flags[2]]  # the peer without an endpoint keeps its flag
        assert w.table["src_len"].tolist() == [0 if flags[0] else 32, 0 if flags[1] else 40, 0]

    for kind, dtype, ok, host, batch in (("init", noise.HS_START_DTYPE, HS_INITIATED, ep.dst_initiated_host, ep.dst_initiated_batch),
                                         ("resp", noise.HS_RESP_DTYPE, HS_RESPONDED, ep.dst_responded_host, ep.dst_responded_batch)):
        w = world3(32)
        w.timers["flags"] |= np.array([0, CLEAR_SRC, CLEAR_SRC], np.uint32)
        tb = Tables(w)
        d = np.zeros(N, dtype)
        d["peer_row"] = rng.choice([0, 1, 2, 3, 0xFFFFFFFF], N)
        status = rng.choice([ok, HS_NONE, -1], N, p=[.8, .1, .1]).astype(np.int32)
        want = host(d, status, w.table, w.timers)
        d_d, d_st = up(d), up(status)
        out = [Guarded(filled(N, ep.ENDPOINT_DTYPE)), Guarded(filled(N, np.int32)), Guarded(filled(N, np.int32))]
        batch(dev, d_d, d_st, tb.table.t, tb.timers.t, out[0].t, out[1].t, out[2].t, n=N, n_peers=3)
        torch.cuda.synchronize()
        for o, h, dt in zip(out, want, (ep.ENDPOINT_DTYPE, np.int32, np.int32)):
            same(o.get(dt), h)
        tb.check()
        same(d_d.cpu().numpy(), d.view(np.uint8)), same(d_st.cpu().numpy(), status.view(np.uint8))
        assert w.table["src_len"].tolist() == [32, 0, 0] and (w.timers["flags"] & CLEAR_SRC).tolist() == [0, 0, CLEAR_SRC], kind


def test_row_counts_of_zero_and_bad_arguments(dev):
    w = world3(40)
    tb = Tables(w)
    eps = up(ep_rows(random_endpoints(np.random.default_rng(41), 4)))
    g = up(w.groups([(w.ids[0], 0)]))
    ep.set_received_batch(dev, None, 4, None, None, None, None, None, n_batches=0, n_rows=0, n_ids=0, n_peers=0)
    ep.recv_batch(dev, None, None, None, None, 8, None, 0, 3, None)
    out = [Guarded(filled(1, ep.ENDPOINT_DTYPE)), Guarded(filled(1, np.int32)), Guarded(filled(1, np.int32))]
    d, st = up(np.zeros(1, noise.HS_RESP_DTYPE)), up(np.array([HS_RESPONDED], np.int32))
    # a table of no rows: the entry takes no part, and its outputs are still written
    ep.dst_responded_batch(dev, d, st, None, None, out[0].t, out[1].t, out[2].t, n=1, n_peers=0)
    torch.cuda.synchronize()
    assert not out[0].get(np.uint8).any() and out[1].get(np.int32)[0] == 0 and out[2].get(np.int32)[0] == 0
    good = dict(groups=g, ep=eps, peer_rows=tb.peer_rows, tab=tb.table.t, claim=tb.claim.t, timers=tb.timers.t)
    bad = [{k: None} for k in good] + [dict(ep=eps[2:]), dict(tab=tb.table.t[1:]), dict(claim=tb.claim.t[2:]),
                                       dict(timers=tb.timers.t[4:]), dict(ep=tb.table.t), dict(claim=tb.table.t),
                                       dict(timers=tb.table.t)]
    for b in bad:
        a = {**good, **b}
        with pytest.raises(WgcsError) as e:
            ep.set_received_batch(dev, a["groups"], 1, a["ep"], a["peer_rows"], a["tab"], a["claim"], a["timers"],
                                  n_batches=1, n_rows=2, n_ids=w.n_ids, n_peers=2)
        assert e.value.code == ERR_INVALID_ARG, b
    for kw in (dict(dst=tb.table.t), dict(v6=out[2].t), dict(tab=tb.table.t[2:]), dict(dst=None)):
        a = {**dict(dst=out[0].t, v6=out[1].t, tab=tb.table.t), **kw}
        with pytest.raises(WgcsError) as e:
            ep.dst_responded_batch(dev, d, st, a["tab"], tb.timers.t, a["dst"], a["v6"], out[2].t, n=1, n_peers=2)
        assert e.value.code == ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    tb.check()


# ---------------------------------------------------------------- coalesce
@pytest.mark.parametrize("is6", [True, False])
def test_coalesce_messages_host_call_44_buffers_of_1489(dev, is6):
    """wgcs_coalesce_messages on host buffers: 65,516 bytes are one message to an IPv6 destination and
    two to an IPv4 one, with the source control in front of UDP_SEGMENT, as the oracle's."""
    from wireguard_amd import conn

    rng = np.random.default_rng(60)
    nbuf, size, cap = 44, 1489, 65535
    data = rng.integers(0, 256, (nbuf, size), dtype=np.uint8)
    src = control_cases()["pktinfo6" if is6 else "pktinfo4"]
    got_b, want_b = ([np.concatenate([data[j], np.zeros(cap - size, np.uint8)]) for j in range(nbuf)] for _ in range(2))
    got_m, want_m = ([Msg(np.zeros(1, np.uint8), 64) for _ in range(nbuf)] for _ in range(2))
    want = oracle.coalesce_messages(want_m, want_b, [size] * nbuf, src, "ep", is6)
    got = conn.coalesce_messages(dev, got_m, got_b, [size] * nbuf, src, "ep", is6)
    assert got == want == (1 if is6 else 2)
    for m in range(want):
        f = next(j for j, x in enumerate(want_b) if x is want_m[m].buf)
        assert got_m[m].buf is got_b[f] and got_m[m].buf_len == want_m[m].buf_len
        assert np.array_equal(got_b[f][:got_m[m].buf_len], want_b[f][:want_m[m].buf_len])
        assert got_m[m].oob_len == want_m[m].oob_len
        assert np.array_equal(got_m[m].oob[:got_m[m].oob_len], want_m[m].oob[:want_m[m].oob_len])
    assert want_m[0].oob_len == len(src) + 24  # setSrcControl, then setGSOSize


def test_coalesce_dst_a_v4_batch_and_a_v6_batch_in_one_call(dev):
    rng = np.random.default_rng(50)
    nbuf, size, stride, cap = 44, 1489, 65536, 65535
    assert nbuf * size == 65516  # past maxIPv4PayloadLen (65,507), within maxIPv6PayloadLen (65,527)
    bufs = rng.integers(0, 256, (nbuf, size), dtype=np.uint8)
    h = np.full((2 * nbuf, stride), 0xC3, np.uint8)
    h[:nbuf, :size] = h[nbuf:, :size] = bufs
    lens, nb = np.full(2 * nbuf, size, np.int32), np.full(2, nbuf, np.int32)

    def run(call):
        d = torch.from_numpy(h).cuda()
        d_lens, d_nb = torch.from_numpy(lens).cuda(), torch.from_numpy(nb).cuda()
        nm = torch.full((2,), 12345, dtype=torch.int32, device="cuda")
        first, mlen, gso = (torch.full((2 * nbuf,), 12345, dtype=torch.int32, device="cuda") for _ in range(3))
        call(d, d_lens, d_nb, nm, first, mlen, gso)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (d, nm, first, mlen, gso)]

    v6 = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    got = run(lambda d, l, n, nm, f, ml, g: ep.coalesce_dst_batch(dev, d, stride, cap, None, l, n, nbuf, 2, v6, nm, f, ml, g))
    assert got[1].tolist() == [2, 1]
    # each batch against the oracle's coalesceMessages for its family
    for b, is6 in enumerate((False, True)):
        bo = [np.concatenate([bufs[j], np.zeros(cap - size, np.uint8)]) for j in range(nbuf)]
        mo = [Msg(np.zeros(1, np.uint8), 64) for _ in range(nbuf)]
        nmo = oracle.coalesce_messages(mo, bo, [size] * nbuf, b"", "ep", is6)
        assert got[1][b] == nmo == (1 if is6 else 2)
        for m in range(nmo):
            f = next(j for j, x in enumerate(bo) if x is mo[m].buf)
            q = b * nbuf + m
            assert (got[2][q], got[3][q]) == (f, mo[m].buf_len)
            assert got[4][q] == (int.from_bytes(mo[m].oob[16:18].tobytes(), "little") if mo[m].oob_len == 24 else -1)
            assert np.array_equal(got[0][b * nbuf + f, :mo[m].buf_len], bo[f][:mo[m].buf_len])
        assert (got[2][b * nbuf + nmo:(b + 1) * nbuf] == 12345).all()
    # the existing entry over the same arena: the bytes it gives for each family are the new entry's for that batch
    for is6 in (0, 1):
        old = run(lambda d, l, n, nm, f, ml, g: dev._check(dev.lib.wgcs_coalesce_messages_batch(
            dev.h, d.data_ptr(), stride, cap, None, l.data_ptr(), n.data_ptr(), nbuf, 2, is6, nm.data_ptr(), f.data_ptr(),
            ml.data_ptr(), g.data_ptr(), None)))
        assert old[1].tolist() == [1, 1] if is6 else old[1].tolist() == [2, 2]
        lo, hi = is6 * nbuf, (is6 + 1) * nbuf
        assert np.array_equal(old[0][lo:hi], got[0][lo:hi])
        for k in (2, 3, 4):
            assert np.array_equal(old[k][lo:hi], got[k][lo:hi])
    with pytest.raises(WgcsError):
        ep.coalesce_dst_batch(dev, torch.zeros(stride, dtype=torch.uint8, device="cuda"), stride, cap, None, v6, v6, 1, 1, None,
                              v6, v6, v6, v6)
