"""The receive chain of tests/test_gpu_path_resident.py carried through to
toWrite with no host step:

  wgcs_split_messages_batch -> wgcs_recv_classify_batch -> wgcs_aead_open_batch
  -> wgcs_replay_batch -> wgcs_recv_source_batch -> wgcs_write_build_batch ->
  wgcs_handle_gro_batch

twice over the same landing buffers and filters, all on one stream with a
single synchronisation at the end.  The first pass must give the arena, the
Write calls' results and the loopback property of tests/path_ref.py and the
accounting rows of tests/write_ref.py; in the second everything open decrypted
is a replay, so no peer validates anything and no call writes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import path_ref
import write_ref
from path_ref import HDR, MARK_TW, N_MSGS
from test_gpu_path_resident import PARAMS, SEED, host, i32, recv_pass, same, up
from wireguard_amd import keystate, writeplan
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

pytestmark = pytest.mark.gpu

CPB = 2  # the scenario has two peers


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0]}-{p[1]}")
def ref(request):
    return path_ref.run_reference(SEED, *request.param)


def write_pass(dev, s, stream, r, key_peer):
    """builder -> handle_gro over every call row, behind recv_pass on `stream`."""
    nb = r.verdict.numel() // N_MSGS
    nc = nb * CPB
    w = SimpleNamespace(nc=nc)
    for name, rows, dt in (("bufs", nb * N_MSGS, GRO_BUF_DTYPE), ("calls", nc, GRO_CALL_DTYPE),
                           ("groups", nc, WRITE_GROUP_DTYPE)):
        setattr(w, name, torch.full((rows * dt.itemsize,), 0xC7, dtype=torch.uint8, device="cuda"))
    w.n_groups, w.status, w.gro_status, w.n_write = i32(nb), i32(nb), i32(nc), i32(nc)
    w.to_write = i32(nb * N_MSGS, MARK_TW)
    writeplan.write_build_batch(dev, r.pkts, r.verdict, N_MSGS, key_peer, HDR, s.stride, CPB, w.bufs, w.calls, w.groups,
                                w.n_groups, w.status, stream=stream, n_batches=nb, n_keys=len(s.key_peer))
    dev.handle_gro_batch(r.arena, w.bufs, w.calls, nc, w.gro_status, w.n_write, w.to_write, stream=stream)
    return w


def test_receive_chain_to_to_write_without_a_host_step(dev, ref):
    s, want = ref.s, ref.rcv
    n, nb = len(ref.n_in), want.n_batches
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        land, n_in, gso = up(ref.land), torch.from_numpy(ref.n_in).cuda(), torch.from_numpy(ref.gso).cuda()
        d = SimpleNamespace(slots=up(s.slots), keys=up(s.keys), image=up(s.recv_router.image),
                            key_peer=up(np.array(s.key_peer, np.uint32)),
                            work=torch.empty(keystate.work_bytes(n), dtype=torch.uint8, device="cuda"))
        filters = up(np.zeros(len(s.keys), REPLAY_FILTER_DTYPE))
        stream.synchronize()  # the uploads; from here to the end nothing waits
        first = recv_pass(dev, s, stream, land, n_in, gso, d, filters)
        w1 = write_pass(dev, s, stream, first, d.key_peer)
        second = recv_pass(dev, s, stream, land, n_in, gso, d, filters)
        w2 = write_pass(dev, s, stream, second, d.key_peer)
        stream.synchronize()

    # ---- first pass
    same(host(first.verdict), want.verdict, "source d_verdict")
    plan = write_ref.write_ref(want.pkts, want.verdict, N_MSGS, np.array(s.key_peer, np.uint32), HDR, s.stride, CPB)
    gro = write_ref.gro_ref(want.arena_opened, plan)
    assert (plan.status == 0).all() and (plan.n_groups > 0).sum() >= 4
    same(host(w1.status), plan.status, "builder d_status")
    same(host(w1.n_groups), plan.n_groups, "builder d_n_groups")
    assert host(w1.calls, GRO_CALL_DTYPE).tobytes() == plan.calls.tobytes(), "builder d_calls"
    assert host(w1.groups, WRITE_GROUP_DTYPE).tobytes() == plan.groups.tobytes(), "builder d_groups"
    got_arena = host(first.arena)
    assert np.array_equal(got_arena, want.arena), "receive arena after GRO"
    assert np.array_equal(gro.arena, want.arena), "one call per peer writes what one call per batch wrote"
    calls, bufs = host(w1.calls, GRO_CALL_DTYPE), host(w1.bufs, GRO_BUF_DTYPE)
    st, nw, tw = host(w1.gro_status), host(w1.n_write), host(w1.to_write)
    same(st, gro.status, "GRO d_status")
    same(nw, gro.n_write, "GRO d_n_write")
    same(tw, gro.to_write, "GRO d_to_write")
    assert bufs.tobytes() == gro.bufs.tobytes(), "slice headers after GRO"
    # each non-empty call is the corresponding Write call of the reference chain
    rows = np.flatnonzero(calls["n"] > 0)
    assert len(rows) == len(want.gro_calls)
    for c, row in enumerate(rows):
        a, r0 = int(calls["first"][row]), int(want.gro_calls["first"][c])
        k = int(want.gro_calls["n"][c])
        assert calls["n"][row] == k and st[row] == want.gro_status[c] and nw[row] == want.n_write[c], c
        assert np.array_equal(tw[a:a + nw[row]], want.to_write[r0:r0 + nw[row]]), c
        assert bufs[a:a + k].tobytes() == want.gro_bufs[r0:r0 + k].tobytes(), c
    dev_rcv = SimpleNamespace(gro_calls=calls, n_write=nw, to_write=tw, gro_bufs=bufs)
    assert path_ref.check_loopback(s, dev_rcv, got_arena) == 5
    empty = np.flatnonzero(calls["n"] == 0)
    assert (st[empty] == 0).all() and (nw[empty] == 0).all()

    # ---- second pass: every peer's filter has seen it all
    assert (want.verdict > 0).any()
    same(host(w2.n_groups), np.zeros(nb, np.int32), "d_n_groups, second pass")
    same(host(w2.status), np.zeros(nb, np.int32), "builder d_status, second pass")
    calls2 = host(w2.calls, GRO_CALL_DTYPE)
    assert (calls2["n"] == 0).all() and np.array_equal(calls2["first"], np.repeat(np.arange(nb) * N_MSGS, CPB))
    assert (host(w2.groups, WRITE_GROUP_DTYPE)["peer"] == write_ref.PEER_NONE).all()
    same(host(w2.gro_status), np.zeros(nb * CPB, np.int32), "GRO d_status, second pass")
    same(host(w2.n_write), np.zeros(nb * CPB, np.int32), "GRO d_n_write, second pass")
    assert (host(w2.to_write) == MARK_TW).all() and not host(w2.bufs).any()
    assert np.array_equal(host(second.arena), want.arena_opened), "receive arena, second pass"
    same(host(land), ref.land, "the landing buffers are only read")
