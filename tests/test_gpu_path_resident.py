"""The two chains of tests/test_gpu_path.py with the per-keypair steps on the
device, on the same scenario and against the same CPU
composition (tests/path_ref.py):

  send     wgcs_gso_split_batch -> wgcs_route_dst_batch -> wgcs_send_assign_batch
           -> wgcs_aead_seal_batch -> wgcs_coalesce_messages_batch
           with no host step and no synchronisation before the last launch
  receive  wgcs_split_messages_batch -> wgcs_recv_classify_batch ->
           wgcs_aead_open_batch -> wgcs_replay_batch -> wgcs_recv_source_batch

Every comparison is exact and whole-array.  The receive chain then takes the
same landing buffers once more on the same filters: everything that open
decrypted the first time is now a replay, and no Write call results."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import path_ref
import replay_ref
from path_ref import HDR, MARK, MARK_PEER, MAX_SEGS, N_MSGS, FIRST_MSG_AT
from replay_ref import ERR_PACKET_TOO_SHORT, ERR_REPLAY, NO_KEY
from wireguard_amd import keystate, router, transport
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

PARAMS = [(4096, 4096), (4112, 4099)]  # tests/test_gpu_path.py's
SEED = 20261019


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0]}-{p[1]}")
def ref(request):
    return path_ref.run_reference(SEED, *request.param)


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def i32(n, fill=MARK):
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} differ, first at {bad[0]} (got {got[bad[0]]}, want {want[bad[0]]}), "
                             f"last at {bad[-1]}")


def test_send_chain_without_a_host_step(dev, ref):
    s, want = ref.s, ref.snd
    nj, stride = len(s.jobs), s.stride
    nslots = nj * MAX_SEGS
    peers = sorted(s.key_of_peer)
    peer_keys = router.session_table(peers, [s.key_of_peer[p] for p in peers], 4)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_read, d_jobs, d_image, d_keys = up(s.read_arena), up(s.gso_jobs), up(s.send_router.image), up(s.keys)
        d_peer_keys, d_nonce = up(peer_keys), up(np.array(s.first_counter, np.uint64))
        arena = torch.full((nslots * stride,), path_ref.SEND_SENTINEL, dtype=torch.uint8, device="cuda")
        sizes, count, status, peer = i32(nslots), i32(nj), i32(nj), i32(nslots, MARK_PEER)
        pkts = torch.full((nslots * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        nbufs, job_key, out_len = i32(nj), i32(nj), i32(nslots)
        n_msgs, msg_first, msg_len, msg_gso = i32(nj), i32(nslots), i32(nslots), i32(nslots)
        work = torch.empty(keystate.work_bytes(nj), dtype=torch.uint8, device="cuda")
        stream.synchronize()  # the uploads; from here to the end nothing waits
        dev.gso_split_batch(d_read, d_jobs, nj, arena, stride, HDR, MAX_SEGS, sizes, count, status, stream=stream)
        router.route_dst_batch(dev, arena, sizes, d_image, peer, stride=stride, offset=HDR, stream=stream, n=nslots)
        keystate.send_assign_batch(dev, sizes, peer, count, status, MAX_SEGS, stride, d_peer_keys, d_nonce, pkts, nbufs,
                                   job_key, work, stream=stream, n_jobs=nj, n_slots=len(peer_keys), n_keys=len(s.keys))
        transport.seal_batch(dev, arena, pkts, d_keys, s.mtu, out_len, stream=stream, n=nslots, n_keys=len(s.keys))
        rc = dev.lib.wgcs_coalesce_messages_batch(dev.h, arena.data_ptr(), stride, stride, None, out_len.data_ptr(),
                                                  nbufs.data_ptr(), MAX_SEGS, nj, 0, n_msgs.data_ptr(),
                                                  msg_first.data_ptr(), msg_len.data_ptr(), msg_gso.data_ptr(),
                                                  stream.cuda_stream)
        assert rc == 0
        stream.synchronize()
    same(host(sizes), want.sizes, "gso_split d_sizes")
    same(host(peer, np.uint32), want.peer, "route_dst d_peer")
    # the descriptor table: the host step's rows, then rows that name no key up to the table's end
    n = len(want.seal_pkts)
    table = np.zeros(nslots, AEAD_PKT_DTYPE)
    table["off"], table["key"] = np.arange(nslots, dtype=np.uint64) * np.uint64(stride), NO_KEY
    table[:n] = want.seal_pkts
    got = host(pkts, AEAD_PKT_DTYPE)
    for field in ("off", "counter", "len", "key"):
        same(got[field], table[field], "seal descriptors." + field)
    assert got.tobytes() == table.tobytes()
    same(host(nbufs), want.nbufs, "d_nbufs")
    want_key = np.array([s.key_of_peer[int(want.peer[j * MAX_SEGS])] if want.nbufs[j] else NO_KEY for j in range(nj)],
                        np.uint32)
    same(host(job_key, np.uint32), want_key, "d_job_key")
    used = [sum(int(want.nbufs[j]) for j in range(nj) if want_key[j] == k) for k in range(len(s.keys))]
    same(host(d_nonce, np.uint64), np.array(s.first_counter, np.uint64) + np.array(used, np.uint64), "d_send_nonce")
    assert all(used)
    # seal ran over the whole table: the rows past the host step's last one name no key
    want_len = want.out_len.copy()
    assert (want_len[n:] == MARK).all()
    want_len[n:] = path_ref.ERR_INVALID_ARG
    same(host(out_len), want_len, "seal d_out_len")
    same(host(n_msgs), want.n_msgs, "coalesce d_n_msgs")
    same(host(msg_first), want.msg_first, "coalesce d_msg_first")
    same(host(msg_len), want.msg_len, "coalesce d_msg_len")
    same(host(msg_gso), want.msg_gso, "coalesce d_msg_gso")
    got_arena = host(arena)
    if not np.array_equal(got_arena, want.arena):
        bad = np.flatnonzero(got_arena != want.arena)
        raise AssertionError(f"send arena: {len(bad)} bytes differ, first in slot {bad[0] // stride}")


def recv_pass(dev, s, stream, land, n_in, gso, d, filters):
    """split -> classify -> open -> replay -> source, back to back on `stream`."""
    stride, nb = s.stride, n_in.numel() // N_MSGS
    n = nb * N_MSGS
    r = SimpleNamespace()
    r.arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
    r.n_out, r.src, r.count, r.split_status = i32(n), i32(n), i32(nb), i32(nb)
    r.pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    r.type, r.pkt_len, r.verdict, r.found = i32(n), i32(n), i32(n), i32(n, MARK_PEER)
    r.counter = torch.full((n * 8,), path_ref.MARK_CTR & 0xFF, dtype=torch.uint8, device="cuda")
    rc = dev.lib.wgcs_split_messages_batch(dev.h, land.data_ptr(), s.in_stride, s.buf_len, n_in.data_ptr(),
                                           gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, r.arena.data_ptr(), stride,
                                           r.n_out.data_ptr(), r.src.data_ptr(), r.count.data_ptr(),
                                           r.split_status.data_ptr(), stream.cuda_stream)
    assert rc == 0
    router.classify_batch(dev, r.arena, r.n_out, d.slots, r.pkts, r.type, stride=stride, stream=stream, n=n,
                          n_slots=len(s.slots))
    transport.open_batch(dev, r.arena, r.pkts, d.keys, r.pkt_len, r.counter, stream=stream, n=n, n_keys=len(s.keys))
    keystate.replay_batch(dev, r.pkts, r.pkt_len, r.counter, filters, r.verdict, d.work, stream=stream, n=n,
                          n_keys=len(s.keys))
    # d_verdict aliases d_pkt_len from here on
    router.source_batch(dev, r.arena, r.pkts, r.verdict, d.key_peer, d.image, r.verdict, peer=r.found, stream=stream,
                        n=n, n_keys=len(s.key_peer))
    return r


def test_receive_chain_with_the_replay_filter(dev, ref):
    s, want = ref.s, ref.rcv
    n = len(ref.n_in)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        land, n_in, gso = up(ref.land), torch.from_numpy(ref.n_in).cuda(), torch.from_numpy(ref.gso).cuda()
        d = SimpleNamespace(slots=up(s.slots), keys=up(s.keys), image=up(s.recv_router.image),
                            key_peer=up(np.array(s.key_peer, np.uint32)),
                            work=torch.empty(keystate.work_bytes(n), dtype=torch.uint8, device="cuda"))
        filters = up(np.zeros(len(s.keys), REPLAY_FILTER_DTYPE))
        first = recv_pass(dev, s, stream, land, n_in, gso, d, filters)
        stream.synchronize()
        filters_1 = host(filters, REPLAY_FILTER_DTYPE).copy()
        second = recv_pass(dev, s, stream, land, n_in, gso, d, filters)
        stream.synchronize()
    # first pass: all counters are distinct, so the filter drops nothing and the chain is recv_ref's
    same(host(first.pkts, AEAD_PKT_DTYPE), want.pkts, "classify d_pkts")
    same(host(first.counter, np.uint64), want.counter, "open d_counter")
    same(host(first.pkt_len), want.pkt_len, "open d_pkt_len")
    same(host(first.verdict), want.verdict, "source d_verdict")
    same(host(first.found, np.uint32), want.found, "source d_peer")
    assert np.array_equal(host(first.arena), want.arena_opened), "receive arena"
    replayed, want_filters = replay_ref.replay_batch_ref(want.pkts, want.pkt_len, want.counter,
                                                         np.zeros(len(s.keys), REPLAY_FILTER_DTYPE))
    same(replayed, want.pkt_len, "the reference filter drops nothing either")
    assert filters_1.tobytes() == want_filters.tobytes()
    # second pass: everything open decrypted is a replay now, every other verdict is as before
    took = (want.pkts["key"] < len(s.keys)) & ((want.pkt_len >= 0) | (want.pkt_len == ERR_PACKET_TOO_SHORT))
    assert took.any() and {int(k) for k in want.pkts["key"][took]} == {0, 1}
    want_2 = np.where(took, ERR_REPLAY, want.verdict).astype(np.int32)
    same(host(second.pkt_len), want.pkt_len, "open d_pkt_len, second pass")
    same(host(second.verdict), want_2, "source d_verdict, second pass")
    assert np.array_equal(host(second.arena), want.arena_opened), "receive arena, second pass"
    _, want_filters_2 = replay_ref.replay_batch_ref(want.pkts, want.pkt_len, want.counter, want_filters)
    assert host(filters, REPLAY_FILTER_DTYPE).tobytes() == want_filters_2.tobytes() == want_filters.tobytes()
    bufs, calls = path_ref.host_write_step(s, want_2, want.n_batches)
    assert len(calls) == 0 and len(bufs) == 0 and (want.verdict > 0).any()
    same(host(land), ref.land, "the landing buffers are only read")
