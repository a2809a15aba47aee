"""The two device-resident chains of INTEGRATION.md §2g / §2h end to end on
the GPU, each kernel reading what the one before it wrote, against the chain
composed on the CPU (tests/path_ref.py, pinned by tests/test_path_ref.py).

  send     wgcs_gso_split_batch -> wgcs_route_dst_batch -> host step ->
           wgcs_aead_seal_batch -> wgcs_coalesce_messages_batch
  receive  wgcs_split_messages_batch -> wgcs_recv_classify_batch ->
           wgcs_aead_open_batch -> wgcs_recv_source_batch -> host step ->
           wgcs_handle_gro_batch

Every comparison is exact and covers the whole arena and the whole of every
output array: arenas start as a sentinel and output arrays as a marker, so a
stage that writes a byte or a row it must not shows.  The launches of a chain
go on one non-default stream; device arrays are handed from kernel to kernel
as INTEGRATION hands them, and the host reads only what the two documented
host steps read (path_ref.host_seal_step, path_ref.host_write_step)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import path_ref
from path_ref import HDR, MARK, MARK_PEER, MARK_TW, MAX_SEGS, N_MSGS, FIRST_MSG_AT
from wireguard_amd import router, transport
from wireguard_amd.transport import AEAD_PKT_DTYPE
from wireguard_amd.tun import GRO_BUF_DTYPE

pytestmark = pytest.mark.gpu

PARAMS = [(4096, 4096), (4112, 4099)]  # (slot stride, landing stride): on 128-byte lines, and off them
SEED = 20261019  # tests/test_path_ref.py checks the scenario at these


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: f"{p[0]}-{p[1]}")
def ref(request):
    return path_ref.run_reference(SEED, *request.param)


class TorchOps:
    """path_ref.wire() on device tensors."""
    _T = {np.uint8: torch.uint8, np.int32: torch.int32}

    @staticmethod
    def full(n, value, dtype):
        return torch.full((n,), value, dtype=TorchOps._T[dtype], device="cuda")

    @staticmethod
    def const(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    where = staticmethod(torch.where)


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


def same_arena(got, want, stride, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        q, x = divmod(int(bad[0]), stride)
        raise AssertionError(f"{what}: {len(bad)} bytes differ in {len(np.unique(bad // stride))} slots, first in slot "
                             f"{q} at byte {x}: got {got[bad[0]:bad[0] + 8].tobytes().hex()} want "
                             f"{want[bad[0]:bad[0] + 8].tobytes().hex()}")


# ------------------------------------------------------------------------ send
def run_send(dev, s, stream, want, snaps=None):
    """The four send launches on `stream` with the documented host step in
    between.  `want` (path_ref.send_ref's result) is what the host step's
    inputs are checked against before descriptors are built from them; the
    caller compares the rest.  `snaps` collects device copies of the arena."""
    nj, stride = len(s.jobs), s.stride
    nslots = nj * MAX_SEGS

    def snap(name):
        if snaps is not None:
            snaps[name] = d.arena.clone()

    d = SimpleNamespace()
    d.read, d.jobs, d.image, d.keys = up(s.read_arena), up(s.gso_jobs), up(s.send_router.image), up(s.keys)
    d.arena = torch.full((nslots * stride,), path_ref.SEND_SENTINEL, dtype=torch.uint8, device="cuda")
    d.sizes, d.count, d.status, d.peer = i32(nslots), i32(nj), i32(nj), i32(nslots, MARK_PEER)
    dev.gso_split_batch(d.read, d.jobs, nj, d.arena, stride, HDR, MAX_SEGS, d.sizes, d.count, d.status, stream=stream)
    snap("split")
    router.route_dst_batch(dev, d.arena, d.sizes, d.image, d.peer, stride=stride, offset=HDR, stream=stream, n=nslots)
    snap("route")
    stream.synchronize()
    # the host step: sizes, counts, statuses and peers come back, descriptors and d_nbufs go up
    sizes, count, status, peer = host(d.sizes), host(d.count), host(d.status), host(d.peer, np.uint32)
    same(sizes, want.sizes, "gso_split d_sizes")
    same(count, want.count, "gso_split d_count")
    same(status, want.status, "gso_split d_status")
    same(peer, want.peer, "route_dst d_peer")
    pk, nbufs = path_ref.host_seal_step(s, sizes, count, status, peer)
    d.h_seal_pkts, d.h_nbufs = pk, nbufs
    d.seal_pkts, d.nbufs = up(pk), torch.from_numpy(nbufs).cuda()
    snap("upload")
    d.out_len = i32(nslots)
    transport.seal_batch(dev, d.arena, d.seal_pkts, d.keys, s.mtu, d.out_len, stream=stream, n=len(pk),
                         n_keys=len(s.keys))
    snap("seal")
    # the same arena as d_bufs, seal's d_out_len as d_lens; cap = stride
    d.n_msgs, d.msg_first, d.msg_len, d.msg_gso = i32(nj), i32(nslots), i32(nslots), i32(nslots)
    rc = dev.lib.wgcs_coalesce_messages_batch(dev.h, d.arena.data_ptr(), stride, stride, None, d.out_len.data_ptr(),
                                              d.nbufs.data_ptr(), MAX_SEGS, nj, 0, d.n_msgs.data_ptr(),
                                              d.msg_first.data_ptr(), d.msg_len.data_ptr(), d.msg_gso.data_ptr(),
                                              stream.cuda_stream)
    assert rc == 0
    return d


def check_send(s, d, want):
    same(d.h_seal_pkts, want.seal_pkts, "seal descriptors")
    same(d.h_nbufs, want.nbufs, "d_nbufs")
    same(host(d.out_len), want.out_len, "seal d_out_len")
    same(host(d.n_msgs), want.n_msgs, "coalesce d_n_msgs")
    same(host(d.msg_first), want.msg_first, "coalesce d_msg_first")
    same(host(d.msg_len), want.msg_len, "coalesce d_msg_len")
    same(host(d.msg_gso), want.msg_gso, "coalesce d_msg_gso")
    same_arena(host(d.arena), want.arena, s.stride, "send arena")


def test_send_chain(dev, ref):
    s, want = ref.s, ref.snd
    stream = torch.cuda.Stream()
    snaps = {}
    with torch.cuda.stream(stream):
        d = run_send(dev, s, stream, want, snaps)
        stream.synchronize()
    same_arena(host(snaps["split"]), want.arena_split, s.stride, "arena after gso_split")
    assert torch.equal(snaps["route"], snaps["split"]), "route_dst wrote the arena"
    assert torch.equal(snaps["upload"], snaps["split"]), "the descriptor upload changed the arena"
    same(host(d.out_len), want.out_len, "seal d_out_len")
    same_arena(host(snaps["seal"]), want.arena_sealed, s.stride, "arena after seal")
    check_send(s, d, want)
    assert (want.arena != want.arena_sealed).any() and (want.arena_sealed != want.arena_split).any()


# --------------------------------------------------------------------- receive
def run_recv(dev, s, stream, land, n_in, gso, want):
    """The receive chain on `stream` from landing buffers on the device: four
    launches back to back, one synchronisation, the documented host step, GRO."""
    stride, nb = s.stride, n_in.numel() // N_MSGS
    n = nb * N_MSGS
    d = SimpleNamespace(n_batches=nb)
    d.slots, d.keys, d.image = up(s.slots), up(s.keys), up(s.recv_router.image)
    d.key_peer = up(np.array(s.key_peer, np.uint32))
    d.arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
    d.n_out, d.src, d.count, d.split_status = i32(n), i32(n), i32(nb), i32(nb)
    d.pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    d.type, d.verdict, d.found = i32(n), i32(n), i32(n, MARK_PEER)
    d.counter = torch.full((n * 8,), path_ref.MARK_CTR & 0xFF, dtype=torch.uint8, device="cuda")
    rc = dev.lib.wgcs_split_messages_batch(dev.h, land.data_ptr(), s.in_stride, s.buf_len, n_in.data_ptr(),
                                           gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, d.arena.data_ptr(), stride,
                                           d.n_out.data_ptr(), d.src.data_ptr(), d.count.data_ptr(),
                                           d.split_status.data_ptr(), stream.cuda_stream)
    assert rc == 0
    router.classify_batch(dev, d.arena, d.n_out, d.slots, d.pkts, d.type, stride=stride, stream=stream, n=n,
                          n_slots=len(s.slots))
    transport.open_batch(dev, d.arena, d.pkts, d.keys, d.verdict, d.counter, stream=stream, n=n, n_keys=len(s.keys))
    # d_verdict aliases d_pkt_len
    router.source_batch(dev, d.arena, d.pkts, d.verdict, d.key_peer, d.image, d.verdict, peer=d.found, stream=stream,
                        n=n, n_keys=len(s.key_peer))
    stream.synchronize()
    # the host step: the verdicts come back, one Write call per batch goes up
    verdict = host(d.verdict)
    same(verdict, want.verdict, "recv_source d_verdict")
    bufs, calls = path_ref.host_write_step(s, verdict, nb)
    d.gro_bufs_in, d.gro_calls_h = bufs, calls
    d.gro_bufs, d.gro_calls = up(bufs), up(calls)
    nc = len(calls)
    d.gro_status, d.n_write, d.to_write = i32(nc), i32(nc), i32(len(bufs), MARK_TW)
    dev.handle_gro_batch(d.arena, d.gro_bufs, d.gro_calls, nc, d.gro_status, d.n_write, d.to_write, stream=stream)
    return d


def check_recv(s, d, want):
    same(host(d.count), want.count, "split d_count")
    same(host(d.split_status), want.split_status, "split d_status")
    same(host(d.n_out), want.n_out, "split d_n_out")
    same(host(d.src), want.src, "split d_src")
    same(host(d.type), want.type, "classify d_type")
    same(host(d.pkts, AEAD_PKT_DTYPE), want.pkts, "classify d_pkts")
    same(host(d.counter, np.uint64), want.counter, "open d_counter")
    same(host(d.verdict), want.verdict, "source d_verdict")
    same(host(d.found, np.uint32), want.found, "source d_peer")
    same(d.gro_bufs_in, want.gro_bufs_in, "Write calls' buffers")
    same(d.gro_calls_h, want.gro_calls, "Write calls")
    same(host(d.gro_status), want.gro_status, "handle_gro d_status")
    same(host(d.n_write), want.n_write, "handle_gro d_n_write")
    same(host(d.to_write), want.to_write, "handle_gro d_to_write")
    same(host(d.gro_bufs, GRO_BUF_DTYPE), want.gro_bufs, "handle_gro slice headers")
    same_arena(host(d.arena), want.arena, s.stride, "receive arena")


def test_receive_chain(dev, ref):
    """From the reference's wire messages: independent of the send kernels."""
    s, want = ref.s, ref.rcv
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        land, n_in, gso = up(ref.land), torch.from_numpy(ref.n_in).cuda(), torch.from_numpy(ref.gso).cuda()
        d = run_recv(dev, s, stream, land, n_in, gso, want)
        stream.synchronize()
    check_recv(s, d, want)
    same(host(land), ref.land, "the landing buffers are only read")
    assert (want.arena != want.arena_opened).any() and (want.arena_opened != want.arena_split).any()


def test_loopback(dev, ref):
    """send chain -> wire() on the device -> receive chain: the bytes that come
    out of GRO are the reference's, and so they are the bytes that went in."""
    s = ref.s
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        snd = run_send(dev, s, stream, ref.snd)
        land, n_in, gso = path_ref.wire(s, ref.plan, snd.arena, snd.msg_len, snd.msg_gso, ops=TorchOps)
        rcv = run_recv(dev, s, stream, land, n_in, gso, ref.rcv)
        stream.synchronize()
    same(host(land), ref.land, "landing buffers")
    same(host(n_in), ref.n_in, "d_n_in")
    same(host(gso), ref.gso, "d_gso")
    check_send(s, snd, ref.snd)
    check_recv(s, rcv, ref.rcv)
    # the loopback property on the device's own bytes and tables
    arena = host(rcv.arena)
    got = SimpleNamespace(gro_calls=rcv.gro_calls_h, n_write=host(rcv.n_write), to_write=host(rcv.to_write),
                          gro_bufs=host(rcv.gro_bufs, GRO_BUF_DTYPE))
    assert path_ref.check_loopback(s, got, arena) == len(s.loopback_jobs) == 5
