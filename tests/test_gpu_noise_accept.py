"""The device-resident handshake accept on the GPU (wgcs_handshake_accept_batch,
the four kernels of noise_accept_kernels.hip) against the host form
wgcs_handshake_accept_host, byte for byte: verdicts, the whole peer table, the
whole descriptor array and the count.  tests/test_noise_accept_ref.py pins the
host form to the sequential restatement of device/noise.go:458-491.

Verdict, descriptor and count buffers are filled with a sentinel first and are
longer than the call's rows; d_init, d_gate, d_table, d_peer_rows and d_tickets
are compared with their uploads afterwards.  The chain test runs split ->
classify -> screen -> consume -> accept -> respond -> seal on one stream with
no synchronisation and lets the restatement's initiator finish the handshakes."""
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import aead_ref
import cookie_ref
import noise_accept_cases as cases
import noise_ref
import noise_resp_ref
from noise_accept_cases import CLAIM_NONE, NOW, T
from noise_accept_ref import ERR_BATCH_FULL, ERR_FLOOD, ERR_REPLAY, HS_ACCEPTED, HS_CONSUMED
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_NO_PEER, HS_NONE
from noise_resp_ref import HS_RESPONDED
from test_gpu_cookie import SENTINEL, flip, up
from wireguard_amd import _lib, cookie, noise, router, transport
from wireguard_amd.noise import HS_INIT_DTYPE, HS_PEER_DTYPE, HS_RESP_DTYPE, HS_TICKET_DTYPE, PEER_KEY_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

SPARE = 3  # rows of d_verdict, d_resp and d_count past the call's: they keep their fill
VERDICT_FILL, COUNT_FILL = 12345, 0x5A5A5A5A
PITCH = 96


def some(a, dtype):
    """a on the device, or one placeholder row where it is empty (a pointer is still passed)."""
    return up(a) if len(a) else up(np.zeros(1, dtype))


def host_step(c, s, peers):
    p = peers.copy()
    verdict = np.full(len(s.init) + SPARE, VERDICT_FILL, np.int32)
    resp = np.full(80 * (len(s.tickets) + SPARE), SENTINEL, np.uint8).view(HS_RESP_DTYPE)
    count = np.full(1 + SPARE, COUNT_FILL, np.uint32)
    noise.accept_host(s.init, s.gate, s.now, c.table, c.peer_rows, p, s.tickets, resp, count, verdict)
    return verdict, p, resp, count


def device_step(dev, c, s, peers, stream=None):
    """(verdict, peers, resp, count) whole, fills included, after the inputs were compared with their uploads."""
    n, nt = len(s.init), len(s.tickets)
    ins = dict(init=(s.init, HS_INIT_DTYPE), gate=(s.gate, np.int32), table=(c.table, PEER_KEY_DTYPE),
               peer_rows=(c.peer_rows, np.uint32), tickets=(s.tickets, HS_TICKET_DTYPE))
    d = {k: some(a, t) for k, (a, t) in ins.items()}
    d_peers = up(peers)
    d_verdict = torch.full((n + SPARE,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    d_resp = torch.full((80 * (nt + SPARE),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_count = torch.from_numpy(np.full(1 + SPARE, COUNT_FILL, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    noise.accept_batch(dev, d["init"], d["gate"], s.now, d["table"], d["peer_rows"], d_peers, d["tickets"], d_resp,
                       d_count, d_verdict, stream=stream, n=n, n_ids=c.n_ids, n_peers=len(c.table), n_tickets=nt)
    torch.cuda.synchronize()
    for k, (a, _) in ins.items():
        if len(a):
            assert d[k].cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), f"{k} was written"
    return (d_verdict.cpu().numpy(), d_peers.cpu().numpy().view(HS_PEER_DTYPE), d_resp.cpu().numpy().view(HS_RESP_DTYPE),
            d_count.cpu().numpy().view(np.uint32))


def check_case(dev, c):
    peers, out = c.peers, []
    for k, s in enumerate(c.steps):
        want = host_step(c, s, peers)
        got = device_step(dev, c, s, peers)
        where = f"{c.name} step {k}"
        bad = np.flatnonzero(got[0] != want[0])
        assert len(bad) == 0, f"{where}: verdict row {bad[0]}: got {got[0][bad[0]]}, want {want[0][bad[0]]}"
        assert got[3].tolist() == want[3].tolist(), where
        assert got[2].tobytes() == want[2].tobytes(), where
        assert got[1].tobytes() == want[1].tobytes(), where
        assert (got[1]["claim"] == CLAIM_NONE).all(), where
        peers = got[1]
        out.append(got)
    return out


NAMED = {c.name: c for c in cases.named()}  # n == 1, n == 0, fewer tickets than winners and none among them


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case_matches_the_host_form(dev, name):
    check_case(dev, NAMED[name])


def test_rows_of_one_peer_in_different_waves_and_blocks(dev):
    c = cases.wide()
    (verdict, peers, resp, count), = check_case(dev, c)
    assert [verdict[q] for q in (3, 70, 290)] == [ERR_REPLAY, HS_ACCEPTED, ERR_FLOOD]
    assert count[0] >= 3 and 70 in resp["init_row"][:count[0]].tolist()
    assert {ERR_NO_PEER, ERR_REPLAY, ERR_FLOOD, HS_ACCEPTED} <= set(verdict[:300].tolist())
    # the same batch again on fresh tables: the same bytes, whichever wave ran first
    again = device_step(dev, c, c.steps[0], c.peers)
    for a, b in zip((verdict, peers, resp, count), again):
        assert a.tobytes() == b.tobytes()


def test_fewer_tickets_than_winners_in_a_wide_batch(dev):
    c = cases.wide()
    s = SimpleNamespace(**vars(c.steps[0]))
    s.tickets = s.tickets[:2]
    c2 = SimpleNamespace(**{**vars(c), "name": "wide_2_tickets", "steps": [s]})
    (verdict, peers, resp, count), = check_case(dev, c2)
    assert count[0] == 2 and (verdict[:300] == ERR_BATCH_FULL).sum() >= 1


def test_more_blocks_than_one_turn_of_the_scan(dev):
    """1,024 * 256 + 300 rows: the scan kernel takes a second turn over the block counts, and a
    winner's rank sums counts of both turns.  It is the one scan kernel (compact_kernels.hip) that
    wgcs_rekey_start_batch and wgcs_timers_expire_batch launch too, so this covers their second turn."""
    n, n_peers = 1024 * 256 + 300, 3000
    rng = np.random.default_rng(262)
    table, rows, n_ids = cases.table_of(n_peers, seed=262)
    peers = cases.peers_of(n_peers, seed=263)
    init = np.zeros(n, HS_INIT_DTYPE)
    init["peer"] = table["peer"][rng.integers(0, n_peers, n)]
    init["peer"][rng.integers(0, n, 50)] = n_ids + 5
    init["sender"] = rng.integers(0, 2**32, n, dtype=np.uint32)
    pool = np.frombuffer(b"".join(T), np.uint8).reshape(4, 12)
    init["timestamp"] = pool[rng.integers(0, 4, n)]
    # winners thin out towards the end but for one peer that shows up only in the last block
    late = 7
    init["peer"][init["peer"] == table["peer"][late]] = table["peer"][late + 1]
    init["peer"][n - 5] = table["peer"][late]
    gate = np.where(rng.random(n) < 0.9, HS_CONSUMED, HS_NONE).astype(np.int32)
    gate[n - 5] = HS_CONSUMED
    c = SimpleNamespace(name="big", table=table, peer_rows=rows, n_ids=n_ids, peers=peers,
                        steps=[SimpleNamespace(init=init, gate=gate, now=NOW, tickets=cases.tickets_of(n_peers + 5, 264))])
    (verdict, p, resp, count), = check_case(dev, c)
    assert verdict[n - 5] == HS_ACCEPTED and resp["init_row"][count[0] - 1] == n - 5
    assert count[0] > 2000 and (np.diff(resp["init_row"][:count[0]].astype(np.int64)) > 0).all()


def test_accept_batch_arguments(dev):
    c = NAMED["three_rising"]
    s = c.steps[0]
    n, nt = len(s.init), len(s.tickets)
    d_init, d_gate, d_table, d_rows, d_peers, d_tickets = (up(s.init), up(s.gate), up(c.table), up(c.peer_rows), up(c.peers),
                                                           up(s.tickets))
    d_verdict = torch.full((n,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    d_resp = torch.full((80 * nt,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_count = torch.full((1,), VERDICT_FILL, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(init=d_init, gate=d_gate, now_ns=s.now, table=d_table, peer_rows=d_rows, peers=d_peers, tickets=d_tickets,
                 resp=d_resp, count=d_count, verdict=d_verdict, n=n, n_ids=c.n_ids, n_peers=len(c.table), n_tickets=nt)
        a.update(kw)
        noise.accept_batch(dev, **a)

    bad = [dict(init=None), dict(gate=None), dict(table=None), dict(peer_rows=None), dict(peers=None), dict(tickets=None),
           dict(resp=None), dict(count=None), dict(verdict=None), dict(verdict=d_gate), dict(n=(1 << 28) + 1),
           dict(n_tickets=(1 << 28) + 1), dict(init=d_init.data_ptr() + 2), dict(gate=d_gate.data_ptr() + 1),
           dict(table=d_table.data_ptr() + 2), dict(peer_rows=d_rows.data_ptr() + 2), dict(peers=d_peers.data_ptr() + 1),
           dict(tickets=d_tickets.data_ptr() + 2), dict(resp=d_resp.data_ptr() + 1), dict(count=d_count.data_ptr() + 2),
           dict(verdict=d_verdict.data_ptr() + 2), dict(n=0, n_tickets=0, count=None)]
    for kw in bad:
        with pytest.raises(_lib.WgcsError) as ei:
            call(**kw)
        assert ei.value.code == ERR_INVALID_ARG, kw
    assert dev.lib.wgcs_handshake_accept_batch(None, d_init.data_ptr(), d_gate.data_ptr(), n, s.now, d_table.data_ptr(),
                                               d_rows.data_ptr(), c.n_ids, d_peers.data_ptr(), len(c.table),
                                               d_tickets.data_ptr(), nt, d_resp.data_ptr(), d_count.data_ptr(),
                                               d_verdict.data_ptr(), None) == ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (d_verdict.cpu().numpy() == VERDICT_FILL).all() and (d_resp.cpu().numpy() == SENTINEL).all()
    assert d_count.item() == VERDICT_FILL and d_peers.cpu().numpy().tobytes() == c.peers.tobytes()
    # n == 0 and no tickets: only the count is written, and no other pointer is needed
    call(n=0, n_tickets=0, init=None, gate=None, table=None, peer_rows=None, peers=None, tickets=None, resp=None,
         verdict=None, n_ids=0, n_peers=0)
    torch.cuda.synchronize()
    assert d_count.item() == 0 and (d_resp.cpu().numpy() == SENTINEL).all()
    # without a table every consumed row has no peer
    call(n_peers=0, table=None, peers=None)
    torch.cuda.synchronize()
    assert (d_verdict.cpu().numpy() == ERR_NO_PEER).all() and d_count.item() == 0
    assert (d_resp.cpu().numpy().view(HS_RESP_DTYPE)["init_row"] == 0xFFFFFFFF).all()


# ----------------------------------------------------------------------- chain
def test_one_stream_chain_from_split_through_accept_to_the_first_sealed_packet(dev):
    """wgcs_split_messages_batch -> wgcs_recv_classify_batch -> wgcs_handshake_screen_batch ->
    wgcs_handshake_consume_batch -> wgcs_handshake_accept_batch -> wgcs_handshake_respond_batch
    (over n_tickets descriptors, NULL gate) -> wgcs_aead_seal_batch under the send-key rows just
    written, all enqueued on one stream with no synchronisation between them.  One initiation's
    timestamp is its peer's stored lastTimestamp, and one peer's initiation is in the batch
    twice: neither the replay nor the copy gets a response.  The restatement's initiator then
    consumes each response and opens the sealed packet with its receive key."""
    import path_ref
    from path_ref import FIRST_MSG_AT, MARK, N_MSGS

    rng = np.random.default_rng(458)
    private = rng.bytes(32)
    responder, public = noise.responder_init(private)
    checker = cookie_ref.Checker(public)
    names = ["a", "b", "old", "d"]
    ini = {k: SimpleNamespace(private=rng.bytes(32), eph=rng.bytes(32), index=int(rng.integers(0, 2**32)),
                              ts=T[1 + i % 3], psk=rng.bytes(32) if k in ("a", "old") else bytes(32))
           for i, k in enumerate(names)}
    stranger = rng.bytes(32)
    for k, p in ini.items():
        p.public = noise_ref.public_key(p.private)
        p.msg, p.hash, p.chain = noise.create_initiation(p.private, public, p.eph, p.ts, p.index)
        p.msg = cookie_ref.add_macs(checker.mac1_key, p.msg)[0]
    others = [noise_ref.public_key(rng.bytes(32)) for _ in range(5)]
    n_ids = 60
    table = noise.peer_keys_build(responder, [ini[k].public for k in names] + others, list(range(50, 50 + len(names) + 5)))
    n_peers = len(table)
    peer_rows = noise.peer_rows_build(table, n_ids)
    psk = np.zeros((n_peers, 32), np.uint8)
    peers = cases.peers_of(n_peers, seed=459)
    peers["flags"] = 0
    for p in ini.values():
        p.peer_row = noise.peer_keys_find(table, p.public)
        psk[p.peer_row] = np.frombuffer(p.psk, np.uint8)
    cases.seen(peers, ini["old"].peer_row, ini["old"].ts, NOW - 10**9)   # this very timestamp was consumed a second ago
    cases.seen(peers, ini["a"].peer_row, T[0], NOW - 10**9)              # an older one: a's is accepted
    peers["flags"][ini["b"].peer_row] |= noise.HS_PEER_COOKIE            # b's response carries MAC2
    bad_ts = cookie_ref.add_macs(checker.mac1_key, flip(ini["a"].msg, 100))[0]
    unknown = cookie_ref.add_macs(checker.mac1_key, noise.create_initiation(stranger, public, rng.bytes(32), rng.bytes(12), 5)[0])[0]

    s = path_ref.scenario(20261020, 4112, 4099)
    nb, stride, per = 2, s.stride, N_MSGS - FIRST_MSG_AT
    pitch, n = per * s.in_stride, 2 * N_MSGS
    land = np.full(nb * pitch, path_ref.LAND_SENTINEL, np.uint8)
    n_in, gso = np.zeros(n, np.int32), np.zeros(n, np.int32)
    batches = [([ini["a"].msg + ini["b"].msg + bad_ts + ini["old"].msg + unknown + ini["b"].msg,
                 cookie_ref.handshake_message(rng, 2, checker.mac1_key)], [148, 0]),   # a UDP-GRO run, then a response
               ([ini["d"].msg, struct.pack("<I", 3) + rng.bytes(60)], [0, 0])]          # single datagrams
    for b, (datagrams, sizes) in enumerate(batches):
        for k, (dg, g) in enumerate(zip(datagrams, sizes)):
            at = b * pitch + k * s.in_stride
            land[at:at + len(dg)] = np.frombuffer(dg, np.uint8)
            n_in[b * N_MSGS + FIRST_MSG_AT + k], gso[b * N_MSGS + FIRST_MSG_AT + k] = len(dg), g
    want = path_ref.recv_ref(s, land, n_in, gso)
    rows_of = {k: [] for k in names}
    consumed = np.zeros(n, np.int32)
    want_init = np.full(n, 0xEE, np.uint8).repeat(128).view(HS_INIT_DTYPE)
    for q in range(n):
        if want.type[q] == 1:
            msg = want.arena_split[q * stride:q * stride + 148].tobytes()
            for k, p in ini.items():
                if p.msg == msg:
                    rows_of[k].append(q)
            consumed[q], row = noise.consume_initiation(responder, table, msg)
            want_init[q] = row[0]
    assert [len(rows_of[k]) for k in names] == [1, 2, 1, 1]
    assert (consumed == HS_CONSUMED).sum() == 5 and (consumed == ERR_AUTH).sum() == 1 and (consumed == ERR_NO_PEER).sum() == 1

    # the caller's pool: more tickets than winners, and one packet to seal per ticket
    n_tickets, key_fill = 5, 0xC3
    n_keys = 2 * n_tickets + 2
    tickets = cases.tickets_of(n_tickets, seed=460)
    want_resp = np.zeros(n_tickets, HS_RESP_DTYPE)
    want_count, want_verdict, want_peers = np.zeros(1, np.uint32), np.zeros(n, np.int32), peers.copy()
    noise.accept_host(want_init, consumed, NOW, table, peer_rows, want_peers, tickets, want_resp, want_count, want_verdict)
    winners = sorted((rows_of[k][0], k) for k in ("a", "b", "d"))  # ranked by row number
    assert want_count[0] == 3 and want_resp["init_row"][:3].tolist() == [q for q, _ in winners]
    assert want_verdict[rows_of["old"][0]] == ERR_REPLAY and want_verdict[rows_of["b"][1]] == ERR_REPLAY
    assert all(want_verdict[q] == HS_ACCEPTED for q, _ in winners)
    gated = consumed != HS_CONSUMED
    assert np.array_equal(want_verdict[gated], consumed[gated])
    seal_pkts = np.zeros(n_tickets, AEAD_PKT_DTYPE)
    mtu, slot = 1420, 256
    seal_arena = np.full(n_tickets * slot + 64, SENTINEL, np.uint8)
    packets = []
    for j in range(n_tickets):
        length = 40 + 4 * j
        packets.append(bytes([0x45, 0, 0, length]) + rng.bytes(length - 4))  # an IPv4 header's first bytes: the trim keeps it all
        off = j * slot + 1 + j  # any byte offset
        seal_arena[off + 16:off + 16 + length] = np.frombuffer(packets[j], np.uint8)
        seal_pkts[j] = (off, (1 << 33) + j, length, int(tickets["send_key"][j]))

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_land, d_n_in, d_gso = up(land), torch.from_numpy(n_in).cuda(), torch.from_numpy(gso).cuda()
        d_slots = up(s.slots)
        d_checker = up(np.frombuffer(checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE))
        d_responder, d_table, d_psk = up(responder), up(table), up(psk)
        d_peer_rows, d_peers, d_tickets = up(peer_rows), up(peers), up(tickets)
        d_arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
        i32 = lambda m, fill=MARK: torch.full((m,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
        d_n_out, d_from, d_count, d_split_status = i32(n), i32(n), i32(nb), i32(nb)
        d_pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        d_type, d_screen, d_consumed, d_verdict = i32(n), i32(n), i32(n), i32(n)
        d_init = torch.full((128 * n,), 0xEE, dtype=torch.uint8, device="cuda")
        d_resp = torch.full((80 * n_tickets,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_n_resp = i32(1)
        d_keys = torch.full((48 * n_keys,), key_fill, dtype=torch.uint8, device="cuda")
        d_msgs = torch.full((PITCH * n_tickets,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_status = i32(n_tickets)
        d_seal_arena, d_seal_pkts, d_out_len = up(seal_arena), up(seal_pkts), i32(n_tickets)
        stream.synchronize()
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d_land.data_ptr(), s.in_stride, s.buf_len, d_n_in.data_ptr(),
                                               d_gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, d_arena.data_ptr(), stride,
                                               d_n_out.data_ptr(), d_from.data_ptr(), d_count.data_ptr(),
                                               d_split_status.data_ptr(), stream.cuda_stream)
        assert rc == 0
        router.classify_batch(dev, d_arena, d_n_out, d_slots, d_pkts, d_type, stride=stride, stream=stream, n=n,
                              n_slots=len(s.slots))
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_screen, under_load=False, stream=stream, n=n)
        noise.consume_batch(dev, d_arena, d_pkts, d_type, d_screen, d_responder, d_table, d_consumed, d_init,
                            stream=stream, n=n, n_peers=n_peers)
        noise.accept_batch(dev, d_init, d_consumed, NOW, d_table, d_peer_rows, d_peers, d_tickets, d_resp, d_n_resp,
                           d_verdict, stream=stream, n=n, n_ids=n_ids, n_peers=n_peers, n_tickets=n_tickets)
        noise.respond_batch(dev, d_resp, d_init, None, d_table, d_psk, d_keys, d_msgs, d_status, stream=stream,
                            n=n_tickets, n_init=n, n_peers=n_peers, n_keys=n_keys)
        transport.seal_batch(dev, d_seal_arena, d_seal_pkts, d_keys, mtu, d_out_len, stream=stream, n=n_tickets,
                             n_keys=n_keys)
        stream.synchronize()
    assert np.array_equal(d_type.cpu().numpy(), want.type)
    assert np.array_equal(d_consumed.cpu().numpy(), consumed)
    assert d_init.cpu().numpy().tobytes() == want_init.tobytes()
    assert np.array_equal(d_verdict.cpu().numpy(), want_verdict)
    assert d_n_resp.item() == 3
    assert d_resp.cpu().numpy().tobytes() == want_resp.tobytes()
    assert d_peers.cpu().numpy().tobytes() == want_peers.tobytes()
    assert d_tickets.cpu().numpy().tobytes() == tickets.tobytes()
    status, msgs = d_status.cpu().numpy(), d_msgs.cpu().numpy()
    keys = d_keys.cpu().numpy().view(AEAD_KEY_DTYPE)
    sealed, out_len = d_seal_arena.cpu().numpy(), d_out_len.cpu().numpy()
    # the replayed and the duplicate rows got no response: three descriptors, and the tail is turned away unread
    assert status.tolist() == [HS_RESPONDED] * 3 + [ERR_INVALID_ARG] * 2
    assert (msgs[PITCH * 3:] == SENTINEL).all(), "a tail descriptor has no response"
    assert (keys.view(np.uint8).reshape(n_keys, 48)[[0, 7, 8, 9, 10, n_keys - 1]] == key_fill).all()
    for j, (q, k) in enumerate(winners):
        p = ini[k]
        local_index = int(tickets["local_index"][j])
        msg = msgs[PITCH * j:PITCH * j + 92].tobytes()
        assert cookie_ref.Checker(p.public).check_mac1(msg), "CheckMAC1 on the initiator's side"
        assert msg[76:] == (cookie_ref.mac128(peers["cookie"][p.peer_row].tobytes(), msg[:76]) if k == "b" else bytes(16))
        rc, sender, send, recv, _, _ = noise_resp_ref.consume_response(p.private, p.hash, p.chain, p.eph, p.index, msg, p.psk)
        assert (rc, sender) == (0, local_index), k
        assert keys[2 * j + 1].tobytes() == noise_resp_ref.aead_key_bytes(recv, p.index)
        assert keys[2 * j + 2].tobytes() == noise_resp_ref.aead_key_bytes(send, 0)
        # the packet the responder sealed under its fresh send key opens under the initiator's receive key
        off = int(seal_pkts["off"][j])
        assert out_len[j] == 32 + len(packets[j]) + aead_ref.padding(len(packets[j]), mtu)
        wire = sealed[off:off + out_len[j]].tobytes()
        assert wire == aead_ref.wg_seal(recv, p.index, (1 << 33) + j, packets[j], mtu)
        ctr, plain = aead_ref.wg_open(recv, wire)
        assert ctr == (1 << 33) + j and plain[:len(packets[j])] == packets[j]
