"""Keypair rotation inside the two chains, each enqueued on one stream with no
synchronisation between its calls: the handshake batches write fresh keys,
the wgcs_keypairs calls put them to use, and the transport batches that follow
on the stream find them through the slot tables.  The peers' sides are computed
on the CPU beforehand -- every ephemeral key is fixed, so the session keys are
known before anything runs -- by the restatements of tests/noise_ref.py,
tests/noise_resp_ref.py and tests/aead_ref.py."""
import struct

import numpy as np
import pytest
import torch

import aead_ref
import cookie_ref
import noise_accept_cases as accept_cases
import noise_ref
import noise_resp_ref
from keypairs_ref import CLAIM_NONE, HS_BEGUN, HS_NONE, INITIATOR, NO_KEYPAIR, PEER_NONE, SET
from path_ref import FIRST_MSG_AT, LAND_SENTINEL, N_MSGS, RECV_SENTINEL
from test_gpu_cookie import SENTINEL, up
from wireguard_amd import cookie, keypairs, keystate, noise, router, transport
from wireguard_amd._lib import ERR_INVALID_ARG, ERR_NO_HANDSHAKE, HS_FINISHED, HS_RESPONDED, REJECT_AFTER_MESSAGES
from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.noise import HS_START_DTYPE, HS_STATE_DTYPE
from wireguard_amd.router import SESSION_SLOT_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

NOW = accept_cases.NOW
MTU, SLOT, MARK = 1420, 256, 12345
SRC, DST = bytes([192, 168, 1, 7]), bytes([10, 1, 2, 3])


def ipv4(rng, length: int) -> bytes:
    """an IPv4 packet of `length` bytes from SRC: what open trims to and the source check reads"""
    return bytes([0x45, 0]) + struct.pack(">H", length) + rng.bytes(8) + SRC + DST + rng.bytes(length - 20)


def key_row(key: bytes, remote_index: int) -> np.ndarray:
    return np.frombuffer(noise_resp_ref.aead_key_bytes(key, remote_index), AEAD_KEY_DTYPE)[0]


def slot_map(slots) -> dict:
    return {int(s["index"]): int(s["key"]) for s in slots if s["key"] != 0xFFFFFFFF}


def i32(m, fill=MARK):
    return torch.full((m,), fill, dtype=torch.int32, device="cuda")


def u8(m, fill=SENTINEL):
    return torch.full((m,), fill, dtype=torch.uint8, device="cuda")


def send_job(rng, peer: int, lengths):
    """One Tun.Read job of len(lengths) segments to `peer`, as gso_split_batch and route_dst_batch leave it:
    (arena, sizes, peer per slot, count, status, the packets)."""
    packets = [ipv4(rng, n) for n in lengths]
    arena = np.full(len(lengths) * SLOT + 64, SENTINEL, np.uint8)
    for k, p in enumerate(packets):
        arena[k * SLOT + 16:k * SLOT + 16 + len(p)] = np.frombuffer(p, np.uint8)
    return (arena, np.array(lengths, np.int32), np.full(len(lengths), peer, np.uint32), np.array([len(lengths)], np.int32),
            np.zeros(1, np.int32), packets)


class SendJob:
    def __init__(self, rng, peer, lengths):
        self.arena, sizes, peers, count, status, self.packets = send_job(rng, peer, lengths)
        self.m = len(lengths)
        self.d_arena, self.d_sizes, self.d_peer = up(self.arena), up(sizes), up(peers)
        self.d_count, self.d_status = up(count), up(status)
        self.d_pkts, self.d_nbufs, self.d_job_key, self.d_out_len = u8(24 * self.m, 0xEE), i32(1), i32(1), i32(self.m)

    def enqueue(self, dev, d_peer_keys, n_peer_slots, d_nonce, d_keys, n_keys, d_work, stream):
        keystate.send_assign_batch(dev, self.d_sizes, self.d_peer, self.d_count, self.d_status, self.m, SLOT, d_peer_keys,
                                   d_nonce, self.d_pkts, self.d_nbufs, self.d_job_key, d_work, stream=stream, n_jobs=1,
                                   n_slots=n_peer_slots, n_keys=n_keys)
        transport.seal_batch(dev, self.d_arena, self.d_pkts, d_keys, MTU, self.d_out_len, stream=stream, n=self.m,
                             n_keys=n_keys)


def test_responder_chain_from_split_to_the_first_packet_under_the_new_keypair(dev):
    """split -> classify -> open -> screen -> consume -> accept -> respond -> begin_responder, a send job, then
    a second receive batch classify -> open -> replay -> received -> source, and the send job again.

    The peer holds an old current keypair whose send nonce is spent (why it rekeys) and an old previous one.  A
    transport packet to the ticket's index that arrives in the first batch, before the begin, is refused by open.
    After the begin the new keypair is next: the first send job finds only the spent current and is dropped.  The
    second receive batch holds one packet under the new keypair, one under the old current and one to the old
    previous's index: the first promotes next, the second still opens, the third is refused and the previous
    keypair's key rows are zero.  The send job then seals under the new key and opens on the initiator's side."""
    rng = np.random.default_rng(664)
    private = rng.bytes(32)
    responder, public = noise.responder_init(private)
    checker = cookie_ref.Checker(public)
    ini_private, ini_eph, ini_index = rng.bytes(32), rng.bytes(32), 0x0A0B0C0D
    ini_public = noise_ref.public_key(ini_private)
    others = [noise_ref.public_key(rng.bytes(32)) for _ in range(3)]
    peer_id, n_ids = 52, 60
    table = noise.peer_keys_build(responder, [ini_public] + others, [peer_id, 53, 54, 55])
    n_peers, pr = len(table), noise.peer_keys_find(table, ini_public)
    peer_rows = noise.peer_rows_build(table, n_ids)
    hs_peers = accept_cases.peers_of(n_peers, seed=665)
    hs_peers["flags"] = 0
    msg, _, _ = noise.create_initiation(ini_private, public, ini_eph, accept_cases.T[1], ini_index)
    msg = cookie_ref.add_macs(checker.mac1_key, msg)[0]
    consumed, init_row = noise.consume_initiation(responder, table, msg)
    assert consumed == noise.HS_CONSUMED
    # the tickets: the first is taken; its ephemeral is fixed, so the restatement's responder knows the keys
    tickets = accept_cases.tickets_of(2, seed=666)
    tickets["send_key"], tickets["recv_key"] = [4, 6], [5, 7]
    t_index = int(tickets["local_index"][0])
    rc, want_msg, new_send, new_recv, _, _ = noise_resp_ref.create_response(
        init_row.tobytes(), ini_public, tickets["ephemeral_private"][0].tobytes(), t_index)
    assert rc == 0
    # the keypairs the peer has had so far: current (rows 0, 1) and previous (rows 2, 3)
    cur_send, cur_recv, prev_send, prev_recv = (rng.bytes(32) for _ in range(4))
    cur_index, prev_index, cur_remote, prev_remote = 0x11110001, 0x11110002, 0x22220001, 0x22220002
    n_keys = 8
    keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    keys[0], keys[1], keys[2], keys[3] = (key_row(cur_send, cur_remote), key_row(cur_recv, 0), key_row(prev_send, prev_remote),
                                          key_row(prev_recv, 0))
    key_peer = np.array([peer_id] * 4 + [PEER_NONE] * 4, np.uint32)
    kp = keypairs.keypairs_table(n_peers)
    kp["current"][pr], kp["previous"][pr] = (0, 1, cur_index, SET, NOW - 170 * 10**9), (2, 3, prev_index, SET, NOW - 300 * 10**9)
    slots = router.session_table(np.array([cur_index, prev_index, t_index, int(tickets["local_index"][1])], np.uint32),
                                 np.array([1, 3, NO_KEYPAIR, NO_KEYPAIR], np.uint32))
    peer_keys = router.session_table(table["peer"], np.where(table["peer"] == peer_id, 0, NO_KEYPAIR).astype(np.uint32))
    nonce = np.zeros(n_keys, np.uint64)
    nonce[0] = REJECT_AFTER_MESSAGES  # the old current can send no more
    r = router.Router()
    r.insert(bytes([192, 168, 1, 0]), 24, peer_id)
    image = r.image()

    # the first receive batch through split: the initiation, and a transport packet that is too early
    early = aead_ref.wg_seal(new_recv, t_index, 0, ipv4(rng, 60), MTU)
    stride, in_stride, buf_len, n = 4112, 4099, 4096, N_MSGS
    land = np.full((N_MSGS - FIRST_MSG_AT) * in_stride, LAND_SENTINEL, np.uint8)
    n_in, gso = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k, dg in enumerate((msg, early)):
        land[k * in_stride:k * in_stride + len(dg)] = np.frombuffer(dg, np.uint8)
        n_in[FIRST_MSG_AT + k] = len(dg)
    # the second receive batch, as the wire gives it
    plain = [ipv4(rng, 84), ipv4(rng, 52), ipv4(rng, 44)]
    wire = [aead_ref.wg_seal(new_recv, t_index, 0, plain[0], MTU), aead_ref.wg_seal(cur_recv, cur_index, 5, plain[1], MTU),
            aead_ref.wg_seal(prev_recv, prev_index, 9, plain[2], MTU)]
    m = len(wire)
    arena2 = np.full(m * SLOT + 8, RECV_SENTINEL, np.uint8)
    off2 = np.array([k * SLOT + 1 + k for k in range(m)], np.uint64)  # any byte offset
    for o, wmsg in zip(off2, wire):
        arena2[int(o):int(o) + len(wmsg)] = np.frombuffer(wmsg, np.uint8)
    size2 = np.array([len(x) for x in wire], np.int32)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_land, d_n_in, d_gso = up(land), up(n_in), up(gso)
        d_checker = up(np.frombuffer(checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE))
        d_responder, d_table, d_peer_rows, d_hs_peers, d_tickets = up(responder), up(table), up(peer_rows), up(hs_peers), up(tickets)
        d_kp, d_slots, d_peer_keys, d_keys, d_key_peer = up(kp), up(slots), up(peer_keys), up(keys), up(key_peer)
        d_nonce, d_filters, d_image = up(nonce), up(np.zeros(n_keys, REPLAY_FILTER_DTYPE)), up(image)
        d_arena = u8(n * stride, RECV_SENTINEL)
        d_n_out, d_from, d_count, d_split_status = i32(n), i32(n), i32(1), i32(1)
        d_pkts = u8(24 * n, 0xEE)
        d_type, d_screen, d_consumed, d_verdict, d_len1 = (i32(n) for _ in range(5))
        d_ctr1 = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_init, d_resp, d_n_resp = u8(128 * n, 0xEE), u8(80 * 2), i32(1)
        d_msgs, d_status, d_begun = u8(96 * 2), i32(2), i32(2 + 1)
        d_work = torch.zeros(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")
        d_arena2, d_off2, d_size2 = up(arena2), up(off2), up(size2)
        d_pkts2, d_type2, d_len2, d_verdict2, d_found = u8(24 * m, 0xEE), i32(m), i32(m), i32(m), i32(m)
        d_ctr2 = torch.zeros(m, dtype=torch.int64, device="cuda")
        d_rotated = i32(m + 1)
        before, after = SendJob(rng, peer_id, [40, 72]), SendJob(rng, peer_id, [40, 72])
        stream.synchronize()
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d_land.data_ptr(), in_stride, buf_len, d_n_in.data_ptr(),
                                               d_gso.data_ptr(), N_MSGS, FIRST_MSG_AT, 1, d_arena.data_ptr(), stride,
                                               d_n_out.data_ptr(), d_from.data_ptr(), d_count.data_ptr(),
                                               d_split_status.data_ptr(), stream.cuda_stream)
        assert rc == 0
        router.classify_batch(dev, d_arena, d_n_out, d_slots, d_pkts, d_type, stride=stride, stream=stream, n=n,
                              n_slots=len(slots))
        transport.open_batch(dev, d_arena, d_pkts, d_keys, d_len1, d_ctr1, stream=stream, n=n, n_keys=n_keys)
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_screen, under_load=False, stream=stream, n=n)
        noise.consume_batch(dev, d_arena, d_pkts, d_type, d_screen, d_responder, d_table, d_consumed, d_init, stream=stream,
                            n=n, n_peers=n_peers)
        noise.accept_batch(dev, d_init, d_consumed, NOW, d_table, d_peer_rows, d_hs_peers, d_tickets, d_resp, d_n_resp,
                           d_verdict, stream=stream, n=n, n_ids=n_ids, n_peers=n_peers, n_tickets=2)
        noise.respond_batch(dev, d_resp, d_init, None, d_table, None, d_keys, d_msgs, d_status, stream=stream, n=2,
                            n_init=n, n_peers=n_peers, n_keys=n_keys)
        keypairs.begin_responder_batch(dev, d_resp, d_status, NOW, d_table, d_kp, d_slots, d_peer_keys, d_keys, d_key_peer,
                                       d_begun, d_work, stream=stream, n=2, n_peers=n_peers, n_slots=len(slots),
                                       n_peer_slots=len(peer_keys), n_keys=n_keys)
        before.enqueue(dev, d_peer_keys, len(peer_keys), d_nonce, d_keys, n_keys, d_work, stream)
        router.classify_batch(dev, d_arena2, d_size2, d_slots, d_pkts2, d_type2, off=d_off2, stream=stream, n=m,
                              n_slots=len(slots))
        transport.open_batch(dev, d_arena2, d_pkts2, d_keys, d_len2, d_ctr2, stream=stream, n=m, n_keys=n_keys)
        keystate.replay_batch(dev, d_pkts2, d_len2, d_ctr2, d_filters, d_verdict2, d_work, stream=stream, n=m, n_keys=n_keys)
        keypairs.received_batch(dev, d_pkts2, d_verdict2, d_key_peer, d_peer_rows, d_kp, d_slots, d_peer_keys, d_keys,
                                d_rotated, stream=stream, n=m, n_keys=n_keys, n_ids=n_ids, n_peers=n_peers,
                                n_slots=len(slots), n_peer_slots=len(peer_keys))
        router.source_batch(dev, d_arena2, d_pkts2, d_verdict2, d_key_peer, d_image, d_verdict2, peer=d_found, stream=stream,
                            n=m, n_keys=n_keys)
        after.enqueue(dev, d_peer_keys, len(peer_keys), d_nonce, d_keys, n_keys, d_work, stream)
        stream.synchronize()

    types, len1 = d_type.cpu().numpy(), d_len1.cpu().numpy()
    q_init, q_early = int(np.flatnonzero(types == 1)[0]), int(np.flatnonzero(types == 4)[0])
    assert (types == 1).sum() == 1 and (types == 4).sum() == 1
    pk1 = d_pkts.cpu().numpy().view(AEAD_PKT_DTYPE)
    assert pk1["key"][q_early] == NO_KEYPAIR and len1[q_early] == ERR_INVALID_ARG, "too early: the index has no keypair yet"
    assert d_verdict.cpu().numpy()[q_init] == noise.HS_ACCEPTED and d_n_resp.item() == 1
    assert d_status.cpu().tolist() == [HS_RESPONDED, ERR_INVALID_ARG]
    assert d_msgs.cpu().numpy()[:92].tobytes() == want_msg
    assert d_begun.cpu().tolist() == [HS_BEGUN, HS_NONE, MARK]
    # the send job between the begin and the first packet: next may not send, and current is spent
    assert before.d_nbufs.item() == 0 and before.d_job_key.cpu().numpy().view(np.uint32)[0] == 0xFFFFFFFF
    assert before.d_out_len.cpu().tolist() == [ERR_INVALID_ARG] * 2 and before.d_arena.cpu().numpy().tobytes() == before.arena.tobytes()
    # the second receive batch
    assert d_type2.cpu().tolist() == [4, 4, 4]
    pk2 = d_pkts2.cpu().numpy().view(AEAD_PKT_DTYPE)
    assert pk2["key"].tolist() == [5, 1, NO_KEYPAIR]
    assert d_rotated.cpu().tolist() == [1, 0, 0, MARK]
    assert d_verdict2.cpu().tolist() == [len(plain[0]), len(plain[1]), ERR_INVALID_ARG]
    got2 = d_arena2.cpu().numpy()
    for k in (0, 1):
        o = int(off2[k]) + 16
        assert got2[o:o + len(plain[k])].tobytes() == plain[k], f"packet {k} did not open"
    o = int(off2[2])
    assert got2[o:o + len(wire[2])].tobytes() == wire[2], "the refused message is untouched"
    assert d_found.cpu().numpy().view(np.uint32)[:2].tolist() == [peer_id, peer_id]
    # the tables
    got_kp = d_kp.cpu().numpy().view(KEYPAIRS_DTYPE)
    assert tuple(got_kp["previous"][pr]) == (0, 1, cur_index, SET, NOW - 170 * 10**9)
    assert tuple(got_kp["current"][pr]) == (4, 5, t_index, SET, NOW) and got_kp["next"][pr]["flags"] == 0
    assert (got_kp["claim"] == CLAIM_NONE).all()
    others_rows = [x for x in range(n_peers) if x != pr]
    assert got_kp[others_rows].tobytes() == kp[others_rows].tobytes()
    got_keys = d_keys.cpu().numpy().view(AEAD_KEY_DTYPE)
    assert not got_keys[2:4].view(np.uint8).any(), "the old previous's key rows are zero"
    assert got_keys[4].tobytes() == noise_resp_ref.aead_key_bytes(new_send, ini_index)
    assert got_keys[5].tobytes() == noise_resp_ref.aead_key_bytes(new_recv, 0)
    assert got_keys[[0, 1, 6, 7]].tobytes() == keys[[0, 1, 6, 7]].tobytes()
    assert d_key_peer.cpu().numpy().view(np.uint32).tolist() == [peer_id, peer_id, PEER_NONE, PEER_NONE, peer_id, peer_id,
                                                                  PEER_NONE, PEER_NONE]
    assert slot_map(d_slots.cpu().numpy().view(SESSION_SLOT_DTYPE)) == {
        cur_index: 1, prev_index: NO_KEYPAIR, t_index: 5, int(tickets["local_index"][1]): NO_KEYPAIR}
    got_pk = slot_map(d_peer_keys.cpu().numpy().view(SESSION_SLOT_DTYPE))
    assert got_pk[peer_id] == 4 and all(v == NO_KEYPAIR for k, v in got_pk.items() if k != peer_id)
    # the send job after the first packet: sealed under the promoted key, and the initiator opens it
    assert after.d_nbufs.item() == 2 and after.d_job_key.cpu().numpy().view(np.uint32)[0] == 4
    sealed, out_len = after.d_arena.cpu().numpy(), after.d_out_len.cpu().numpy()
    for k, p in enumerate(after.packets):
        w = sealed[k * SLOT:k * SLOT + out_len[k]].tobytes()
        assert w == aead_ref.wg_seal(new_send, ini_index, k, p, MTU)
        ctr, opened = aead_ref.wg_open(new_send, w)
        assert ctr == k and opened[:len(p)] == p
    assert d_nonce.cpu().numpy().view(np.uint64).tolist() == [REJECT_AFTER_MESSAGES, 0, 0, 0, 2, 0, 0, 0]


def test_initiator_chain_from_initiate_to_the_first_sealed_packet(dev):
    """initiate -> (the restatement's responder answers) -> classify -> screen -> finish -> begin_initiator ->
    send-assign -> seal, then a following receive batch with the response once more and a packet under the
    former current keypair.  The response is in the first batch twice.  The sealed packet opens under the
    responder's receive key; the former current is previous and its traffic still opens; the duplicate
    responses change nothing."""
    rng = np.random.default_rng(700)
    a_private, b_private = rng.bytes(32), rng.bytes(32)
    a_self, a_public = noise.responder_init(a_private)
    b_public = noise_ref.public_key(b_private)
    others = [noise_ref.public_key(rng.bytes(32)) for _ in range(3)]
    peer_id = 71
    table = noise.peer_keys_build(a_self, [b_public] + others, [peer_id, 72, 73, 74])
    n_peers, pr = len(table), noise.peer_keys_find(table, b_public)
    b_self, _ = noise.responder_init(b_private)
    b_table = noise.peer_keys_build(b_self, [a_public], [5])
    local_index, b_index, eph, ts = 0x0C0FFEE0, 0x0B0B0B0B, rng.bytes(32), accept_cases.T[2]
    start = np.zeros(1, HS_START_DTYPE)
    start[0] = (0, pr, local_index, 2, 3, 0, np.frombuffer(ts, np.uint8), 0, np.frombuffer(eph, np.uint8), 0, 0)
    # B's side, on the CPU: consume the initiation A will build, answer it, keep the keys
    init_msg, _, _ = noise.create_initiation(a_private, b_public, eph, ts, local_index)
    init_msg = cookie_ref.add_macs(noise_resp_ref.mac1_key(b_public), init_msg)[0]
    consumed, init_row = noise.consume_initiation(b_self, b_table, init_msg)
    assert consumed == noise.HS_CONSUMED
    rc, response, b_send, b_recv, _, _ = noise_resp_ref.create_response(init_row.tobytes(), a_public, rng.bytes(32), b_index)
    assert rc == 0
    # A's keypair with B so far: current, as the initiator (rows 0, 1)
    cur_send, cur_recv, cur_index, cur_remote = rng.bytes(32), rng.bytes(32), 0x33330001, 0x44440001
    n_keys = 6
    keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    keys[0], keys[1] = key_row(cur_send, cur_remote), key_row(cur_recv, 0)
    key_peer = np.array([peer_id, peer_id] + [PEER_NONE] * 4, np.uint32)
    kp = keypairs.keypairs_table(n_peers)
    kp["current"][pr] = (0, 1, cur_index, SET | INITIATOR, NOW - 120 * 10**9)
    slots = router.session_table(np.array([cur_index, local_index], np.uint32), np.array([1, NO_KEYPAIR], np.uint32))
    hs_slots = router.session_table(np.array([local_index], np.uint32), np.array([0], np.uint32))
    peer_keys = router.session_table(table["peer"], np.where(table["peer"] == peer_id, 0, NO_KEYPAIR).astype(np.uint32))
    checker = np.frombuffer(cookie_ref.Checker(a_public).tobytes(), cookie.COOKIE_CHECKER_DTYPE)
    # the two receive batches: the response twice; the response once more and a packet under the former current
    old_plain = ipv4(rng, 64)
    old_wire = aead_ref.wg_seal(cur_recv, cur_index, 77, old_plain, MTU)
    batches = [[response, response], [response, old_wire]]
    arenas, offs, sizes = [], [], []
    for msgs in batches:
        a = np.full(2 * SLOT + 8, RECV_SENTINEL, np.uint8)
        o = np.array([3, SLOT + 2], np.uint64)
        for at, x in zip(o, msgs):
            a[int(at):int(at) + len(x)] = np.frombuffer(x, np.uint8)
        arenas.append(a), offs.append(o), sizes.append(np.array([len(x) for x in msgs], np.int32))

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_start, d_pub, d_table, d_self, d_checker = up(start), up(np.frombuffer(a_public, np.uint8)), up(table), up(a_self), up(checker)
        d_states, d_init_msgs, d_status = u8(128), u8(160), i32(1)
        d_kp, d_slots, d_hs_slots, d_peer_keys, d_keys, d_key_peer = (up(x) for x in (kp, slots, hs_slots, peer_keys, keys, key_peer))
        d_nonce = up(np.zeros(n_keys, np.uint64))
        d_work = torch.zeros(keystate.work_bytes(2), dtype=torch.uint8, device="cuda")
        d_fwork = u8(noise.FINISH_WORK_BYTES * 2)
        d = [dict(arena=up(arenas[b]), off=up(offs[b]), size=up(sizes[b]), pkts=u8(48, 0xEE), type=i32(2), screen=i32(2),
                  finished=i32(2), begun=i32(3), len=i32(2), ctr=torch.zeros(2, dtype=torch.int64, device="cuda"))
             for b in range(2)]
        job = SendJob(rng, peer_id, [48])
        d_snap = [torch.zeros_like(x) for x in (d_kp, d_slots, d_peer_keys, d_keys, d_key_peer)]
        stream.synchronize()
        noise.initiate_batch(dev, d_start, d_pub, d_table, d_states, d_init_msgs, d_status, n_keys, stream=stream, n=1,
                             n_peers=n_peers, n_states=1)
        for b, x in enumerate(d):
            router.classify_batch(dev, x["arena"], x["size"], d_slots, x["pkts"], x["type"], off=x["off"], stream=stream, n=2,
                                  n_slots=len(slots))
            cookie.screen_batch(dev, x["arena"], x["pkts"], x["type"], d_checker, None, x["screen"], under_load=False,
                                stream=stream, n=2)
            noise.finish_batch(dev, x["arena"], x["pkts"], x["type"], x["screen"], d_self, d_hs_slots, d_states, None, d_keys,
                               d_fwork, x["finished"], stream=stream, n=2, n_slots=len(hs_slots), n_states=1,
                               n_peers=n_peers, n_keys=n_keys)
            keypairs.begin_initiator_batch(dev, x["arena"], x["pkts"], x["finished"], NOW + b, d_hs_slots, d_states, d_table,
                                           d_kp, d_slots, d_peer_keys, d_keys, d_key_peer, x["begun"], d_work, stream=stream,
                                           n=2, n_hs_slots=len(hs_slots), n_states=1, n_peers=n_peers, n_slots=len(slots),
                                           n_peer_slots=len(peer_keys), n_keys=n_keys)
            if b == 0:
                job.enqueue(dev, d_peer_keys, len(peer_keys), d_nonce, d_keys, n_keys, d_work, stream)
                for dst, src in zip(d_snap, (d_kp, d_slots, d_peer_keys, d_keys, d_key_peer)):
                    dst.copy_(src)  # on the stream: the tables as the first batch left them
            else:
                transport.open_batch(dev, x["arena"], x["pkts"], d_keys, x["len"], x["ctr"], stream=stream, n=2, n_keys=n_keys)
        stream.synchronize()

    assert d_status.cpu().tolist() == [noise.HS_INITIATED]
    assert d_init_msgs.cpu().numpy()[:148].tobytes() == init_msg
    assert d[0]["type"].cpu().tolist() == [2, 2] and d[0]["finished"].cpu().tolist() == [HS_FINISHED, ERR_NO_HANDSHAKE]
    assert d[0]["begun"].cpu().tolist() == [HS_BEGUN, HS_NONE, MARK]
    # the new keypair is current at once and the send chain seals under it
    a_send, a_recv = b_recv, b_send
    got_keys = d_keys.cpu().numpy().view(AEAD_KEY_DTYPE)
    assert got_keys[2].tobytes() == noise_resp_ref.aead_key_bytes(a_send, b_index)
    assert got_keys[3].tobytes() == noise_resp_ref.aead_key_bytes(a_recv, 0)
    assert got_keys[[0, 1, 4, 5]].tobytes() == keys[[0, 1, 4, 5]].tobytes()
    assert job.d_nbufs.item() == 1 and job.d_job_key.cpu().numpy().view(np.uint32)[0] == 2
    n_out = job.d_out_len.cpu().numpy()[0]
    w = job.d_arena.cpu().numpy()[:n_out].tobytes()
    assert w == aead_ref.wg_seal(b_recv, b_index, 0, job.packets[0], MTU)
    ctr, opened = aead_ref.wg_open(b_recv, w)
    assert ctr == 0 and opened[:48] == job.packets[0], "the responder opens it under its receive key"
    got_kp = d_kp.cpu().numpy().view(KEYPAIRS_DTYPE)
    assert tuple(got_kp["previous"][pr]) == (0, 1, cur_index, SET | INITIATOR, NOW - 120 * 10**9)
    assert tuple(got_kp["current"][pr]) == (2, 3, local_index, SET | INITIATOR, NOW) and got_kp["next"][pr]["flags"] == 0
    assert slot_map(d_slots.cpu().numpy().view(SESSION_SLOT_DTYPE)) == {cur_index: 1, local_index: 3}
    assert slot_map(d_peer_keys.cpu().numpy().view(SESSION_SLOT_DTYPE))[peer_id] == 2
    assert d_key_peer.cpu().numpy().view(np.uint32).tolist() == [peer_id] * 4 + [PEER_NONE] * 2
    # the following batch: the duplicate response changes nothing, the former current's packet still opens
    assert d[1]["type"].cpu().tolist() == [2, 4] and d[1]["finished"].cpu().tolist() == [ERR_NO_HANDSHAKE, HS_NONE]
    assert d[1]["begun"].cpu().tolist() == [HS_NONE, HS_NONE, MARK]
    for snap, now in zip(d_snap, (d_kp, d_slots, d_peer_keys, d_keys, d_key_peer)):
        assert snap.cpu().numpy().tobytes() == now.cpu().numpy().tobytes()
    pk = d[1]["pkts"].cpu().numpy().view(AEAD_PKT_DTYPE)
    assert pk["key"][1] == 1 and d[1]["len"].cpu().tolist()[1] == len(old_plain) and d[1]["ctr"].cpu().tolist()[1] == 77
    o = int(offs[1][1]) + 16
    assert d[1]["arena"].cpu().numpy()[o:o + len(old_plain)].tobytes() == old_plain
    states = d_states.cpu().numpy().view(HS_STATE_DTYPE)
    assert states[0].tobytes() == np.array([(0, local_index, pr, b_index, 2, 3, 0xFFFFFFFF, 0, 0, 0, 0)], HS_STATE_DTYPE).tobytes()
