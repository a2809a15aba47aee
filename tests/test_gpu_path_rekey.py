"""A session that ages out on the device is renewed on the device: both
endpoints' chains enqueued on one stream with a single synchronise at the end.

The initiator's current keypair is 181 s old on the caller's clock.  Its send
job is refused by the send gate, the start call turns the wish into a
wgcs_hs_start descriptor, initiate builds the message; the responder consumes
it, answers, notes lastSentHandshake and installs its next keypair; the
initiator finishes and installs its current one; the same job passes the gate
and is sealed under the new key; the responder's receive chain opens it, while
a packet under the old keypair, offered at the same clock, is turned away by
the receive gate with its bytes untouched.  A message crosses from one
endpoint's buffer to the other's by a copy on the stream.  The worlds are built
with the helpers of tests/test_gpu_path_keypairs.py."""
import numpy as np
import pytest
import torch

import aead_ref
import cookie_ref
import noise_accept_cases as accept_cases
from keypairs_ref import HS_BEGUN, INITIATOR, NO_KEYPAIR, PEER_NONE, SET
from path_ref import RECV_SENTINEL
from rekey_ref import ERR_KEY_EXPIRED, HS_STARTED, SECOND, SESSION_EXPIRED, WANT_REJECT_TIME
from test_gpu_path_keypairs import MARK, MTU, SLOT, SendJob, i32, ipv4, key_row, u8, up
from wireguard_amd import cookie, keypairs, keystate, noise, rekey, router, transport
from wireguard_amd._lib import ERR_INVALID_ARG, HS_FINISHED, HS_RESPONDED, REJECT_AFTER_MESSAGES
from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.noise import HS_START_DTYPE
from wireguard_amd.rekey import REKEY_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

NOW = accept_cases.NOW
LENGTHS = [40, 72]


def test_an_aged_session_is_renewed_without_a_host_step(dev):
    rng = np.random.default_rng(1801)
    a_private, b_private = rng.bytes(32), rng.bytes(32)
    a_self, a_public = noise.responder_init(a_private)
    b_self, b_public = noise.responder_init(b_private)
    others = [noise.responder_init(rng.bytes(32))[1] for _ in range(3)]
    b_at_a, a_at_b, n_ids = 71, 52, 80  # the peer ids each side knows the other by
    a_table = noise.peer_keys_build(a_self, [b_public] + others, [b_at_a, 72, 73, 74])
    b_table = noise.peer_keys_build(b_self, [a_public] + others, [a_at_b, 53, 54, 55])
    n_peers = 4
    a_pr, b_pr = noise.peer_keys_find(a_table, b_public), noise.peer_keys_find(b_table, a_public)
    a_rows, b_rows = noise.peer_rows_build(a_table, n_ids), noise.peer_rows_build(b_table, n_ids)
    # the established session: A initiated it 181 s ago; A seals under old_ab, B under old_ba
    old_ab, old_ba, a_old_index, b_old_index = rng.bytes(32), rng.bytes(32), 0x33330001, 0x44440001
    created = NOW - 181 * SECOND
    n_keys = 4
    a_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    b_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    a_keys[0], a_keys[1] = key_row(old_ab, b_old_index), key_row(old_ba, 0)
    b_keys[0], b_keys[1] = key_row(old_ba, a_old_index), key_row(old_ab, 0)
    a_kp, b_kp = keypairs.keypairs_table(n_peers), keypairs.keypairs_table(n_peers)
    a_kp["current"][a_pr] = (0, 1, a_old_index, SET | INITIATOR, created)
    b_kp["current"][b_pr] = (0, 1, b_old_index, SET, created)
    a_key_peer = np.array([b_at_a, b_at_a, PEER_NONE, PEER_NONE], np.uint32)
    b_key_peer = np.array([a_at_b, a_at_b, PEER_NONE, PEER_NONE], np.uint32)
    # what the hosts prepared: one ticket each, their indices registered without a keypair
    a_new_index, ts = 0x0C0FFEE0, accept_cases.T[2]
    a_tickets = np.zeros(1, HS_START_DTYPE)
    a_tickets[0] = (0, 0xEEEEEEEE, a_new_index, 2, 3, 0xEEEEEEEE, np.frombuffer(ts, np.uint8), 0xEE,
                    np.frombuffer(rng.bytes(32), np.uint8), 0xEE, 0xEE)
    b_tickets = accept_cases.tickets_of(1, seed=1802)
    b_tickets["send_key"], b_tickets["recv_key"] = 2, 3
    b_new_index = int(b_tickets["local_index"][0])
    a_slots = router.session_table(np.array([a_old_index, a_new_index], np.uint32), np.array([1, NO_KEYPAIR], np.uint32))
    b_slots = router.session_table(np.array([b_old_index, b_new_index], np.uint32), np.array([1, NO_KEYPAIR], np.uint32))
    a_hs_slots = router.session_table(np.array([a_new_index], np.uint32), np.array([0], np.uint32))
    a_peer_keys = router.session_table(a_table["peer"], np.where(a_table["peer"] == b_at_a, 0, NO_KEYPAIR).astype(np.uint32))
    b_peer_keys = router.session_table(b_table["peer"], np.where(b_table["peer"] == a_at_b, 0, NO_KEYPAIR).astype(np.uint32))
    a_hs_peers, b_hs_peers = accept_cases.peers_of(n_peers, seed=1803), accept_cases.peers_of(n_peers, seed=1804)
    a_hs_peers["flags"], b_hs_peers["flags"] = 0, 0
    a_rekey, b_rekey = rekey.rekey_table(n_peers, NOW), rekey.rekey_table(n_peers, NOW)
    b_checker = np.frombuffer(cookie_ref.Checker(b_public).tobytes(), cookie.COOKIE_CHECKER_DTYPE)
    ra, rb = router.Router(), router.Router()
    ra.insert(bytes([10, 1, 2, 0]), 24, b_at_a)      # A routes the job's destination to B
    rb.insert(bytes([192, 168, 1, 0]), 24, a_at_b)   # B allows the job's source from A
    a_image, b_image = ra.image(), rb.image()
    # B's last receive batch: room for A's two sealed packets, and a packet under the old keypair at the same clock
    wire_len = [len(aead_ref.wg_seal(bytes(32), 0, 0, bytes(n), MTU)) for n in LENGTHS]
    old_plain = ipv4(rng, 60)
    old_wire = aead_ref.wg_seal(old_ab, b_old_index, 9, old_plain, MTU)
    m = 3
    off2 = np.array([k * SLOT + 1 + k for k in range(m)], np.uint64)  # any byte offset
    size2 = np.array(wire_len + [len(old_wire)], np.int32)
    arena2 = np.full(m * SLOT + 8, RECV_SENTINEL, np.uint8)
    arena2[int(off2[2]):int(off2[2]) + len(old_wire)] = np.frombuffer(old_wire, np.uint8)
    # what the host forms say of the two wgcs_rekey tables
    want_a, want_b = a_rekey.copy(), b_rekey.copy()
    job_peer, job_count, job_status = np.full(2, b_at_a, np.uint32), np.array([2], np.int32), np.zeros(1, np.int32)
    h_gate = np.zeros(1, np.int32)
    rekey.send_gate_host(job_peer, job_count, job_status, 2, NOW, a_rows, a_kp, np.zeros(n_keys, np.uint64),
                         REJECT_AFTER_MESSAGES, want_a, h_gate)
    assert h_gate.tolist() == [ERR_KEY_EXPIRED] and want_a["want"][a_pr] == WANT_REJECT_TIME
    h_start, h_sp, h_count = np.zeros(1, HS_START_DTYPE), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    h_status, h_reasons = np.zeros(n_peers, np.int32), np.zeros(n_peers, np.uint32)
    rekey.start_host(NOW, want_a, a_hs_peers, a_tickets, h_start, h_sp, h_count, h_status, h_reasons)
    h_resp = np.zeros(1, noise.HS_RESP_DTYPE)
    h_resp["peer_row"] = b_pr
    rekey.responded_host(h_resp, np.array([HS_RESPONDED], np.int32), NOW, want_b)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        A = {k: up(v) for k, v in dict(table=a_table, rows=a_rows, kp=a_kp, keys=a_keys, key_peer=a_key_peer, slots=a_slots,
                                       hs_slots=a_hs_slots, peer_keys=a_peer_keys, hs_peers=a_hs_peers, rekey=a_rekey,
                                       tickets=a_tickets, self=a_self, pub=np.frombuffer(a_public, np.uint8),
                                       image=a_image, nonce=np.zeros(n_keys, np.uint64)).items()}
        B = {k: up(v) for k, v in dict(table=b_table, rows=b_rows, kp=b_kp, keys=b_keys, key_peer=b_key_peer, slots=b_slots,
                                       peer_keys=b_peer_keys, hs_peers=b_hs_peers, rekey=b_rekey, tickets=b_tickets,
                                       self=b_self, checker=b_checker, image=b_image,
                                       filters=np.zeros(n_keys, REPLAY_FILTER_DTYPE)).items()}
        before, after = SendJob(np.random.default_rng(7), b_at_a, LENGTHS), SendJob(np.random.default_rng(7), b_at_a, LENGTHS)
        for job in (before, after):
            job.d_peer = i32(2)  # route-dst finds it
            job.d_status_in, job.d_status = job.d_status, i32(1 + 1)  # send-assign reads what the gate left
        d_start, d_start_peer, d_count, d_start_status, d_reasons = u8(96), i32(1 + 1), i32(1 + 1), i32(n_peers + 1), i32(n_peers + 1)
        d_states, d_init_msgs, d_init_status = u8(128), u8(160), i32(1)
        d_work = torch.zeros(keystate.work_bytes(8), dtype=torch.uint8, device="cuda")
        d_fwork = u8(noise.FINISH_WORK_BYTES)
        # B's handshake batch (one message) and A's (one message)
        d_arena_b1, d_size_b1 = u8(SLOT, RECV_SENTINEL), up(np.array([148], np.int32))
        d_pkts_b1, d_type_b1, d_screen_b1, d_consumed, d_accept = u8(24, 0xEE), i32(1), i32(1), i32(1), i32(1)
        d_hs_init, d_resp, d_n_resp, d_resp_msgs, d_resp_status, d_begun_b = u8(128, 0xEE), u8(80), i32(1), u8(96), i32(1), i32(1 + 1)
        d_arena_a1, d_size_a1 = u8(SLOT, RECV_SENTINEL), up(np.array([92], np.int32))
        d_pkts_a1, d_type_a1, d_finished, d_begun_a = u8(24, 0xEE), i32(1), i32(1), i32(1 + 1)
        # B's transport batch
        d_arena2, d_off2, d_size2 = up(arena2), up(off2), up(size2)
        d_pkts2, d_type2, d_len2, d_verdict2, d_found, d_rotated = u8(24 * m, 0xEE), i32(m), i32(m), i32(m), i32(m), i32(m + 1)
        d_ctr2 = torch.zeros(m, dtype=torch.int64, device="cuda")
        stream.synchronize()

        def send(job):
            """route-dst -> send-gate -> send-assign -> seal -> sent, on A"""
            router.route_dst_batch(dev, job.d_arena, job.d_sizes, A["image"], job.d_peer, stride=SLOT, offset=16, stream=stream,
                                   n=job.m)
            rekey.send_gate_batch(dev, job.d_peer, job.d_count, job.d_status_in, job.m, NOW, A["rows"], A["kp"], A["nonce"],
                                  REJECT_AFTER_MESSAGES, A["rekey"], job.d_status, stream=stream, n_jobs=1, n_ids=n_ids,
                                  n_peers=n_peers, n_keys=n_keys)
            job.enqueue(dev, A["peer_keys"], len(a_peer_keys), A["nonce"], A["keys"], n_keys, d_work, stream)
            rekey.sent_batch(dev, job.d_peer, job.d_count, job.d_status, job.d_job_key, job.m, NOW, A["rows"], A["kp"],
                             A["nonce"], REJECT_AFTER_MESSAGES, A["rekey"], stream=stream, n_jobs=1, n_ids=n_ids,
                             n_peers=n_peers, n_keys=n_keys)

        # A: the job is refused, the wish becomes a descriptor, the descriptor a message
        send(before)
        rekey.start_batch(dev, NOW, A["rekey"], A["hs_peers"], A["tickets"], d_start, d_start_peer, d_count, d_start_status,
                          d_reasons, d_work, stream=stream, n_peers=n_peers, n_tickets=1)
        noise.initiate_batch(dev, d_start, A["pub"], A["table"], d_states, d_init_msgs, d_init_status, n_keys, stream=stream,
                             n=1, n_peers=n_peers, n_states=1)
        # B: classify -> screen -> consume -> accept -> respond -> responded -> begin-responder
        d_arena_b1[:148].copy_(d_init_msgs[:148])
        router.classify_batch(dev, d_arena_b1, d_size_b1, B["slots"], d_pkts_b1, d_type_b1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(b_slots))
        cookie.screen_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, B["checker"], None, d_screen_b1, under_load=False,
                            stream=stream, n=1)
        noise.consume_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, d_screen_b1, B["self"], B["table"], d_consumed, d_hs_init,
                            stream=stream, n=1, n_peers=n_peers)
        noise.accept_batch(dev, d_hs_init, d_consumed, NOW, B["table"], B["rows"], B["hs_peers"], B["tickets"], d_resp, d_n_resp,
                           d_accept, stream=stream, n=1, n_ids=n_ids, n_peers=n_peers, n_tickets=1)
        noise.respond_batch(dev, d_resp, d_hs_init, None, B["table"], None, B["keys"], d_resp_msgs, d_resp_status, stream=stream,
                            n=1, n_init=1, n_peers=n_peers, n_keys=n_keys)
        rekey.responded_batch(dev, d_resp, d_resp_status, NOW, B["rekey"], stream=stream, n=1, n_peers=n_peers)
        keypairs.begin_responder_batch(dev, d_resp, d_resp_status, NOW, B["table"], B["kp"], B["slots"], B["peer_keys"],
                                       B["keys"], B["key_peer"], d_begun_b, d_work, stream=stream, n=1, n_peers=n_peers,
                                       n_slots=len(b_slots), n_peer_slots=len(b_peer_keys), n_keys=n_keys)
        # A: classify -> finish -> begin-initiator
        d_arena_a1[:92].copy_(d_resp_msgs[:92])
        router.classify_batch(dev, d_arena_a1, d_size_a1, A["slots"], d_pkts_a1, d_type_a1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(a_slots))
        noise.finish_batch(dev, d_arena_a1, d_pkts_a1, d_type_a1, None, A["self"], A["hs_slots"], d_states, None, A["keys"],
                           d_fwork, d_finished, stream=stream, n=1, n_slots=len(a_hs_slots), n_states=1, n_peers=n_peers,
                           n_keys=n_keys)
        keypairs.begin_initiator_batch(dev, d_arena_a1, d_pkts_a1, d_finished, NOW, A["hs_slots"], d_states, A["table"], A["kp"],
                                       A["slots"], A["peer_keys"], A["keys"], A["key_peer"], d_begun_a, d_work, stream=stream,
                                       n=1, n_hs_slots=len(a_hs_slots), n_states=1, n_peers=n_peers, n_slots=len(a_slots),
                                       n_peer_slots=len(a_peer_keys), n_keys=n_keys)
        # A: the same job again
        send(after)
        # B: classify -> recv-gate -> open -> replay -> received -> source
        for k in range(2):
            o = int(off2[k])
            d_arena2[o:o + wire_len[k]].copy_(after.d_arena[k * SLOT:k * SLOT + wire_len[k]])
        router.classify_batch(dev, d_arena2, d_size2, B["slots"], d_pkts2, d_type2, off=d_off2, stream=stream, n=m,
                              n_slots=len(b_slots))
        rekey.recv_gate_batch(dev, d_pkts2, NOW, B["key_peer"], B["rows"], B["kp"], stream=stream, n=m, n_keys=n_keys,
                              n_ids=n_ids, n_peers=n_peers)
        transport.open_batch(dev, d_arena2, d_pkts2, B["keys"], d_len2, d_ctr2, stream=stream, n=m, n_keys=n_keys)
        keystate.replay_batch(dev, d_pkts2, d_len2, d_ctr2, B["filters"], d_verdict2, d_work, stream=stream, n=m, n_keys=n_keys)
        keypairs.received_batch(dev, d_pkts2, d_verdict2, B["key_peer"], B["rows"], B["kp"], B["slots"], B["peer_keys"],
                                B["keys"], d_rotated, stream=stream, n=m, n_keys=n_keys, n_ids=n_ids, n_peers=n_peers,
                                n_slots=len(b_slots), n_peer_slots=len(b_peer_keys))
        router.source_batch(dev, d_arena2, d_pkts2, d_verdict2, B["key_peer"], B["image"], d_verdict2, peer=d_found,
                            stream=stream, n=m, n_keys=n_keys)
        stream.synchronize()  # the only one since the chains began

    # A, first pass: refused at the gate, so nothing was assigned or sealed, and a handshake was started
    assert before.d_peer.cpu().numpy().view(np.uint32).tolist() == [b_at_a] * 2
    assert before.d_status.cpu().tolist() == [ERR_KEY_EXPIRED, MARK]
    assert before.d_nbufs.item() == 0 and before.d_out_len.cpu().tolist() == [ERR_INVALID_ARG] * 2
    assert before.d_arena.cpu().numpy().tobytes() == before.arena.tobytes()
    assert d_start_status.cpu().tolist() == h_status.tolist() + [MARK] and h_status[a_pr] == HS_STARTED
    assert d_reasons.cpu().numpy()[a_pr] == WANT_REJECT_TIME and d_count.cpu().tolist() == [1, MARK]
    assert d_start_peer.cpu().tolist() == [a_pr, MARK] and d_start.cpu().numpy().tobytes() == h_start.tobytes()
    assert d_init_status.cpu().tolist() == [noise.HS_INITIATED]
    # B: the handshake
    assert d_type_b1.cpu().tolist() == [1] and d_accept.cpu().tolist() == [noise.HS_ACCEPTED]
    assert d_resp_status.cpu().tolist() == [HS_RESPONDED] and d_begun_b.cpu().tolist() == [HS_BEGUN, MARK]
    # A: the response
    assert d_type_a1.cpu().tolist() == [2] and d_finished.cpu().tolist() == [HS_FINISHED]
    assert d_begun_a.cpu().tolist() == [HS_BEGUN, MARK]
    got_a_kp = A["kp"].cpu().numpy().view(KEYPAIRS_DTYPE)
    assert tuple(got_a_kp["current"][a_pr]) == (2, 3, a_new_index, SET | INITIATOR, NOW)
    assert tuple(got_a_kp["previous"][a_pr]) == (0, 1, a_old_index, SET | INITIATOR, created)
    # A, second pass: the gate lets the job through and it is sealed under the new key
    assert after.d_status.cpu().tolist() == [0, MARK] and after.d_nbufs.item() == 2
    assert after.d_job_key.cpu().numpy().view(np.uint32)[0] == 2 and after.d_out_len.cpu().tolist() == wire_len
    # B: the plaintext arrives; the old keypair's packet is turned away untouched
    pk2 = d_pkts2.cpu().numpy().view(AEAD_PKT_DTYPE)
    assert d_type2.cpu().tolist() == [4, 4, 4] and pk2["key"].tolist() == [3, 3, SESSION_EXPIRED]
    assert d_len2.cpu().tolist() == LENGTHS + [ERR_INVALID_ARG] and d_verdict2.cpu().tolist() == LENGTHS + [ERR_INVALID_ARG]
    got2 = d_arena2.cpu().numpy()
    for k, p in enumerate(after.packets):
        o = int(off2[k]) + 16
        assert got2[o:o + len(p)].tobytes() == p, f"packet {k} did not arrive"
    o = int(off2[2])
    assert got2[o:o + len(old_wire)].tobytes() == old_wire, "the expired keypair's message is untouched"
    assert got2[o + len(old_wire):].tobytes() == arena2[o + len(old_wire):].tobytes()
    assert d_rotated.cpu().tolist() == [1, 0, 0, MARK] and d_found.cpu().numpy().view(np.uint32)[:2].tolist() == [a_at_b] * 2
    got_b_kp = B["kp"].cpu().numpy().view(KEYPAIRS_DTYPE)
    assert tuple(got_b_kp["current"][b_pr]) == (2, 3, b_new_index, SET, NOW) and got_b_kp["next"][b_pr]["flags"] == 0
    # the wgcs_rekey tables are what the host forms say: nothing wanted, lastSentHandshake at the call's clock
    got_a, got_b = A["rekey"].cpu().numpy().view(REKEY_DTYPE), B["rekey"].cpu().numpy().view(REKEY_DTYPE)
    assert got_a.tobytes() == want_a.tobytes() and got_b.tobytes() == want_b.tobytes()
    assert not got_a["want"].any() and not got_b["want"].any()
    assert got_a["last_sent_ns"][a_pr] == NOW and got_b["last_sent_ns"][b_pr] == NOW
    assert (np.delete(got_a["last_sent_ns"], a_pr) == NOW - 6 * SECOND).all()
