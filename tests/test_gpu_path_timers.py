"""A lost initiation is noticed and retried on the device, and the session it
leads to starts with a keepalive: both endpoints' chains enqueued on one stream
with a single synchronise at the end, the clock only an argument.

A has no keypair for B.  Its send job is refused by the send gate, start and
initiate build a message, timers_initiated arms resendHandshake -- and the
message is dropped.  An expire call one nanosecond before the deadline does
nothing; the one at the deadline counts the attempt and asks for a retry, which
start and initiate carry out with the second ticket.  B consumes, accepts,
responds and installs its next keypair; A finishes and installs its current
one, and timers_finished owes a keepalive, which the expire call at the same
clock emits as a job that the send chain seals.  B's receive chain opens it,
promotes its next keypair on it and leaves a keepalive-only write group.
Every wgcs_timers and wgcs_rekey table is compared with the same chain through
the host forms.  The worlds are built with the helpers of
tests/test_gpu_path_keypairs.py."""
import numpy as np
import pytest
import torch

import cookie_ref
import noise_accept_cases as accept_cases
from keypairs_ref import HS_BEGUN, INITIATOR, NO_KEYPAIR, PEER_NONE, SET
from path_ref import RECV_SENTINEL
from rekey_ref import ERR_KEY_EXPIRED, HS_STARTED, SECOND, WANT_NO_KEYPAIR
from test_gpu_path_keypairs import MARK, MTU, SLOT, SendJob, i32, u8, up
from timers_ref import (ACT_KEEPALIVE, ACTIVE, CLEAR_SRC, HS_FINISHED, HS_INITIATED, HS_RESPONDED, LAST_MINUTE, WANT_RETRY,
                        fired)
from wireguard_amd import cookie, keypairs, keystate, noise, rekey, router, timers, transport, writeplan
from wireguard_amd._lib import REJECT_AFTER_MESSAGES
from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.noise import HS_RESP_DTYPE, HS_START_DTYPE, HS_STATE_DTYPE
from wireguard_amd.rekey import REKEY_DTYPE
from wireguard_amd.timers import TIMERS_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE
from wireguard_amd.tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

pytestmark = pytest.mark.gpu

NOW = accept_cases.NOW
SEED = 0xA11CE
LIMIT = REJECT_AFTER_MESSAGES


def test_a_lost_initiation_is_retried_and_the_session_opens_with_a_keepalive(dev):
    rng = np.random.default_rng(2001)
    a_private, b_private = rng.bytes(32), rng.bytes(32)
    a_self, a_public = noise.responder_init(a_private)
    b_self, b_public = noise.responder_init(b_private)
    others = [noise.responder_init(rng.bytes(32))[1] for _ in range(3)]
    b_at_a, a_at_b, n_ids = 71, 52, 80  # the peer ids each side knows the other by
    a_table = noise.peer_keys_build(a_self, [b_public] + others, [b_at_a, 72, 73, 74])
    b_table = noise.peer_keys_build(b_self, [a_public] + others, [a_at_b, 53, 54, 55])
    n_peers, n_keys = 4, 4
    a_pr, b_pr = noise.peer_keys_find(a_table, b_public), noise.peer_keys_find(b_table, a_public)
    a_rows, b_rows = noise.peer_rows_build(a_table, n_ids), noise.peer_rows_build(b_table, n_ids)
    a_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    b_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    a_kp, b_kp = keypairs.keypairs_table(n_peers), keypairs.keypairs_table(n_peers)  # nobody has a keypair
    a_key_peer, b_key_peer = np.full(n_keys, PEER_NONE, np.uint32), np.full(n_keys, PEER_NONE, np.uint32)
    # what the hosts prepared: A two tickets (one per attempt), B one; their indices registered without a keypair
    a_index = [0x0C0FFEE0, 0x0C0FFEE1]
    a_tickets = np.zeros(2, HS_START_DTYPE)
    for k in range(2):
        a_tickets[k] = (k, 0xEEEEEEEE, a_index[k], 2 * k, 2 * k + 1, 0xEEEEEEEE, np.frombuffer(accept_cases.T[2 + k], np.uint8),
                        0xEE, np.frombuffer(rng.bytes(32), np.uint8), 0xEE, 0xEE)
    b_tickets = accept_cases.tickets_of(1, seed=2002)
    b_tickets["send_key"], b_tickets["recv_key"] = 2, 3
    b_index = int(b_tickets["local_index"][0])
    a_slots = router.session_table(np.array(a_index, np.uint32), np.full(2, NO_KEYPAIR, np.uint32))
    b_slots = router.session_table(np.array([b_index], np.uint32), np.array([NO_KEYPAIR], np.uint32))
    a_hs_slots = router.session_table(np.array(a_index, np.uint32), np.array([0, 1], np.uint32))
    a_peer_keys = router.session_table(a_table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
    b_peer_keys = router.session_table(b_table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
    a_hs_peers, b_hs_peers = accept_cases.peers_of(n_peers, seed=2003), accept_cases.peers_of(n_peers, seed=2004)
    a_hs_peers["flags"], b_hs_peers["flags"] = 0, 0
    a_rekey, b_rekey = rekey.rekey_table(n_peers, NOW), rekey.rekey_table(n_peers, NOW)
    a_rekey["flags"][a_pr] = LAST_MINUTE  # left over from the session before: timersHandshakeComplete clears it
    a_timers, b_timers = timers.timers_table(n_peers), timers.timers_table(n_peers, 25)
    b_checker = np.frombuffer(cookie_ref.Checker(b_public).tobytes(), cookie.COOKIE_CHECKER_DTYPE)
    ra = router.Router()
    ra.insert(bytes([10, 1, 2, 0]), 24, b_at_a)  # A routes the job's destination to B
    a_image = ra.image()
    deadline = NOW + 5 * SECOND + timers.jitter_ms(SEED, a_pr) * 1_000_000  # resendHandshake's, after the first attempt
    m = 1  # B's transport batch: the keepalive
    off2, size2 = np.array([5], np.uint64), np.array([32], np.int32)
    arena2 = np.full(m * SLOT + 8, RECV_SENTINEL, np.uint8)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        A = {k: up(v) for k, v in dict(table=a_table, rows=a_rows, kp=a_kp, keys=a_keys, key_peer=a_key_peer, slots=a_slots,
                                       hs_slots=a_hs_slots, peer_keys=a_peer_keys, hs_peers=a_hs_peers, rekey=a_rekey,
                                       timers=a_timers, tickets=a_tickets, self=a_self, pub=np.frombuffer(a_public, np.uint8),
                                       image=a_image, nonce=np.zeros(n_keys, np.uint64)).items()}
        B = {k: up(v) for k, v in dict(table=b_table, rows=b_rows, kp=b_kp, keys=b_keys, key_peer=b_key_peer, slots=b_slots,
                                       peer_keys=b_peer_keys, hs_peers=b_hs_peers, rekey=b_rekey, timers=b_timers,
                                       tickets=b_tickets, self=b_self, checker=b_checker,
                                       filters=np.zeros(n_keys, REPLAY_FILTER_DTYPE)).items()}
        job = SendJob(np.random.default_rng(7), b_at_a, [40, 72])
        job.d_peer = i32(2)  # route-dst finds it
        job.d_status_in, job.d_status = job.d_status, i32(1 + 1)
        d_work = torch.zeros(keystate.work_bytes(8), dtype=torch.uint8, device="cuda")
        d_fwork = u8(noise.FINISH_WORK_BYTES)
        d_states = u8(2 * 128)
        # one set of start / initiate buffers per attempt, and one set of expire outputs per call
        att = [dict(start=u8(96), start_peer=i32(1 + 1), count=i32(1 + 1), status=i32(n_peers + 1), reasons=i32(n_peers + 1),
                    msgs=u8(160), init_status=i32(1)) for _ in range(2)]
        exp = [dict(ka_peer=i32(1 + 1), ka_count=i32(1 + 1), ka_sizes=i32(1 + 1), ka_status=i32(1 + 1), n_ka=i32(1 + 1),
                    actions=i32(n_peers + 1)) for _ in range(3)]
        # B's handshake batch (one message) and A's (one message)
        d_arena_b1, d_size_b1 = u8(SLOT, RECV_SENTINEL), up(np.array([148], np.int32))
        d_pkts_b1, d_type_b1, d_screen_b1, d_consumed, d_accept = u8(24, 0xEE), i32(1), i32(1), i32(1), i32(1)
        d_hs_init, d_resp, d_n_resp, d_resp_msgs, d_resp_status, d_begun_b = u8(128, 0xEE), u8(80), i32(1), u8(96), i32(1), i32(1 + 1)
        d_arena_a1, d_size_a1 = u8(SLOT, RECV_SENTINEL), up(np.array([92], np.int32))
        d_pkts_a1, d_type_a1, d_finished, d_begun_a = u8(24, 0xEE), i32(1), i32(1), i32(1 + 1)
        # A's keepalive job and B's transport batch
        d_ka_arena, d_ka_gate, d_ka_pkts, d_ka_nbufs, d_ka_key, d_ka_len = u8(SLOT + 64), i32(1 + 1), u8(24, 0xEE), i32(1), i32(1), i32(1)
        d_arena2, d_off2, d_size2 = up(arena2), up(off2), up(size2)
        d_pkts2, d_type2, d_len2, d_verdict2, d_rotated = u8(24 * m, 0xEE), i32(m), i32(m), i32(m), i32(m + 1)
        d_ctr2 = torch.zeros(m, dtype=torch.int64, device="cuda")
        d_bufs, d_calls, d_groups = (u8(dt.itemsize * m) for dt in (GRO_BUF_DTYPE, GRO_CALL_DTYPE, WRITE_GROUP_DTYPE))
        d_n_groups, d_wstatus = i32(1), i32(1)
        stream.synchronize()

        def expire(now, o):
            timers.expire_batch(dev, now, A["timers"], A["rekey"], A["table"], None, A["kp"], A["slots"], A["peer_keys"],
                                A["keys"], A["key_peer"], o["ka_peer"], o["ka_count"], o["ka_sizes"], o["ka_status"], o["n_ka"],
                                o["actions"], d_work, stream=stream, n_peers=n_peers, n_slots=len(a_slots),
                                n_peer_slots=len(a_peer_keys), n_keys=n_keys, n_ka_max=1)

        def attempt(now, o, ticket):
            """start -> initiate -> timers_initiated, on A"""
            rekey.start_batch(dev, now, A["rekey"], A["hs_peers"], A["tickets"][96 * ticket:96 * ticket + 96], o["start"],
                              o["start_peer"], o["count"], o["status"], o["reasons"], d_work, stream=stream, n_peers=n_peers,
                              n_tickets=1)
            noise.initiate_batch(dev, o["start"], A["pub"], A["table"], d_states, o["msgs"], o["init_status"], n_keys,
                                 stream=stream, n=1, n_peers=n_peers, n_states=2)
            timers.initiated_batch(dev, o["reasons"], o["start_peer"], o["init_status"], now, SEED, A["timers"], stream=stream,
                                   n_tickets=1, n_peers=n_peers)

        # 1. A has no keypair: the job is refused, the wish becomes a message -- which is dropped
        router.route_dst_batch(dev, job.d_arena, job.d_sizes, A["image"], job.d_peer, stride=SLOT, offset=16, stream=stream,
                               n=job.m)
        rekey.send_gate_batch(dev, job.d_peer, job.d_count, job.d_status_in, job.m, NOW, A["rows"], A["kp"], A["nonce"], LIMIT,
                              A["rekey"], job.d_status, stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
        attempt(NOW, att[0], 0)
        # 2., 3. nothing a nanosecond early; at the deadline the attempt is counted and a retry asked for
        expire(deadline - 1, exp[0])
        expire(deadline, exp[1])
        # 4. the retry, with the second ticket
        now = deadline
        attempt(now, att[1], 1)
        # 5. B: classify -> screen -> consume -> accept -> respond -> responded (rekey, timers) -> begin-responder
        d_arena_b1[:148].copy_(att[1]["msgs"][:148])
        router.classify_batch(dev, d_arena_b1, d_size_b1, B["slots"], d_pkts_b1, d_type_b1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(b_slots))
        cookie.screen_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, B["checker"], None, d_screen_b1, under_load=False,
                            stream=stream, n=1)
        noise.consume_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, d_screen_b1, B["self"], B["table"], d_consumed, d_hs_init,
                            stream=stream, n=1, n_peers=n_peers)
        noise.accept_batch(dev, d_hs_init, d_consumed, now, B["table"], B["rows"], B["hs_peers"], B["tickets"], d_resp, d_n_resp,
                           d_accept, stream=stream, n=1, n_ids=n_ids, n_peers=n_peers, n_tickets=1)
        noise.respond_batch(dev, d_resp, d_hs_init, None, B["table"], None, B["keys"], d_resp_msgs, d_resp_status, stream=stream,
                            n=1, n_init=1, n_peers=n_peers, n_keys=n_keys)
        rekey.responded_batch(dev, d_resp, d_resp_status, now, B["rekey"], stream=stream, n=1, n_peers=n_peers)
        timers.responded_batch(dev, d_resp, d_resp_status, now, B["timers"], stream=stream, n=1, n_peers=n_peers)
        keypairs.begin_responder_batch(dev, d_resp, d_resp_status, now, B["table"], B["kp"], B["slots"], B["peer_keys"],
                                       B["keys"], B["key_peer"], d_begun_b, d_work, stream=stream, n=1, n_peers=n_peers,
                                       n_slots=len(b_slots), n_peer_slots=len(b_peer_keys), n_keys=n_keys)
        # 6. A: classify -> finish -> begin-initiator -> timers_finished
        d_arena_a1[:92].copy_(d_resp_msgs[:92])
        router.classify_batch(dev, d_arena_a1, d_size_a1, A["slots"], d_pkts_a1, d_type_a1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(a_slots))
        noise.finish_batch(dev, d_arena_a1, d_pkts_a1, d_type_a1, None, A["self"], A["hs_slots"], d_states, None, A["keys"],
                           d_fwork, d_finished, stream=stream, n=1, n_slots=len(a_hs_slots), n_states=2, n_peers=n_peers,
                           n_keys=n_keys)
        keypairs.begin_initiator_batch(dev, d_arena_a1, d_pkts_a1, d_finished, now, A["hs_slots"], d_states, A["table"], A["kp"],
                                       A["slots"], A["peer_keys"], A["keys"], A["key_peer"], d_begun_a, d_work, stream=stream,
                                       n=1, n_hs_slots=len(a_hs_slots), n_states=2, n_peers=n_peers, n_slots=len(a_slots),
                                       n_peer_slots=len(a_peer_keys), n_keys=n_keys)
        timers.finished_batch(dev, d_arena_a1, d_pkts_a1, d_finished, d_begun_a, now, A["hs_slots"], d_states, A["timers"],
                              A["rekey"], stream=stream, n=1, n_hs_slots=len(a_hs_slots), n_states=2, n_peers=n_peers)
        # 7. A: the expire call at the same clock emits the keepalive; send-gate -> send-assign -> seal -> sent
        ka = exp[2]
        expire(now, ka)
        rekey.send_gate_batch(dev, ka["ka_peer"], ka["ka_count"], ka["ka_status"], 1, now, A["rows"], A["kp"], A["nonce"], LIMIT,
                              A["rekey"], d_ka_gate, stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
        keystate.send_assign_batch(dev, ka["ka_sizes"], ka["ka_peer"], ka["ka_count"], d_ka_gate, 1, SLOT, A["peer_keys"],
                                   A["nonce"], d_ka_pkts, d_ka_nbufs, d_ka_key, d_work, stream=stream, n_jobs=1,
                                   n_slots=len(a_peer_keys), n_keys=n_keys)
        transport.seal_batch(dev, d_ka_arena, d_ka_pkts, A["keys"], MTU, d_ka_len, stream=stream, n=1, n_keys=n_keys)
        rekey.sent_batch(dev, ka["ka_peer"], ka["ka_count"], d_ka_gate, d_ka_key, 1, now, A["rows"], A["kp"], A["nonce"], LIMIT,
                         A["rekey"], stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
        timers.sent_batch(dev, ka["ka_sizes"], ka["ka_peer"], ka["ka_count"], d_ka_gate, d_ka_key, 1, now, SEED, A["rows"],
                          A["timers"], stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers)
        # 8. B: classify -> recv-gate -> open -> replay -> received -> rotated -> write-build -> received (rekey, timers)
        d_arena2[5:5 + 32].copy_(d_ka_arena[:32])
        router.classify_batch(dev, d_arena2, d_size2, B["slots"], d_pkts2, d_type2, off=d_off2, stream=stream, n=m,
                              n_slots=len(b_slots))
        rekey.recv_gate_batch(dev, d_pkts2, now, B["key_peer"], B["rows"], B["kp"], stream=stream, n=m, n_keys=n_keys,
                              n_ids=n_ids, n_peers=n_peers)
        transport.open_batch(dev, d_arena2, d_pkts2, B["keys"], d_len2, d_ctr2, stream=stream, n=m, n_keys=n_keys)
        keystate.replay_batch(dev, d_pkts2, d_len2, d_ctr2, B["filters"], d_verdict2, d_work, stream=stream, n=m, n_keys=n_keys)
        keypairs.received_batch(dev, d_pkts2, d_verdict2, B["key_peer"], B["rows"], B["kp"], B["slots"], B["peer_keys"],
                                B["keys"], d_rotated, stream=stream, n=m, n_keys=n_keys, n_ids=n_ids, n_peers=n_peers,
                                n_slots=len(b_slots), n_peer_slots=len(b_peer_keys))
        timers.rotated_batch(dev, d_pkts2, d_rotated, now, B["key_peer"], B["rows"], B["timers"], B["rekey"], stream=stream,
                             n=m, n_keys=n_keys, n_ids=n_ids, n_peers=n_peers)
        writeplan.write_build_batch(dev, d_pkts2, d_verdict2, m, B["key_peer"], 16, SLOT, 1, d_bufs, d_calls, d_groups,
                                    d_n_groups, d_wstatus, stream=stream, n_batches=1, n_keys=n_keys)
        rekey.received_batch(dev, d_groups, 1, now, B["rows"], B["kp"], B["rekey"], stream=stream, n_batches=1, n_ids=n_ids,
                             n_peers=n_peers)
        timers.received_batch(dev, d_groups, 1, now, B["rows"], B["timers"], stream=stream, n_batches=1, n_ids=n_ids,
                              n_peers=n_peers)
        stream.synchronize()  # the only one since the chains began

    down = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    # 1.: refused at the gate, started, initiated
    assert job.d_status.cpu().tolist() == [ERR_KEY_EXPIRED, MARK] and job.d_peer.cpu().numpy().view(np.uint32).tolist() == [b_at_a] * 2
    for k, why in enumerate((WANT_NO_KEYPAIR, WANT_RETRY)):
        o = att[k]
        assert o["status"].cpu().tolist()[a_pr] == HS_STARTED and o["count"].cpu().tolist() == [1, MARK]
        assert o["start_peer"].cpu().tolist() == [a_pr, MARK] and o["init_status"].cpu().tolist() == [HS_INITIATED]
        assert down(o["reasons"], np.uint32)[a_pr] == why and down(o["start"], HS_START_DTYPE)["local_index"][0] == a_index[k]
    # 2., 3.: one nanosecond decides
    assert exp[0]["actions"].cpu().tolist() == [0] * n_peers + [MARK] and exp[0]["n_ka"].cpu().tolist() == [0, MARK]
    assert down(exp[0]["ka_peer"], np.uint32).tolist() == [PEER_NONE, MARK]
    assert down(exp[1]["actions"], np.uint32)[a_pr] == fired(1) and exp[1]["n_ka"].cpu().tolist() == [0, MARK]
    # 5., 6.: the handshake
    assert d_type_b1.cpu().tolist() == [1] and d_accept.cpu().tolist() == [noise.HS_ACCEPTED]
    assert d_resp_status.cpu().tolist() == [HS_RESPONDED] and d_begun_b.cpu().tolist() == [HS_BEGUN, MARK]
    assert d_type_a1.cpu().tolist() == [2] and d_finished.cpu().tolist() == [HS_FINISHED]
    assert d_begun_a.cpu().tolist() == [HS_BEGUN, MARK]
    got_a_kp, got_b_kp = down(A["kp"], KEYPAIRS_DTYPE), down(B["kp"], KEYPAIRS_DTYPE)
    assert tuple(got_a_kp["current"][a_pr]) == (2, 3, a_index[1], SET | INITIATOR, deadline)
    # 7.: one keepalive job, sealed under the new key
    assert down(ka["ka_peer"], np.uint32).tolist() == [b_at_a, MARK] and ka["ka_count"].cpu().tolist() == [1, MARK]
    assert ka["ka_sizes"].cpu().tolist() == [0, MARK] and ka["ka_status"].cpu().tolist() == [0, MARK]
    assert ka["n_ka"].cpu().tolist() == [1, MARK] and down(ka["actions"], np.uint32)[a_pr] == ACT_KEEPALIVE
    assert d_ka_gate.cpu().tolist() == [0, MARK] and d_ka_nbufs.item() == 1 and down(d_ka_key, np.uint32)[0] == 2
    assert d_ka_len.cpu().tolist() == [32]
    # 8.: B opens it, promotes its next keypair on it, and its write group is a keepalive-only group
    assert d_type2.cpu().tolist() == [4] and down(d_pkts2, AEAD_PKT_DTYPE)["key"].tolist() == [3]
    assert d_len2.cpu().tolist() == [0] and d_verdict2.cpu().tolist() == [0] and d_rotated.cpu().tolist() == [1, MARK]
    b_index_kp = (2, 3, b_index, SET, deadline)
    assert tuple(got_b_kp["current"][b_pr]) == b_index_kp and got_b_kp["next"][b_pr]["flags"] == 0
    groups = down(d_groups, WRITE_GROUP_DTYPE)
    assert d_n_groups.cpu().tolist() == [1] and d_wstatus.cpu().tolist() == [0]
    assert (groups["peer"][0], groups["tail"][0], groups["flags"][0], groups["n_valid"][0]) == (a_at_b, 0, 0, 1)
    assert groups["rx_bytes"][0] == 32

    # the same chain through the host forms, over the rows the device calls left for each other
    tm_a, rk_a, tm_b, rk_b = a_timers.copy(), a_rekey.copy(), b_timers.copy(), b_rekey.copy()
    nonce0 = np.zeros(n_keys, np.uint64)
    h = np.zeros(1, np.int32)
    rekey.send_gate_host(np.full(2, b_at_a, np.uint32), np.array([2], np.int32), np.zeros(1, np.int32), 2, NOW, a_rows, a_kp,
                         nonce0, LIMIT, rk_a, h)
    assert h.tolist() == [ERR_KEY_EXPIRED]
    tables = lambda: [x.copy() for x in (a_kp, a_slots, a_peer_keys, a_keys, a_key_peer)]  # noqa: E731

    def host_attempt(now, k):
        o = dict(start=np.zeros(1, HS_START_DTYPE), start_peer=np.zeros(1, np.uint32), count=np.zeros(1, np.uint32),
                 status=np.zeros(n_peers, np.int32), reasons=np.zeros(n_peers, np.uint32))
        rekey.start_host(now, rk_a, a_hs_peers, a_tickets[k:k + 1], o["start"], o["start_peer"], o["count"], o["status"],
                         o["reasons"])
        for name in ("start", "start_peer", "status", "reasons"):
            assert o[name].tobytes() == down(att[k][name], np.uint8)[:o[name].nbytes].tobytes(), (k, name)
        timers.initiated_host(o["reasons"], o["start_peer"], down(att[k]["init_status"], np.int32), now, SEED, tm_a)

    def host_expire(now, k):
        o = dict(ka_peer=np.zeros(1, np.uint32), ka_count=np.zeros(1, np.int32), ka_sizes=np.zeros(1, np.int32),
                 ka_status=np.zeros(1, np.int32), n_ka=np.zeros(1, np.uint32), actions=np.zeros(n_peers, np.uint32))
        timers.expire_host(now, tm_a, rk_a, a_table, None, *tables(), o["ka_peer"], o["ka_count"], o["ka_sizes"],
                           o["ka_status"], o["n_ka"], o["actions"])
        for name, x in o.items():
            assert x.tobytes() == down(exp[k][name], np.uint8)[:x.nbytes].tobytes(), (k, name)

    host_attempt(NOW, 0)
    assert tm_a["deadline_ns"][a_pr, 1] == deadline and tm_a["pending"][a_pr] == 0b00010
    host_expire(deadline - 1, 0)
    host_expire(deadline, 1)
    assert tm_a["attempts"][a_pr] == 1 and rk_a["want"][a_pr] == WANT_RETRY and tm_a["flags"][a_pr] == ACTIVE | CLEAR_SRC
    host_attempt(deadline, 1)
    h_resp, h_gate = down(d_resp, HS_RESP_DTYPE), down(d_resp_status, np.int32)
    rekey.responded_host(h_resp, h_gate, deadline, rk_b)
    timers.responded_host(h_resp, h_gate, deadline, tm_b)
    timers.finished_host(down(d_arena_a1, np.uint8), down(d_pkts_a1, AEAD_PKT_DTYPE), down(d_finished, np.int32),
                         down(d_begun_a, np.int32)[:1], deadline, a_hs_slots, down(d_states, HS_STATE_DTYPE), tm_a, rk_a)
    host_expire(deadline, 2)
    ka_h = [down(ka[k], dt)[:1].copy() for k, dt in (("ka_sizes", np.int32), ("ka_peer", np.uint32), ("ka_count", np.int32))]
    gate_h, key_h = down(d_ka_gate, np.int32)[:1].copy(), down(d_ka_key, np.uint32)[:1].copy()
    nonce1 = down(A["nonce"], np.uint64).copy()
    rekey.sent_host(ka_h[1], ka_h[2], gate_h, key_h, 1, deadline, a_rows, got_a_kp, nonce1, LIMIT, rk_a)
    timers.sent_host(ka_h[0], ka_h[1], ka_h[2], gate_h, key_h, 1, deadline, SEED, a_rows, tm_a)
    timers.rotated_host(down(d_pkts2, AEAD_PKT_DTYPE), down(d_rotated, np.uint32)[:m], deadline, down(B["key_peer"], np.uint32),
                        b_rows, tm_b, rk_b)
    rekey.received_host(groups, 1, deadline, b_rows, got_b_kp, rk_b)
    timers.received_host(groups, 1, deadline, b_rows, tm_b)
    got = {k: down(x[n], dt) for k, (x, n, dt) in dict(tm_a=(A, "timers", TIMERS_DTYPE), rk_a=(A, "rekey", REKEY_DTYPE),
                                                      tm_b=(B, "timers", TIMERS_DTYPE), rk_b=(B, "rekey", REKEY_DTYPE)).items()}
    for k, want in dict(tm_a=tm_a, rk_a=rk_a, tm_b=tm_b, rk_b=rk_b).items():
        assert got[k].tobytes() == want.tobytes(), (k, got[k], want)
    # the end state
    for t, row in ((got["tm_a"], a_pr), (got["tm_b"], b_pr)):
        assert t["attempts"][row] == 0 and not t["pending"][row] >> 1 & 1 and t["last_handshake_ns"][row] == deadline
    assert not got["rk_a"]["flags"].any() and not got["rk_a"]["want"].any() and not got["rk_b"]["want"].any()
    assert got["tm_a"]["flags"][a_pr] == ACTIVE | CLEAR_SRC and got["tm_a"]["pending"][a_pr] == 0b10000  # zeroOutKeys alone
    assert got["tm_b"]["pending"][b_pr] == 0b11000 and got["tm_b"]["deadline_ns"][b_pr, 3] == deadline + 25 * SECOND
    assert (np.delete(got["tm_a"]["pending"], a_pr) == 0).all() and (np.delete(got["tm_b"]["pending"], b_pr) == 0).all()
    assert d_arena2.cpu().numpy()[5 + 32:].tobytes() == arena2[5 + 32:].tobytes()
