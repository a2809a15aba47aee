"""The whole cookie round trip on the device: two endpoints' chains enqueued on
one stream with a single synchronise at the end, the clock only an argument.

1. A: start -> initiate -> timers_initiated -> cookie_initiated.
2. The initiation reaches B: split -> classify -> screen with under_load = 1.
   It carries no MAC2: WGCS_HS_COOKIE, and a reply is written.
3. The reply reaches A: split -> classify -> cookie_consume: WGCS_HS_COOKIE_KEPT.
4. A: cookie_age (nothing cleared) -> timers expire at resendHandshake's deadline
   -> start -> initiate.  The second initiation carries the MAC2 the reference
   would write.
5. B: split -> classify -> screen under load passes it -> cookie_consume (not
   its row) -> consume -> accept -> respond -> cookie_responded.
6. A: split -> classify -> finish.
7. A: cookie_age at exactly 120 s after the reply keeps the cookie; one
   nanosecond later it clears the bit, and the initiation that timers expire,
   start and initiate build then has a zero MAC2.
A message crosses from one role to the other by a copy on the stream into the
other's landing buffer.  Every expectation is computed by the host forms and
the restatements over the same inputs; state, key and generator tables are
compared whole."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cookie_ref
import noise_accept_cases as accept_cases
from keypairs_ref import NO_KEYPAIR, PEER_NONE
from rekey_ref import HS_STARTED, SECOND, WANT_NO_KEYPAIR
from test_gpu_cookie import src_row
from test_gpu_path_keypairs import SLOT, i32, u8, up
from timers_ref import HS_FINISHED, HS_INITIATED, HS_RESPONDED, WANT_RETRY
from wireguard_amd import cookie, cookiegen as cg, keypairs, keystate, noise, rekey, router, timers
from wireguard_amd._lib import HS_ACCEPTED, HS_CONSUMED, HS_COOKIE, HS_COOKIE_KEPT, HS_NONE, HS_PASS, HS_PEER_COOKIE
from wireguard_amd.noise import HS_INIT_DTYPE, HS_PEER_DTYPE, HS_RESP_DTYPE, HS_START_DTYPE, HS_STATE_DTYPE
from wireguard_amd.rekey import REKEY_DTYPE
from wireguard_amd.timers import TIMERS_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

NOW = accept_cases.NOW
SEED = 0xC00C1E
REFRESH = cg.COOKIE_REFRESH_NS
N = 2  # message slots of a recvmmsg batch: slot 1 is the landing buffer, the split moves its packet to slot 0


def test_cookie_round_trip_on_one_stream(dev):
    rng = np.random.default_rng(2210)
    a_private, b_private = rng.bytes(32), rng.bytes(32)
    a_self, a_public = noise.responder_init(a_private)
    b_self, b_public = noise.responder_init(b_private)
    others = [noise.responder_init(rng.bytes(32))[1] for _ in range(3)]
    n_ids, n_peers, n_keys = 80, 4, 6
    a_table = noise.peer_keys_build(a_self, others[:1] + [b_public] + others[1:], [72, 71, 73, 74])
    b_table = noise.peer_keys_build(b_self, others[:2] + [a_public] + others[2:], [53, 54, 52, 55])
    a_pr, b_pr = noise.peer_keys_find(a_table, b_public), noise.peer_keys_find(b_table, a_public)
    a_rows, b_rows = noise.peer_rows_build(a_table, n_ids), noise.peer_rows_build(b_table, n_ids)
    a_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    b_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    a_kp = keypairs.keypairs_table(n_peers)
    a_key_peer, b_key_peer = np.full(n_keys, PEER_NONE, np.uint32), np.full(n_keys, PEER_NONE, np.uint32)
    # what the hosts prepared: A three tickets (one per attempt), B one; their indices registered without a keypair
    a_index = [0x0C00C1E0, 0x0C00C1E1, 0x0C00C1E2]
    a_tickets = np.zeros(3, HS_START_DTYPE)
    for k in range(3):
        a_tickets[k] = (k, 0xEEEEEEEE, a_index[k], 2 * k, 2 * k + 1, 0xEEEEEEEE, np.frombuffer(accept_cases.T[1 + k], np.uint8),
                        0xEE, np.frombuffer(rng.bytes(32), np.uint8), 0xEE, 0xEE)
    b_tickets = accept_cases.tickets_of(1, seed=2211)
    b_tickets["send_key"], b_tickets["recv_key"] = 2, 3
    b_index = int(b_tickets["local_index"][0])
    a_slots = router.session_table(np.array(a_index, np.uint32), np.full(3, NO_KEYPAIR, np.uint32))
    b_slots = router.session_table(np.array([b_index], np.uint32), np.array([NO_KEYPAIR], np.uint32))
    a_hs_slots = router.session_table(np.array(a_index, np.uint32), np.array([0, 1, 2], np.uint32))
    a_peer_keys = router.session_table(a_table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
    a_hs_peers, b_hs_peers = accept_cases.peers_of(n_peers, seed=2212), accept_cases.peers_of(n_peers, seed=2213)
    a_hs_peers["flags"], b_hs_peers["flags"] = 0, 0  # nobody holds a cookie; the cookie bytes are junk no flag makes valid
    a_rekey = rekey.rekey_table(n_peers, NOW)
    a_rekey["want"][a_pr] = WANT_NO_KEYPAIR  # what a refused send job leaves
    a_timers = timers.timers_table(n_peers)
    a_gen, b_gen = cg.gen_build(a_table), cg.gen_build(b_table)
    a_states = np.full(3 * 128, 0xA5, np.uint8).view(HS_STATE_DTYPE)
    checker = cookie_ref.Checker(b_public, rng.bytes(32))  # B is under load and holds a secret
    a_src = cookie_ref.src_bytes(bytes([198, 51, 100, 7]), 51820)  # where B sees A's datagrams come from
    b_src_rows = np.concatenate([src_row(a_src)] * N)
    nonces = rng.bytes(24 * N)
    # the clock: the reply is kept a second after the first attempt; the retry comes at resendHandshake's deadline
    t_reply = NOW + SECOND
    t_retry = NOW + 5 * SECOND + timers.jitter_ms(SEED, a_pr) * 1_000_000
    t_kept, t_gone = t_reply + REFRESH, t_reply + REFRESH + 1

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        A = {k: up(v) for k, v in dict(table=a_table, rows=a_rows, kp=a_kp, keys=a_keys, key_peer=a_key_peer, slots=a_slots,
                                       hs_slots=a_hs_slots, peer_keys=a_peer_keys, hs_peers=a_hs_peers, rekey=a_rekey,
                                       timers=a_timers, tickets=a_tickets, self=a_self, pub=np.frombuffer(a_public, np.uint8),
                                       gen=a_gen, states=a_states).items()}
        B = {k: up(v) for k, v in dict(table=b_table, rows=b_rows, keys=b_keys, key_peer=b_key_peer, slots=b_slots,
                                       hs_peers=b_hs_peers, tickets=b_tickets, self=b_self, gen=b_gen,
                                       checker=np.frombuffer(checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE), src=b_src_rows,
                                       nonce=np.frombuffer(nonces, np.uint8)).items()}
        d_work = torch.zeros(keystate.work_bytes(8), dtype=torch.uint8, device="cuda")
        att = [dict(start=u8(96), start_peer=i32(1 + 1), count=i32(1 + 1), status=i32(n_peers + 1), reasons=i32(n_peers + 1),
                    msgs=u8(160), init_status=i32(1)) for _ in range(3)]
        exp = [dict(ka_peer=i32(1 + 1), ka_count=i32(1 + 1), ka_sizes=i32(1 + 1), ka_status=i32(1 + 1), n_ka=i32(1 + 1),
                    actions=i32(n_peers + 1)) for _ in range(2)]

        def landing(length):
            """One recvmmsg batch of N slots whose one datagram has `length` bytes, and what split and classify write."""
            return SimpleNamespace(land=u8(SLOT), n_in=up(np.array([0, length], np.int32)), gso=up(np.zeros(N, np.int32)),
                                   arena=u8(N * SLOT), n_out=i32(N), frm=i32(N), count=i32(1), status=i32(1),
                                   pkts=u8(24 * N, 0xEE), type=i32(N), length=length)

        def deliver(d_msg, t, slots, n_slots):
            """the datagram lands (a copy on the stream); split -> classify"""
            t.land[:t.length].copy_(d_msg[:t.length])
            rc = dev.lib.wgcs_split_messages_batch(dev.h, t.land.data_ptr(), SLOT, SLOT, t.n_in.data_ptr(), t.gso.data_ptr(),
                                                   N, 1, 1, t.arena.data_ptr(), SLOT, t.n_out.data_ptr(), t.frm.data_ptr(),
                                                   t.count.data_ptr(), t.status.data_ptr(), stream.cuda_stream)
            assert rc == 0
            router.classify_batch(dev, t.arena, t.n_out, slots, t.pkts, t.type, stride=SLOT, stream=stream, n=N,
                                  n_slots=n_slots)

        def attempt(now, o, k):
            """start -> initiate -> timers_initiated -> cookie_initiated, on A, with ticket k"""
            rekey.start_batch(dev, now, A["rekey"], A["hs_peers"], A["tickets"][96 * k:96 * k + 96], o["start"],
                              o["start_peer"], o["count"], o["status"], o["reasons"], d_work, stream=stream, n_peers=n_peers,
                              n_tickets=1)
            noise.initiate_batch(dev, o["start"], A["pub"], A["table"], A["states"], o["msgs"], o["init_status"], n_keys,
                                 stream=stream, n=1, n_peers=n_peers, n_states=3)
            timers.initiated_batch(dev, o["reasons"], o["start_peer"], o["init_status"], now, SEED, A["timers"], stream=stream,
                                   n_tickets=1, n_peers=n_peers)
            cg.initiated_batch(dev, o["start"], o["init_status"], o["msgs"], A["gen"], stream=stream, n=1, n_peers=n_peers)

        def expire(now, o):
            timers.expire_batch(dev, now, A["timers"], A["rekey"], A["table"], None, A["kp"], A["slots"], A["peer_keys"],
                                A["keys"], A["key_peer"], o["ka_peer"], o["ka_count"], o["ka_sizes"], o["ka_status"], o["n_ka"],
                                o["actions"], d_work, stream=stream, n_peers=n_peers, n_slots=len(a_slots),
                                n_peer_slots=len(a_peer_keys), n_keys=n_keys, n_ka_max=1)

        def a_consume(t, now, verdict, work):
            cg.consume_batch(dev, t.arena, t.pkts, t.type, now, A["hs_slots"], A["states"], A["slots"], A["key_peer"], A["rows"],
                             A["gen"], A["hs_peers"], work, verdict, stream=stream, n=N, n_hs_slots=len(a_hs_slots), n_states=3,
                             n_slots=len(a_slots), n_keys=n_keys, n_ids=n_ids, n_peers=n_peers)

        def b_screen(t, verdict, reply):
            cookie.screen_batch(dev, t.arena, t.pkts, t.type, B["checker"], B["src"], verdict, under_load=True, nonce=B["nonce"],
                                reply=reply, stream=stream, n=N)

        lb1, la1, lb2, la2 = landing(148), landing(64), landing(148), landing(92)
        d_screen1, d_reply1, d_screen2, d_reply2 = i32(N), u8(64 * N), i32(N), u8(64 * N)
        d_kept, d_cwork, d_b_cookie, d_b_cwork = i32(N), u8(16 * N, 0xEE), i32(N), u8(16 * N, 0xEE)
        d_consumed, d_accept, d_hs_init = i32(N), i32(N), u8(128 * N, 0xEE)
        d_resp, d_n_resp, d_resp_msgs, d_resp_status = u8(80), i32(1), u8(96), i32(1)
        d_finished, d_fwork = i32(N), u8(noise.FINISH_WORK_BYTES * N)
        stream.synchronize()

        # 1. A's first attempt: no cookie, MAC2 zero
        attempt(NOW, att[0], 0)
        # 2. B under load answers with a cookie reply
        deliver(att[0]["msgs"], lb1, B["slots"], len(b_slots))
        b_screen(lb1, d_screen1, d_reply1)
        # 3. A keeps the cookie
        deliver(d_reply1, la1, A["slots"], len(a_slots))
        a_consume(la1, t_reply, d_kept, d_cwork)
        # 4. nothing ages out; resendHandshake fires; the retry carries MAC2
        cg.age_batch(dev, t_retry, A["gen"], A["hs_peers"], stream=stream, n_peers=n_peers)
        expire(t_retry, exp[0])
        attempt(t_retry, att[1], 1)
        # 5. B passes it and responds
        deliver(att[1]["msgs"], lb2, B["slots"], len(b_slots))
        b_screen(lb2, d_screen2, d_reply2)
        cg.consume_batch(dev, lb2.arena, lb2.pkts, lb2.type, t_retry, None, None, B["slots"], B["key_peer"], B["rows"], B["gen"],
                         B["hs_peers"], d_b_cwork, d_b_cookie, stream=stream, n=N, n_hs_slots=0, n_states=0,
                         n_slots=len(b_slots), n_keys=n_keys, n_ids=n_ids, n_peers=n_peers)
        noise.consume_batch(dev, lb2.arena, lb2.pkts, lb2.type, d_screen2, B["self"], B["table"], d_consumed, d_hs_init,
                            stream=stream, n=N, n_peers=n_peers)
        noise.accept_batch(dev, d_hs_init, d_consumed, t_retry, B["table"], B["rows"], B["hs_peers"], B["tickets"], d_resp,
                           d_n_resp, d_accept, stream=stream, n=N, n_ids=n_ids, n_peers=n_peers, n_tickets=1)
        noise.respond_batch(dev, d_resp, d_hs_init, None, B["table"], None, B["keys"], d_resp_msgs, d_resp_status, stream=stream,
                            n=1, n_init=N, n_peers=n_peers, n_keys=n_keys)
        cg.responded_batch(dev, d_resp, d_resp_status, d_resp_msgs, B["gen"], stream=stream, n=1, n_peers=n_peers)
        # 6. A finishes
        deliver(d_resp_msgs, la2, A["slots"], len(a_slots))
        noise.finish_batch(dev, la2.arena, la2.pkts, la2.type, None, A["self"], A["hs_slots"], A["states"], None, A["keys"],
                           d_fwork, d_finished, stream=stream, n=N, n_slots=len(a_hs_slots), n_states=3, n_peers=n_peers,
                           n_keys=n_keys)
        # 7. exactly 120 s after the reply the cookie stays; a nanosecond later it goes, and the next MAC2 is zero
        cg.age_batch(dev, t_kept, A["gen"], A["hs_peers"], stream=stream, n_peers=n_peers)
        d_peers_kept = A["hs_peers"].clone()
        cg.age_batch(dev, t_gone, A["gen"], A["hs_peers"], stream=stream, n_peers=n_peers)
        expire(t_gone, exp[1])
        attempt(t_gone, att[2], 2)
        stream.synchronize()  # the only one since the chains began

    down = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    for t, want_type in ((lb1, 1), (la1, 3), (lb2, 1), (la2, 2)):
        got = t.type.cpu().tolist()
        assert got[0] == want_type and got[1] not in (1, 2, 3) and t.count.cpu().tolist() == [1] and t.status.cpu().tolist() == [0]
        assert t.n_out.cpu().tolist() == [t.length, 0]

    # ---- the same chains through the host forms and the restatements
    rk, tm, hp, gen, states, keys = (x.copy() for x in (a_rekey, a_timers, a_hs_peers, a_gen, a_states, a_keys))
    tables = lambda: [x.copy() for x in (a_kp, a_slots, a_peer_keys, a_keys, a_key_peer)]  # noqa: E731

    def host_attempt(now, k):
        o = dict(start=np.zeros(1, HS_START_DTYPE), start_peer=np.zeros(1, np.uint32), count=np.zeros(1, np.uint32),
                 status=np.zeros(n_peers, np.int32), reasons=np.zeros(n_peers, np.uint32),
                 msgs=np.full(160, 0xA5, np.uint8), init_status=np.zeros(1, np.int32))
        rekey.start_host(now, rk, hp, a_tickets[k:k + 1], o["start"], o["start_peer"], o["count"], o["status"], o["reasons"])
        noise.initiate_host(o["start"], a_public, a_table, states, o["msgs"], o["init_status"], n_keys)
        timers.initiated_host(o["reasons"], o["start_peer"], o["init_status"], now, SEED, tm)
        cg.initiated_host(o["start"], o["init_status"], o["msgs"], gen)
        assert o["status"][a_pr] == HS_STARTED and o["init_status"].tolist() == [HS_INITIATED] and o["start_peer"].tolist() == [a_pr]
        for name, x in o.items():
            assert x.tobytes() == down(att[k][name], np.uint8)[:x.nbytes].tobytes(), (k, name)
        return o

    def host_expire(now, k):
        o = dict(ka_peer=np.zeros(1, np.uint32), ka_count=np.zeros(1, np.int32), ka_sizes=np.zeros(1, np.int32),
                 ka_status=np.zeros(1, np.int32), n_ka=np.zeros(1, np.uint32), actions=np.zeros(n_peers, np.uint32))
        timers.expire_host(now, tm, rk, a_table, None, *tables(), o["ka_peer"], o["ka_count"], o["ka_sizes"], o["ka_status"],
                           o["n_ka"], o["actions"])
        for name, x in o.items():
            assert x.tobytes() == down(exp[k][name], np.uint8)[:x.nbytes].tobytes(), (k, name)

    def arena_with(msg: bytes):
        a = np.full(N * SLOT, 0xA5, np.uint8)
        a[:len(msg)] = np.frombuffer(msg, np.uint8)
        return a

    # 1.
    o0 = host_attempt(NOW, 0)
    msg1 = o0["msgs"][:148].tobytes()
    assert msg1[132:] == bytes(16) and o0["reasons"][a_pr] == WANT_NO_KEYPAIR and not o0["start"]["flags"][0]
    assert gen["last_mac1"][a_pr].tobytes() == msg1[116:132] and gen["flags"].tolist() == [int(r == a_pr) for r in range(n_peers)]
    # 2. the restatement of the screen: a cookie reply for the source A's datagram came from
    v, reply = cookie_ref.screen(checker, 1, msg1, a_src, True, nonces[:24])
    assert v == HS_COOKIE and d_screen1.cpu().tolist() == [HS_COOKIE, HS_NONE]
    assert down(d_reply1, np.uint8)[:64].tobytes() == reply
    # 3. the host form over the rows classify wrote
    want_kept = cg.consume_host(arena_with(reply), down(la1.pkts, AEAD_PKT_DTYPE), down(la1.type, np.int32), t_reply, a_hs_slots,
                                states, a_slots, a_key_peer, a_rows, gen, hp)
    assert want_kept.tolist() == [HS_COOKIE_KEPT, HS_NONE] == d_kept.cpu().tolist() and not down(d_cwork, np.uint8).any()
    the_cookie = checker.cookie(a_src)
    assert hp["cookie"][a_pr].tobytes() == the_cookie and hp["flags"][a_pr] == HS_PEER_COOKIE
    assert gen["cookie_set_at_ns"][a_pr] == t_reply
    # 4.
    cg.age_host(t_retry, gen, hp)
    assert hp["flags"][a_pr] == HS_PEER_COOKIE
    host_expire(t_retry, 0)
    assert rk["want"][a_pr] == WANT_RETRY
    o1 = host_attempt(t_retry, 1)
    msg2 = o1["msgs"][:148].tobytes()
    assert msg2[132:] == cookie_ref.mac128(the_cookie, msg2[:132])  # the reference's MAC2, cookie.go:309-313
    assert msg2 == cookie_ref.add_macs(checker.mac1_key, msg2[:116] + bytes(32), the_cookie)[0]
    assert gen["last_mac1"][a_pr].tobytes() == msg2[116:132]
    # 5.
    v, r = cookie_ref.screen(checker, 1, msg2, a_src, True, nonces[:24])
    assert (v, r) == (HS_PASS, None) and d_screen2.cpu().tolist() == [HS_PASS, HS_NONE]
    assert (down(d_reply2, np.uint8) == 0xA5).all()
    assert d_b_cookie.cpu().tolist() == [HS_NONE, HS_NONE] and not down(d_b_cwork, np.uint8).any()
    consumed, init_row = noise.consume_initiation(b_self, b_table, msg2)
    h_init = np.full(128 * N, 0xEE, np.uint8).view(HS_INIT_DTYPE)
    h_init[0] = init_row[0]
    assert consumed == HS_CONSUMED and d_consumed.cpu().tolist() == [HS_CONSUMED, HS_NONE]
    assert down(d_hs_init, np.uint8).tobytes() == h_init.tobytes()
    b_hp, h_resp, h_count, h_accept = b_hs_peers.copy(), np.zeros(1, HS_RESP_DTYPE), np.zeros(1, np.uint32), np.zeros(N, np.int32)
    noise.accept_host(h_init, np.array([HS_CONSUMED, HS_NONE], np.int32), t_retry, b_table, b_rows, b_hp, b_tickets, h_resp,
                      h_count, h_accept)
    assert h_accept.tolist() == [HS_ACCEPTED, HS_NONE] == d_accept.cpu().tolist() and d_n_resp.cpu().tolist() == [1]
    assert down(d_resp, np.uint8).tobytes() == h_resp.tobytes() and down(B["hs_peers"], np.uint8).tobytes() == b_hp.tobytes()
    rc, resp_msg, send, recv = noise.create_response(init_row, a_public, b_tickets["ephemeral_private"][0].tobytes(), b_index)
    assert rc == 0 and d_resp_status.cpu().tolist() == [HS_RESPONDED]
    assert down(d_resp_msgs, np.uint8).tobytes() == resp_msg + bytes(4) and resp_msg[76:] == bytes(16)  # B holds no cookie
    want_b_keys = b_keys.copy()
    want_b_keys["key"][2], want_b_keys["key"][3] = np.frombuffer(send, np.uint8), np.frombuffer(recv, np.uint8)
    want_b_keys["remote_index"][2], want_b_keys["remote_index"][3] = int(init_row["sender"][0]), 0
    want_b_keys["pad"][2:4] = 0
    assert down(B["keys"], np.uint8).tobytes() == want_b_keys.tobytes()
    h_b_gen = b_gen.copy()
    cg.responded_host(h_resp, np.array([HS_RESPONDED], np.int32), np.frombuffer(resp_msg + bytes(4), np.uint8), h_b_gen)
    assert h_b_gen["last_mac1"][b_pr].tobytes() == resp_msg[60:76] and h_b_gen["flags"][b_pr] == 1
    assert down(B["gen"], np.uint8).tobytes() == h_b_gen.tobytes()
    # 6.
    h_finished, h_fwork = np.zeros(N, np.int32), np.zeros(noise.FINISH_WORK_BYTES * N, np.uint8)
    noise.finish_host(arena_with(resp_msg), down(la2.pkts, AEAD_PKT_DTYPE), down(la2.type, np.int32), None, a_self, a_hs_slots,
                      states, None, keys, h_fwork, h_finished, n_peers=n_peers)
    assert h_finished.tolist() == [HS_FINISHED, HS_NONE] == d_finished.cpu().tolist()
    assert keys["key"][2].tobytes() == recv and keys["key"][3].tobytes() == send  # ticket 1's rows: A sends under B's recv
    # 7.
    cg.age_host(t_kept, gen, hp)
    assert hp["flags"][a_pr] == HS_PEER_COOKIE and d_peers_kept.cpu().numpy().tobytes() == hp.tobytes()
    cg.age_host(t_gone, gen, hp)
    assert hp["flags"][a_pr] == 0 and hp["cookie"][a_pr].tobytes() == the_cookie
    host_expire(t_gone, 1)
    o2 = host_attempt(t_gone, 2)
    assert o2["msgs"][132:148].tobytes() == bytes(16) and not o2["start"]["flags"][0]
    # the tables, whole
    for name, want, dt in (("rekey", rk, REKEY_DTYPE), ("timers", tm, TIMERS_DTYPE), ("hs_peers", hp, HS_PEER_DTYPE),
                           ("gen", gen, cg.COOKIE_GEN_DTYPE), ("states", states, HS_STATE_DTYPE), ("keys", keys, AEAD_KEY_DTYPE)):
        assert down(A[name], dt).tobytes() == want.tobytes(), name
    for name, want in (("table", a_table), ("rows", a_rows), ("hs_slots", a_hs_slots), ("slots", a_slots),
                       ("key_peer", a_key_peer), ("tickets", a_tickets)):
        assert down(A[name], np.uint8).tobytes() == want.tobytes(), name
    assert not gen["claim"].any() and gen["cookie_set_at_ns"][a_pr] == t_reply
