"""Packets that arrive before there is a session leave under the session they
caused, without a host step: both endpoints' chains enqueued on one stream with
a single synchronise at the end.

A has no keypair for B.  Four packets for B arrive, a 3-segment job and a
single one.  The send gate refuses them, the stage call puts them into B's ring
on A, the expire call -- which reads the queue's own length array as d_staged
-- owes no keepalive for that row, start and initiate build the message; B
consumes, accepts, responds and installs its next keypair; A finishes, installs
its current one, and the release call turns the ring into a job table that
send-assign, sent and seal take as it is.  B opens the four packets in the
order they were handed in, under counters 0..3, and a fifth packet sent through
the ordinary chain takes counter 4.  In the last test the handshake attempts
run out instead, and the flush call empties the ring over the expire call's
actions.  The worlds are built with the helpers of
tests/test_gpu_path_keypairs.py."""
import numpy as np
import pytest
import torch

import aead_ref
import cookie_ref
import noise_accept_cases as accept_cases
from keypairs_ref import HS_BEGUN, INITIATOR, NO_KEYPAIR, PEER_NONE, SET
from path_ref import RECV_SENTINEL
from rekey_ref import ERR_KEY_EXPIRED, HS_STARTED, WANT_NO_KEYPAIR
from test_gpu_path_keypairs import MARK, MTU, SLOT, SendJob, i32, ipv4, u8, up
from wireguard_amd import cookie, keypairs, keystate, noise, rekey, router, staged, timers, transport
from wireguard_amd._lib import (HS_FINISHED, HS_RESPONDED, REJECT_AFTER_MESSAGES, STAGED_NONE, STAGED_RELEASED,
                                TIMERS_ACT_FLUSH_STAGED, TIMERS_ACT_GAVE_UP, TIMERS_ACT_KEEPALIVE, TIMERS_KEEPALIVE_NOW,
                                TIMERS_MAX_ATTEMPTS)
from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.noise import HS_START_DTYPE
from wireguard_amd.rekey import REKEY_DTYPE
from wireguard_amd.timers import TIMERS_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

NOW = accept_cases.NOW
SEED = 0xA11CE
LIMIT = REJECT_AFTER_MESSAGES
LENGTHS = [40, 72, 56, 33]  # a 3-segment job and a single one
CAP, N_OUT_MAX, MAX_SEGS = 8, 8, 3
b_at_a, a_at_b, n_ids, n_peers, n_keys = 71, 52, 80, 4, 4  # the peer ids each side knows the other by


def down(t, dt):
    return t.cpu().numpy().view(dt)


class Ends:
    """A and B without a session, and what their hosts prepared: one ticket each"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        a_private, b_private = rng.bytes(32), rng.bytes(32)
        self.a_self, self.a_public = noise.responder_init(a_private)
        self.b_self, self.b_public = noise.responder_init(b_private)
        others = [noise.responder_init(rng.bytes(32))[1] for _ in range(3)]
        self.a_table = noise.peer_keys_build(self.a_self, [self.b_public] + others, [b_at_a, 72, 73, 74])
        self.b_table = noise.peer_keys_build(self.b_self, [self.a_public] + others, [a_at_b, 53, 54, 55])
        self.a_pr = noise.peer_keys_find(self.a_table, self.b_public)
        self.b_pr = noise.peer_keys_find(self.b_table, self.a_public)
        self.a_rows, self.b_rows = noise.peer_rows_build(self.a_table, n_ids), noise.peer_rows_build(self.b_table, n_ids)
        self.a_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
        self.b_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
        self.a_kp, self.b_kp = keypairs.keypairs_table(n_peers), keypairs.keypairs_table(n_peers)
        self.a_key_peer, self.b_key_peer = np.full(n_keys, PEER_NONE, np.uint32), np.full(n_keys, PEER_NONE, np.uint32)
        self.a_index = 0x0C0FFEE0
        self.a_tickets = np.zeros(1, HS_START_DTYPE)
        self.a_tickets[0] = (0, 0xEEEEEEEE, self.a_index, 2, 3, 0xEEEEEEEE, np.frombuffer(accept_cases.T[2], np.uint8), 0xEE,
                             np.frombuffer(rng.bytes(32), np.uint8), 0xEE, 0xEE)
        self.b_tickets = accept_cases.tickets_of(1, seed=seed + 1)
        self.b_tickets["send_key"], self.b_tickets["recv_key"] = 2, 3
        self.b_index = int(self.b_tickets["local_index"][0])
        self.a_slots = router.session_table(np.array([self.a_index], np.uint32), np.array([NO_KEYPAIR], np.uint32))
        self.b_slots = router.session_table(np.array([self.b_index], np.uint32), np.array([NO_KEYPAIR], np.uint32))
        self.a_hs_slots = router.session_table(np.array([self.a_index], np.uint32), np.array([0], np.uint32))
        self.a_peer_keys = router.session_table(self.a_table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
        self.b_peer_keys = router.session_table(self.b_table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
        self.a_hs_peers = accept_cases.peers_of(n_peers, seed=seed + 2)
        self.b_hs_peers = accept_cases.peers_of(n_peers, seed=seed + 3)
        self.a_hs_peers["flags"], self.b_hs_peers["flags"] = 0, 0
        self.a_rekey, self.b_rekey = rekey.rekey_table(n_peers, NOW), rekey.rekey_table(n_peers, NOW)
        self.a_timers = timers.timers_table(n_peers)
        self.b_checker = np.frombuffer(cookie_ref.Checker(self.b_public).tobytes(), cookie.COOKIE_CHECKER_DTYPE)
        ra = router.Router()
        ra.insert(bytes([10, 1, 2, 0]), 24, b_at_a)  # A routes the packets' destination to B
        self.a_image = ra.image()
        # the four packets as gso_split_batch leaves them: job 0 fills its three slots, job 1 one of three
        self.packets = [ipv4(rng, n) for n in LENGTHS]
        self.arena = np.full(2 * MAX_SEGS * SLOT, 0xA5, np.uint8)
        self.sizes = np.zeros(2 * MAX_SEGS, np.int32)
        for q, p in zip((0, 1, 2, 3), self.packets):
            self.arena[q * SLOT + 16:q * SLOT + 16 + len(p)] = np.frombuffer(p, np.uint8)
            self.sizes[q] = len(p)
        self.count = np.array([3, 1], np.int32)

    def upload_a(self):
        return {k: up(v) for k, v in dict(table=self.a_table, rows=self.a_rows, kp=self.a_kp, keys=self.a_keys,
                                          key_peer=self.a_key_peer, slots=self.a_slots, hs_slots=self.a_hs_slots,
                                          peer_keys=self.a_peer_keys, hs_peers=self.a_hs_peers, rekey=self.a_rekey,
                                          timers=self.a_timers, tickets=self.a_tickets, self=self.a_self,
                                          pub=np.frombuffer(self.a_public, np.uint8), image=self.a_image,
                                          nonce=np.zeros(n_keys, np.uint64), arena=self.arena, sizes=self.sizes,
                                          count=self.count, status_in=np.zeros(2, np.int32)).items()}

    def state(self):
        h = staged.state(n_peers, CAP, SLOT, fill=0xA5)
        return staged.State(*[up(a) for a in h.arrays()], n_peers, CAP, SLOT)


def refuse_and_stage(dev, A, st, o, stream):
    """route -> send gate -> send-assign -> stage over A's two jobs"""
    m = 2 * MAX_SEGS
    o.update(peer=i32(m), gate=i32(2 + 1), pkts=u8(24 * m, 0xEE), nbufs=i32(2), job_key=i32(2), where=i32(m + 1))
    router.route_dst_batch(dev, A["arena"], A["sizes"], A["image"], o["peer"], stride=SLOT, offset=16, stream=stream, n=m)
    rekey.send_gate_batch(dev, o["peer"], A["count"], A["status_in"], MAX_SEGS, NOW, A["rows"], A["kp"], A["nonce"], LIMIT,
                          A["rekey"], o["gate"], stream=stream, n_jobs=2, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
    keystate.send_assign_batch(dev, A["sizes"], o["peer"], A["count"], o["gate"], MAX_SEGS, SLOT, A["peer_keys"], A["nonce"],
                               o["pkts"], o["nbufs"], o["job_key"], o["work"], stream=stream, n_jobs=2,
                               n_slots=A["n_peer_slots"], n_keys=n_keys)
    staged.stage_batch(dev, A["arena"], A["sizes"], o["peer"], A["count"], A["status_in"], o["gate"], o["job_key"], MAX_SEGS,
                       A["rows"], st, o["where"], o["work"], stream=stream, n_jobs=2, n_ids=n_ids)


def expire(dev, A, st, now, o, stream, n_slots):
    o.update(ka_peer=i32(1 + 1), ka_count=i32(1 + 1), ka_sizes=i32(1 + 1), ka_status=i32(1 + 1), n_ka=i32(1 + 1),
             actions=i32(n_peers + 1))
    timers.expire_batch(dev, now, A["timers"], A["rekey"], A["table"], st.len, A["kp"], A["slots"], A["peer_keys"], A["keys"],
                        A["key_peer"], o["ka_peer"], o["ka_count"], o["ka_sizes"], o["ka_status"], o["n_ka"], o["actions"],
                        o["work"], stream=stream, n_peers=n_peers, n_slots=n_slots, n_peer_slots=A["n_peer_slots"],
                        n_keys=n_keys, n_ka_max=1)


def test_packets_without_a_session_leave_under_the_one_they_caused(dev):
    e = Ends(2301)
    a_pr, b_pr = e.a_pr, e.b_pr
    e.a_timers["flags"][a_pr] |= TIMERS_KEEPALIVE_NOW  # a keepalive is owed: the staged packets go out in its place
    wire_len = [len(aead_ref.wg_seal(bytes(32), 0, 0, bytes(n), MTU)) for n in LENGTHS + [64]]
    m = 5  # B's transport batch: the four staged packets and the fifth
    off2 = np.array([k * SLOT + 1 + k for k in range(m)], np.uint64)  # any byte offset
    arena2 = np.full(m * SLOT + 8, RECV_SENTINEL, np.uint8)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        A = e.upload_a()
        A["n_peer_slots"] = len(e.a_peer_keys)
        B = {k: up(v) for k, v in dict(table=e.b_table, rows=e.b_rows, kp=e.b_kp, keys=e.b_keys, key_peer=e.b_key_peer,
                                       slots=e.b_slots, peer_keys=e.b_peer_keys, hs_peers=e.b_hs_peers, rekey=e.b_rekey,
                                       tickets=e.b_tickets, self=e.b_self, checker=e.b_checker,
                                       filters=np.zeros(n_keys, REPLAY_FILTER_DTYPE)).items()}
        st = e.state()
        d_work = torch.zeros(keystate.work_bytes(8), dtype=torch.uint8, device="cuda")
        first, exp = dict(work=d_work), dict(work=d_work)
        d_start, d_start_peer, d_count, d_start_status, d_reasons = u8(96), i32(1 + 1), i32(1 + 1), i32(n_peers + 1), i32(n_peers + 1)
        d_states, d_init_msgs, d_init_status, d_fwork = u8(128), u8(160), i32(1), u8(noise.FINISH_WORK_BYTES)
        d_arena_b1, d_size_b1 = u8(SLOT, RECV_SENTINEL), up(np.array([148], np.int32))
        d_pkts_b1, d_type_b1, d_screen_b1, d_consumed, d_accept = u8(24, 0xEE), i32(1), i32(1), i32(1), i32(1)
        d_hs_init, d_resp, d_n_resp, d_resp_msgs, d_resp_status, d_begun_b = u8(128, 0xEE), u8(80), i32(1), u8(96), i32(1), i32(1 + 1)
        d_arena_a1, d_size_a1 = u8(SLOT, RECV_SENTINEL), up(np.array([92], np.int32))
        d_pkts_a1, d_type_a1, d_finished, d_begun_a = u8(24, 0xEE), i32(1), i32(1), i32(1 + 1)
        # release's job table and what the chain behind it writes
        d_out, d_out_peer, d_out_count = u8(N_OUT_MAX * SLOT + 64, 0xA5), i32(N_OUT_MAX + 1), i32(N_OUT_MAX + 1)
        d_out_sizes, d_out_status, d_n_out, d_rel = i32(N_OUT_MAX + 1), i32(N_OUT_MAX + 1), i32(1 + 1), i32(n_peers + 1)
        d_out_pkts, d_out_nbufs, d_out_key, d_out_len = u8(24 * N_OUT_MAX, 0xEE), i32(N_OUT_MAX), i32(N_OUT_MAX), i32(N_OUT_MAX)
        fifth = SendJob(np.random.default_rng(11), b_at_a, [64])
        fifth.d_peer = i32(1)
        fifth.d_status_in, fifth.d_status = fifth.d_status, i32(1 + 1)
        d_arena2, d_off2, d_size2 = up(arena2), up(off2), up(np.array(wire_len, np.int32))
        d_pkts2, d_type2, d_len2, d_verdict2 = u8(24 * m, 0xEE), i32(m), i32(m), i32(m)
        d_ctr2 = torch.zeros(m, dtype=torch.int64, device="cuda")
        stream.synchronize()

        # A: route -> send gate -> send-assign -> stage -> expire -> start -> initiate
        refuse_and_stage(dev, A, st, first, stream)
        expire(dev, A, st, NOW, exp, stream, len(e.a_slots))
        rekey.start_batch(dev, NOW, A["rekey"], A["hs_peers"], A["tickets"], d_start, d_start_peer, d_count, d_start_status,
                          d_reasons, d_work, stream=stream, n_peers=n_peers, n_tickets=1)
        noise.initiate_batch(dev, d_start, A["pub"], A["table"], d_states, d_init_msgs, d_init_status, n_keys, stream=stream,
                             n=1, n_peers=n_peers, n_states=1)
        # B: classify -> screen -> consume -> accept -> respond -> begin-responder
        d_arena_b1[:148].copy_(d_init_msgs[:148])
        router.classify_batch(dev, d_arena_b1, d_size_b1, B["slots"], d_pkts_b1, d_type_b1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(e.b_slots))
        cookie.screen_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, B["checker"], None, d_screen_b1, under_load=False,
                            stream=stream, n=1)
        noise.consume_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, d_screen_b1, B["self"], B["table"], d_consumed, d_hs_init,
                            stream=stream, n=1, n_peers=n_peers)
        noise.accept_batch(dev, d_hs_init, d_consumed, NOW, B["table"], B["rows"], B["hs_peers"], B["tickets"], d_resp, d_n_resp,
                           d_accept, stream=stream, n=1, n_ids=n_ids, n_peers=n_peers, n_tickets=1)
        noise.respond_batch(dev, d_resp, d_hs_init, None, B["table"], None, B["keys"], d_resp_msgs, d_resp_status, stream=stream,
                            n=1, n_init=1, n_peers=n_peers, n_keys=n_keys)
        keypairs.begin_responder_batch(dev, d_resp, d_resp_status, NOW, B["table"], B["kp"], B["slots"], B["peer_keys"],
                                       B["keys"], B["key_peer"], d_begun_b, d_work, stream=stream, n=1, n_peers=n_peers,
                                       n_slots=len(e.b_slots), n_peer_slots=len(e.b_peer_keys), n_keys=n_keys)
        # A: classify -> finish -> begin-initiator -> release -> send-assign -> sent (rekey, timers) -> seal
        d_arena_a1[:92].copy_(d_resp_msgs[:92])
        router.classify_batch(dev, d_arena_a1, d_size_a1, A["slots"], d_pkts_a1, d_type_a1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(e.a_slots))
        noise.finish_batch(dev, d_arena_a1, d_pkts_a1, d_type_a1, None, A["self"], A["hs_slots"], d_states, None, A["keys"],
                           d_fwork, d_finished, stream=stream, n=1, n_slots=len(e.a_hs_slots), n_states=1, n_peers=n_peers,
                           n_keys=n_keys)
        keypairs.begin_initiator_batch(dev, d_arena_a1, d_pkts_a1, d_finished, NOW, A["hs_slots"], d_states, A["table"], A["kp"],
                                       A["slots"], A["peer_keys"], A["keys"], A["key_peer"], d_begun_a, d_work, stream=stream,
                                       n=1, n_hs_slots=len(e.a_hs_slots), n_states=1, n_peers=n_peers, n_slots=len(e.a_slots),
                                       n_peer_slots=len(e.a_peer_keys), n_keys=n_keys)
        staged.release_batch(dev, NOW, A["table"], A["kp"], A["nonce"], LIMIT, A["rekey"], st, N_OUT_MAX, d_out, d_out_peer,
                             d_out_count, d_out_sizes, d_out_status, d_n_out, d_rel, d_work, stream=stream, n_keys=n_keys)
        keystate.send_assign_batch(dev, d_out_sizes, d_out_peer, d_out_count, d_out_status, 1, SLOT, A["peer_keys"], A["nonce"],
                                   d_out_pkts, d_out_nbufs, d_out_key, d_work, stream=stream, n_jobs=N_OUT_MAX,
                                   n_slots=len(e.a_peer_keys), n_keys=n_keys)
        rekey.sent_batch(dev, d_out_peer, d_out_count, d_out_status, d_out_key, 1, NOW, A["rows"], A["kp"], A["nonce"], LIMIT,
                         A["rekey"], stream=stream, n_jobs=N_OUT_MAX, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
        timers.sent_batch(dev, d_out_sizes, d_out_peer, d_out_count, d_out_status, d_out_key, 1, NOW, SEED, A["rows"],
                          A["timers"], stream=stream, n_jobs=N_OUT_MAX, n_ids=n_ids, n_peers=n_peers)
        transport.seal_batch(dev, d_out, d_out_pkts, A["keys"], MTU, d_out_len, stream=stream, n=N_OUT_MAX, n_keys=n_keys)
        # A: a fifth packet through the ordinary chain
        router.route_dst_batch(dev, fifth.d_arena, fifth.d_sizes, A["image"], fifth.d_peer, stride=SLOT, offset=16,
                               stream=stream, n=1)
        rekey.send_gate_batch(dev, fifth.d_peer, fifth.d_count, fifth.d_status_in, 1, NOW, A["rows"], A["kp"], A["nonce"], LIMIT,
                              A["rekey"], fifth.d_status, stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
        fifth.enqueue(dev, A["peer_keys"], len(e.a_peer_keys), A["nonce"], A["keys"], n_keys, d_work, stream)
        # B: classify -> open -> replay over the five messages
        for k in range(4):
            o = int(off2[k])
            d_arena2[o:o + wire_len[k]].copy_(d_out[k * SLOT:k * SLOT + wire_len[k]])
        o = int(off2[4])
        d_arena2[o:o + wire_len[4]].copy_(fifth.d_arena[:wire_len[4]])
        router.classify_batch(dev, d_arena2, d_size2, B["slots"], d_pkts2, d_type2, off=d_off2, stream=stream, n=m,
                              n_slots=len(e.b_slots))
        transport.open_batch(dev, d_arena2, d_pkts2, B["keys"], d_len2, d_ctr2, stream=stream, n=m, n_keys=n_keys)
        keystate.replay_batch(dev, d_pkts2, d_len2, d_ctr2, B["filters"], d_verdict2, d_work, stream=stream, n=m, n_keys=n_keys)
        stream.synchronize()  # the only one since the chains began

    # A: refused for want of a keypair, and staged in the order handed in
    assert first["gate"].cpu().tolist() == [ERR_KEY_EXPIRED, ERR_KEY_EXPIRED, MARK]
    s0 = a_pr * CAP
    assert down(first["where"], np.uint32).tolist() == [s0, s0 + 1, s0 + 2, s0 + 3, STAGED_NONE, STAGED_NONE, MARK]
    assert down(d_reasons, np.uint32)[a_pr] == WANT_NO_KEYPAIR and d_start_status.cpu().tolist()[a_pr] == HS_STARTED
    # the expire call read d_len: the keepalive that was owed is not sent, the staged packets go in its place
    assert exp["n_ka"].cpu().tolist() == [0, MARK] and down(exp["actions"], np.uint32)[a_pr] == 0
    assert down(exp["ka_peer"], np.uint32).tolist() == [PEER_NONE, MARK]
    h = dict(ka_peer=np.zeros(1, np.uint32), ka_count=np.zeros(1, np.int32), ka_sizes=np.zeros(1, np.int32),
             ka_status=np.zeros(1, np.int32), n_ka=np.zeros(1, np.uint32), actions=np.zeros(n_peers, np.uint32))
    timers.expire_host(NOW, e.a_timers.copy(), e.a_rekey.copy(), e.a_table, None, e.a_kp.copy(), e.a_slots.copy(),
                       e.a_peer_keys.copy(), e.a_keys.copy(), e.a_key_peer.copy(), *h.values())
    assert h["actions"][a_pr] == TIMERS_ACT_KEEPALIVE, "without d_staged a keepalive would have been sent"
    # the handshake
    assert d_init_status.cpu().tolist() == [noise.HS_INITIATED] and d_accept.cpu().tolist() == [noise.HS_ACCEPTED]
    assert d_resp_status.cpu().tolist() == [HS_RESPONDED] and d_begun_b.cpu().tolist() == [HS_BEGUN, MARK]
    assert d_finished.cpu().tolist() == [HS_FINISHED] and d_begun_a.cpu().tolist() == [HS_BEGUN, MARK]
    assert tuple(down(A["kp"], KEYPAIRS_DTYPE)["current"][a_pr]) == (2, 3, e.a_index, SET | INITIATOR, NOW)
    # the release: four jobs in order, then the tail; the ring is empty
    rel = d_rel.cpu().tolist()
    assert rel[a_pr] == STAGED_RELEASED and sum(rel[:n_peers]) == STAGED_RELEASED and rel[n_peers] == MARK
    assert d_n_out.cpu().tolist() == [4, MARK]
    assert down(d_out_peer, np.uint32).tolist() == [b_at_a] * 4 + [PEER_NONE] * 4 + [MARK]
    assert d_out_count.cpu().tolist() == [1] * 4 + [0] * 4 + [MARK] and d_out_sizes.cpu().tolist() == LENGTHS + [0] * 4 + [MARK]
    assert d_out_status.cpu().tolist() == [0] * 8 + [MARK]
    assert d_out_nbufs.cpu().tolist() == [1] * 4 + [0] * 4 and down(d_out_key, np.uint32)[:4].tolist() == [2] * 4
    assert d_out_len.cpu().tolist()[:4] == wire_len[:4]
    assert not down(st.len, np.uint32).any() and not down(st.head, np.uint32).any() and not down(st.lost, np.uint32).any()
    assert down(A["nonce"], np.uint64)[2] == 5
    assert not down(A["rekey"], REKEY_DTYPE)["want"].any()
    assert not down(A["timers"], TIMERS_DTYPE)["flags"][a_pr] & TIMERS_KEEPALIVE_NOW
    # B: the four plaintexts in the order they were handed in under counters 0..3, the fifth under 4
    assert d_type2.cpu().tolist() == [4] * m and down(d_pkts2, AEAD_PKT_DTYPE)["key"].tolist() == [3] * m
    assert d_ctr2.cpu().tolist() == [0, 1, 2, 3, 4]
    assert d_len2.cpu().tolist() == LENGTHS + [64] and d_verdict2.cpu().tolist() == LENGTHS + [64]
    got2 = d_arena2.cpu().numpy()
    for k, p in enumerate(e.packets + fifth.packets):
        o = int(off2[k]) + 16
        assert got2[o:o + len(p)].tobytes() == p, f"packet {k} did not arrive"


def test_the_queue_is_flushed_when_the_attempts_run_out(dev):
    e = Ends(2311)
    a_pr = e.a_pr
    t = e.a_timers[a_pr]
    t["attempts"], t["pending"] = TIMERS_MAX_ATTEMPTS + 1, 1 << timers.TIMER_RESEND_HANDSHAKE
    t["deadline_ns"][timers.TIMER_RESEND_HANDSHAKE] = NOW
    e.a_timers[a_pr] = t
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        A = e.upload_a()
        A["n_peer_slots"] = len(e.a_peer_keys)
        st = e.state()
        d_work = torch.zeros(keystate.work_bytes(8), dtype=torch.uint8, device="cuda")
        first, exp = dict(work=d_work), dict(work=d_work)
        stream.synchronize()
        refuse_and_stage(dev, A, st, first, stream)
        d_len_then = st.len.clone()
        expire(dev, A, st, NOW, exp, stream, len(e.a_slots))
        staged.flush_batch(dev, exp["actions"], st, stream=stream)
        stream.synchronize()
    assert down(d_len_then, np.uint32)[a_pr] == 4
    act = down(exp["actions"], np.uint32)
    assert act[a_pr] & TIMERS_ACT_GAVE_UP and act[a_pr] & TIMERS_ACT_FLUSH_STAGED and not np.delete(act[:n_peers], a_pr).any()
    assert not down(st.len, np.uint32).any() and not down(st.head, np.uint32).any()
    lost = down(st.lost, np.uint32)
    assert lost[a_pr] == 4 and lost.sum() == 4
