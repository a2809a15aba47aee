"""The peer endpoints in their places on the two chains, two roles on one stream
with nothing read back until the single synchronise at the end.

A initiates to B, whose address it has from the UAPI; B is under load, so A's
initiation carries a MAC2 for the cookie of the address it comes from.
  A  send-gate (refused) -> start -> initiate -> dst_initiated
  B  split -> endpoint_recv -> classify -> screen (under load, d_addr_out as its
     d_src) -> ratelimit (d_addr_out) -> consume -> accept -> set_accepted ->
     respond -> dst_responded: the response is addressed to the initiation's
     source, with the sticky source of the slot the split put it in
  A  endpoint_recv -> classify -> finish -> set_finished -> begin-initiator, then
     a send job: seal -> dst_jobs -> coalesce_dst
  B  two transport packets of A, the first from address A0 and the second from
     the IPv6 address A1: endpoint_recv -> ... -> write_build -> set_received; B's
     next job goes to A1 with A1's sticky source, as an IPv6 batch of coalesce_dst
  B  16 s later newHandshake fires in the expire call and sets
     WGCS_TIMERS_CLEAR_SRC: the next job's source is empty and the table's too; a
     packet received afterwards restores it
  B  a job for a peer that has a keypair and never had an endpoint gets
     WGCS_ERR_NO_ENDPOINT and no message.
The worlds are built with the helpers of tests/test_gpu_path_keypairs.py."""
import numpy as np
import pytest
import torch

import cookie_ref
import noise_accept_cases as accept_cases
from endpoint_cases import PKTINFO4, PKTINFO6, addr_row, dst_bytes
from keypairs_ref import HS_BEGUN, NO_KEYPAIR, PEER_NONE, SET
from path_ref import RECV_SENTINEL
from rekey_ref import ERR_KEY_EXPIRED, SECOND
from test_gpu_path_keypairs import MARK, MTU, SLOT, SendJob, i32, u8, up
from timers_ref import ACTIVE, CLEAR_SRC, HS_FINISHED, HS_INITIATED, HS_RESPONDED
from wireguard_amd import cookie, endpoint as ep, keypairs, keystate, noise, ratelimit as rl, rekey, router, timers, transport, writeplan
from wireguard_amd._lib import ERR_NO_ENDPOINT, HS_PASS, HS_PEER_COOKIE, REJECT_AFTER_MESSAGES
from wireguard_amd.cookie import SRC_ADDR_DTYPE
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.noise import HS_START_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE
from wireguard_amd.tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

pytestmark = pytest.mark.gpu

NOW = accept_cases.NOW
SEED = 0xE9D
LIMIT = REJECT_AFTER_MESSAGES
OOB = 64  # bytes of control per slot


def sticky4(ifindex: int, last: int) -> bytes:
    return PKTINFO4[:16] + ifindex.to_bytes(4, "little") + bytes([10, 9, 0, last]) + bytes([10, 9, 0, last]) + bytes(4)


def oob_table(controls) -> tuple:
    oob, nn = np.full(len(controls) * OOB, 0xCC, np.uint8), np.zeros(len(controls), np.int32)
    for q, c in enumerate(controls):
        oob[q * OOB:q * OOB + len(c)] = np.frombuffer(c, np.uint8)
        nn[q] = len(c)
    return oob, nn


def test_endpoints_on_both_chains_with_nothing_read_back(dev):
    rng = np.random.default_rng(3001)
    a_private, b_private = rng.bytes(32), rng.bytes(32)
    a_self, a_public = noise.responder_init(a_private)
    b_self, b_public = noise.responder_init(b_private)
    others = [noise.responder_init(rng.bytes(32))[1] for _ in range(3)]
    b_at_a, a_at_b, c_at_b, n_ids = 71, 52, 53, 80
    a_table = noise.peer_keys_build(a_self, [b_public] + others, [b_at_a, 72, 73, 74])
    b_table = noise.peer_keys_build(b_self, [a_public] + others, [a_at_b, c_at_b, 54, 55])
    n_peers, n_keys = 4, 6
    a_pr, b_pr = noise.peer_keys_find(a_table, b_public), noise.peer_keys_find(b_table, a_public)
    c_pr = noise.peer_keys_find(b_table, others[0])
    a_rows, b_rows = noise.peer_rows_build(a_table, n_ids), noise.peer_rows_build(b_table, n_ids)
    a_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    b_keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
    a_kp, b_kp = keypairs.keypairs_table(n_peers), keypairs.keypairs_table(n_peers)
    a_key_peer, b_key_peer = np.full(n_keys, PEER_NONE, np.uint32), np.full(n_keys, PEER_NONE, np.uint32)
    # B's third party C has a keypair (key rows 4 and 5) and never had an endpoint
    b_kp["current"][c_pr] = (4, 5, 0x00005353, SET, NOW)
    b_key_peer[4:6] = c_at_b
    a_index = 0x0E0FFEE0
    a_tickets = np.zeros(1, HS_START_DTYPE)
    a_tickets[0] = (0, 0xEEEEEEEE, a_index, 0, 1, 0xEEEEEEEE, np.frombuffer(accept_cases.T[2], np.uint8), 0xEE,
                    np.frombuffer(rng.bytes(32), np.uint8), 0xEE, 0xEE)
    b_tickets = accept_cases.tickets_of(1, seed=3002)
    b_tickets["send_key"], b_tickets["recv_key"] = 2, 3
    b_index = int(b_tickets["local_index"][0])
    a_slots = router.session_table(np.array([a_index], np.uint32), np.array([NO_KEYPAIR], np.uint32))
    b_slots = router.session_table(np.array([b_index], np.uint32), np.array([NO_KEYPAIR], np.uint32))
    a_hs_slots = router.session_table(np.array([a_index], np.uint32), np.array([0], np.uint32))
    a_peer_keys = router.session_table(a_table["peer"], np.full(n_peers, NO_KEYPAIR, np.uint32))
    b_peer_keys = router.session_table(b_table["peer"], np.where(b_table["peer"] == c_at_b, 4, NO_KEYPAIR).astype(np.uint32))
    a_hs_peers, b_hs_peers = accept_cases.peers_of(n_peers, seed=3003), accept_cases.peers_of(n_peers, seed=3004)
    a_hs_peers["flags"], b_hs_peers["flags"] = 0, 0
    a_rekey, b_rekey = rekey.rekey_table(n_peers, NOW), rekey.rekey_table(n_peers, NOW)
    a_timers, b_timers = timers.timers_table(n_peers), timers.timers_table(n_peers)
    # addresses and sticky sources
    A0, A1 = dst_bytes(bytes([203, 0, 113, 5]), 40001), dst_bytes(bytes.fromhex("20010db8" + "00" * 11 + "a1"), 40002)
    B0 = dst_bytes(bytes([198, 51, 100, 7]), 51820)
    S0, S2, S_A, S1 = sticky4(3, 1), sticky4(4, 2), sticky4(2, 9), PKTINFO6
    # B is under load: A holds the cookie B would hand the address A0 (a cookie reply it consumed earlier)
    checker = cookie_ref.Checker(b_public, rng.bytes(32))
    b_checker = np.frombuffer(checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE)
    a_hs_peers["cookie"][a_pr] = np.frombuffer(checker.cookie(A0), np.uint8)
    a_hs_peers["flags"][a_pr] = HS_PEER_COOKIE
    # the endpoint tables: A knows B's address from the UAPI, B knows nobody's
    a_ep, a_claim = ep.table(n_peers)
    a_ep[a_pr] = ep.row(B0[:4], 51820)[0]
    b_ep, b_claim = ep.table(n_peers)
    ra = router.Router()
    ra.insert(bytes([10, 1, 2, 0]), 24, b_at_a)
    a_image = ra.image()
    T2 = NOW + 16 * SECOND  # past newHandshake's 15 s + jitter (< 334 ms)

    # B's handshake batch: 4 slots, messages land from slot 2 on; the split carries slot 2's message to slot 0
    n1, first = 4, 2
    addr1 = np.zeros(n1, SRC_ADDR_DTYPE)
    addr1[2] = addr_row(A0)[0]
    oob1, nn1 = oob_table([S0, b"", S2, b""])  # slot 0 keeps the control of an earlier recvmmsg: the packet takes it
    n_in1, gso1 = np.array([0, 0, 148, 0], np.int32), np.zeros(n1, np.int32)
    # A's handshake batch (the response, from B0), B's transport batches (two packets, then one)
    addr_a, (oob_a, nn_a) = addr_row(B0), oob_table([S_A])
    addr2, (oob2, nn2) = np.concatenate([addr_row(A0), addr_row(A1)]), oob_table([S0, S1])
    addr3, (oob3, nn3) = addr_row(A1), oob_table([S1])

    def endpoint_outputs(n):
        return dict(dst=u8(64 * n, 0xEE), v6=i32(n), status=i32(n), tx=torch.full((n,), -1, dtype=torch.int64, device="cuda"),
                    nm=i32(1), first=i32(n), mlen=i32(n), gso=i32(n))

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        A = {k: up(v) for k, v in dict(table=a_table, rows=a_rows, kp=a_kp, keys=a_keys, key_peer=a_key_peer, slots=a_slots,
                                       hs_slots=a_hs_slots, peer_keys=a_peer_keys, hs_peers=a_hs_peers, rekey=a_rekey,
                                       timers=a_timers, tickets=a_tickets, self=a_self, pub=np.frombuffer(a_public, np.uint8),
                                       image=a_image, nonce=np.zeros(n_keys, np.uint64), ep=a_ep, claim=a_claim).items()}
        B = {k: up(v) for k, v in dict(table=b_table, rows=b_rows, kp=b_kp, keys=b_keys, key_peer=b_key_peer, slots=b_slots,
                                       peer_keys=b_peer_keys, hs_peers=b_hs_peers, rekey=b_rekey, timers=b_timers,
                                       tickets=b_tickets, self=b_self, checker=b_checker, nonce=np.zeros(n_keys, np.uint64),
                                       filters=np.zeros(n_keys, REPLAY_FILTER_DTYPE), ep=b_ep, claim=b_claim,
                                       rl=rl.table(64)).items()}
        d_work = torch.zeros(keystate.work_bytes(8), dtype=torch.uint8, device="cuda")
        d_rl_work = torch.zeros(rl.work_bytes(n1), dtype=torch.uint8, device="cuda")
        d_fwork, d_states = u8(noise.FINISH_WORK_BYTES), u8(128)
        job0 = SendJob(np.random.default_rng(7), b_at_a, [40])
        job0.d_peer, job0.d_status_in, job0.d_status = i32(1), job0.d_status, i32(1)
        att = dict(start=u8(96), start_peer=i32(1), count=i32(1), status=i32(n_peers), reasons=i32(n_peers), msgs=u8(160),
                   init_status=i32(1))
        oI, oR = endpoint_outputs(1), endpoint_outputs(1)
        # B's handshake batch
        d_land, d_n_in1, d_gso1 = u8(2 * SLOT, RECV_SENTINEL), up(n_in1), up(gso1)
        d_arena_b1, d_n_out1, d_from1, d_count1, d_split1 = u8(n1 * SLOT, RECV_SENTINEL), i32(n1), i32(n1), i32(1), i32(1)
        d_addr1, d_oob1, d_nn1 = up(addr1), up(oob1), up(nn1)
        d_ep1, d_addr_out1 = u8(64 * n1, 0xEE), u8(20 * n1, 0xEE)
        d_pkts_b1, d_type_b1, d_screen, d_limited, d_consumed, d_accept = u8(24 * n1, 0xEE), i32(n1), i32(n1), i32(n1), i32(n1), i32(n1)
        d_nonce, d_reply = up(np.frombuffer(rng.bytes(24 * n1), np.uint8)), u8(64 * n1)
        d_hs_init, d_resp, d_n_resp, d_resp_msgs, d_resp_status, d_begun_b = u8(128 * n1, 0xEE), u8(80), i32(1), u8(96), i32(1), i32(1)
        # A's handshake batch
        d_arena_a1, d_size_a1 = u8(SLOT, RECV_SENTINEL), up(np.array([92], np.int32))
        d_addr_a, d_oob_a, d_nn_a, d_ep_a = up(addr_a), up(oob_a), up(nn_a), u8(64, 0xEE)
        d_pkts_a1, d_type_a1, d_finished, d_begun_a = u8(24, 0xEE), i32(1), i32(1), i32(1)

        def send(side, job, now, out, with_timers=False):
            """send-gate -> send-assign -> seal -> dst_jobs -> coalesce_dst, one job"""
            job.d_status_in, job.d_status = job.d_status, i32(1)
            rekey.send_gate_batch(dev, job.d_peer, job.d_count, job.d_status_in, job.m, now, side["rows"], side["kp"],
                                  side["nonce"], LIMIT, side["rekey"], job.d_status, stream=stream, n_jobs=1, n_ids=n_ids,
                                  n_peers=n_peers, n_keys=n_keys)
            job.enqueue(dev, side["peer_keys"], n_peers_slots[id(side)], side["nonce"], side["keys"], n_keys, d_work, stream)
            if with_timers:
                timers.sent_batch(dev, job.d_sizes, job.d_peer, job.d_count, job.d_status, job.d_job_key, job.m, now, SEED,
                                  side["rows"], side["timers"], stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers)
            ep.dst_jobs_batch(dev, job.d_peer, job.d_count, job.d_status, job.d_job_key, job.m, job.d_out_len, job.d_nbufs,
                              side["rows"], side["ep"], side["timers"], out["dst"], out["v6"], out["status"], out["tx"],
                              stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers)
            ep.coalesce_dst_batch(dev, job.d_arena, SLOT, SLOT, None, job.d_out_len, job.d_nbufs, job.m, 1, out["v6"], out["nm"],
                                  out["first"], out["mlen"], out["gso"], stream=stream)

        n_peers_slots = {id(A): len(a_peer_keys), id(B): len(b_peer_keys)}

        def receive(d_arena, m, d_addr, d_oob, d_nn, now, o):
            """B: endpoint_recv -> classify -> recv-gate -> open -> replay -> received -> write-build -> set_received"""
            ep.recv_batch(dev, d_addr, None, o["size"], d_oob, OOB, d_nn, m, 1, o["ep"], None, stream=stream)
            router.classify_batch(dev, d_arena, o["size"], B["slots"], o["pkts"], o["type"], stride=SLOT, stream=stream, n=m,
                                  n_slots=len(b_slots))
            rekey.recv_gate_batch(dev, o["pkts"], now, B["key_peer"], B["rows"], B["kp"], stream=stream, n=m, n_keys=n_keys,
                                  n_ids=n_ids, n_peers=n_peers)
            transport.open_batch(dev, d_arena, o["pkts"], B["keys"], o["len"], o["ctr"], stream=stream, n=m, n_keys=n_keys)
            keystate.replay_batch(dev, o["pkts"], o["len"], o["ctr"], B["filters"], o["verdict"], d_work, stream=stream, n=m,
                                  n_keys=n_keys)
            keypairs.received_batch(dev, o["pkts"], o["verdict"], B["key_peer"], B["rows"], B["kp"], B["slots"], B["peer_keys"],
                                    B["keys"], o["rotated"], stream=stream, n=m, n_keys=n_keys, n_ids=n_ids, n_peers=n_peers,
                                    n_slots=len(b_slots), n_peer_slots=len(b_peer_keys))
            writeplan.write_build_batch(dev, o["pkts"], o["verdict"], m, B["key_peer"], 16, SLOT, 1, o["bufs"], o["calls"],
                                        o["groups"], o["n_groups"], o["wstatus"], stream=stream, n_batches=1, n_keys=n_keys)
            ep.set_received_batch(dev, o["groups"], 1, o["ep"], B["rows"], B["ep"], B["claim"], B["timers"], stream=stream,
                                  n_batches=1, n_rows=m, n_ids=n_ids, n_peers=n_peers)
            timers.received_batch(dev, o["groups"], 1, now, B["rows"], B["timers"], stream=stream, n_batches=1, n_ids=n_ids,
                                  n_peers=n_peers)

        def receive_outputs(m, sizes):
            return dict(size=up(np.array(sizes, np.int32)), ep=u8(64 * m, 0xEE), pkts=u8(24 * m, 0xEE), type=i32(m), len=i32(m),
                        ctr=torch.zeros(m, dtype=torch.int64, device="cuda"), verdict=i32(m), rotated=i32(m),
                        bufs=u8(GRO_BUF_DTYPE.itemsize * m), calls=u8(GRO_CALL_DTYPE.itemsize), groups=u8(WRITE_GROUP_DTYPE.itemsize),
                        n_groups=i32(1), wstatus=i32(1))

        jobA1, jobA2 = SendJob(np.random.default_rng(8), b_at_a, [64, 64]), SendJob(np.random.default_rng(9), b_at_a, [64])
        jobB1, jobB2 = SendJob(np.random.default_rng(10), a_at_b, [64, 64]), SendJob(np.random.default_rng(11), a_at_b, [64, 64])
        jobC = SendJob(np.random.default_rng(12), c_at_b, [64])
        oA1, oA2, oB1, oB2, oC = (endpoint_outputs(j.m) for j in (jobA1, jobA2, jobB1, jobB2, jobC))
        d_arena2, d_arena3 = u8(2 * SLOT, RECV_SENTINEL), u8(SLOT, RECV_SENTINEL)
        r2, r3 = receive_outputs(2, [96, 96]), receive_outputs(1, [96])
        d_addr2, d_oob2, d_nn2, d_addr3, d_oob3, d_nn3 = up(addr2), up(oob2), up(nn2), up(addr3), up(oob3), up(nn3)
        exp = dict(ka_peer=i32(1), ka_count=i32(1), ka_sizes=i32(1), ka_status=i32(1), n_ka=i32(1), actions=i32(n_peers))
        stream.synchronize()

        # 1. A: no keypair, so the job is refused and a handshake started; the initiation's destination is the UAPI's row
        router.route_dst_batch(dev, job0.d_arena, job0.d_sizes, A["image"], job0.d_peer, stride=SLOT, offset=16, stream=stream,
                               n=1)
        rekey.send_gate_batch(dev, job0.d_peer, job0.d_count, job0.d_status_in, 1, NOW, A["rows"], A["kp"], A["nonce"], LIMIT,
                              A["rekey"], job0.d_status, stream=stream, n_jobs=1, n_ids=n_ids, n_peers=n_peers, n_keys=n_keys)
        rekey.start_batch(dev, NOW, A["rekey"], A["hs_peers"], A["tickets"], att["start"], att["start_peer"], att["count"],
                          att["status"], att["reasons"], d_work, stream=stream, n_peers=n_peers, n_tickets=1)
        noise.initiate_batch(dev, att["start"], A["pub"], A["table"], d_states, att["msgs"], att["init_status"], n_keys,
                             stream=stream, n=1, n_peers=n_peers, n_states=1)
        ep.dst_initiated_batch(dev, att["start"], att["init_status"], A["ep"], A["timers"], oI["dst"], oI["v6"], oI["status"],
                               stream=stream, n=1, n_peers=n_peers)
        # 2. B: split -> endpoint_recv -> classify -> screen (under load) -> ratelimit -> consume -> accept -> set_accepted
        #       -> respond -> dst_responded -> begin-responder
        d_land[:148].copy_(att["msgs"][:148])
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d_land.data_ptr(), SLOT, SLOT, d_n_in1.data_ptr(), d_gso1.data_ptr(), n1,
                                               first, 1, d_arena_b1.data_ptr(), SLOT, d_n_out1.data_ptr(), d_from1.data_ptr(),
                                               d_count1.data_ptr(), d_split1.data_ptr(), stream.cuda_stream)
        assert rc == 0
        ep.recv_batch(dev, d_addr1, d_from1, d_n_out1, d_oob1, OOB, d_nn1, n1, 1, d_ep1, d_addr_out1, stream=stream)
        router.classify_batch(dev, d_arena_b1, d_n_out1, B["slots"], d_pkts_b1, d_type_b1, stride=SLOT, stream=stream, n=n1,
                              n_slots=len(b_slots))
        cookie.screen_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, B["checker"], d_addr_out1, d_screen, under_load=True,
                            nonce=d_nonce, reply=d_reply, stream=stream, n=n1)
        rl.allow_batch(dev, d_screen, d_addr_out1, B["rl"], NOW, d_limited, d_rl_work, stream=stream, n=n1, n_slots=64)
        noise.consume_batch(dev, d_arena_b1, d_pkts_b1, d_type_b1, d_limited, B["self"], B["table"], d_consumed, d_hs_init,
                            stream=stream, n=n1, n_peers=n_peers)
        noise.accept_batch(dev, d_hs_init, d_consumed, NOW, B["table"], B["rows"], B["hs_peers"], B["tickets"], d_resp, d_n_resp,
                           d_accept, stream=stream, n=n1, n_ids=n_ids, n_peers=n_peers, n_tickets=1)
        ep.set_accepted_batch(dev, d_resp, d_ep1, B["ep"], B["claim"], B["timers"], stream=stream, n_tickets=1, n_rows=n1,
                              n_peers=n_peers)
        noise.respond_batch(dev, d_resp, d_hs_init, None, B["table"], None, B["keys"], d_resp_msgs, d_resp_status, stream=stream,
                            n=1, n_init=n1, n_peers=n_peers, n_keys=n_keys)
        ep.dst_responded_batch(dev, d_resp, d_resp_status, B["ep"], B["timers"], oR["dst"], oR["v6"], oR["status"],
                               stream=stream, n=1, n_peers=n_peers)
        keypairs.begin_responder_batch(dev, d_resp, d_resp_status, NOW, B["table"], B["kp"], B["slots"], B["peer_keys"],
                                       B["keys"], B["key_peer"], d_begun_b, d_work, stream=stream, n=1, n_peers=n_peers,
                                       n_slots=len(b_slots), n_peer_slots=len(b_peer_keys), n_keys=n_keys)
        # 3. A: endpoint_recv -> classify -> finish -> set_finished -> begin-initiator; then its first job
        d_arena_a1[:92].copy_(d_resp_msgs[:92])
        ep.recv_batch(dev, d_addr_a, None, d_size_a1, d_oob_a, OOB, d_nn_a, 1, 1, d_ep_a, None, stream=stream)
        router.classify_batch(dev, d_arena_a1, d_size_a1, A["slots"], d_pkts_a1, d_type_a1, stride=SLOT, stream=stream, n=1,
                              n_slots=len(a_slots))
        noise.finish_batch(dev, d_arena_a1, d_pkts_a1, d_type_a1, None, A["self"], A["hs_slots"], d_states, None, A["keys"],
                           d_fwork, d_finished, stream=stream, n=1, n_slots=len(a_hs_slots), n_states=1, n_peers=n_peers,
                           n_keys=n_keys)
        ep.set_finished_batch(dev, d_arena_a1, d_pkts_a1, d_finished, A["hs_slots"], d_states, d_ep_a, A["ep"], A["claim"],
                              A["timers"], stream=stream, n=1, n_hs_slots=len(a_hs_slots), n_states=1, n_peers=n_peers)
        keypairs.begin_initiator_batch(dev, d_arena_a1, d_pkts_a1, d_finished, NOW, A["hs_slots"], d_states, A["table"], A["kp"],
                                       A["slots"], A["peer_keys"], A["keys"], A["key_peer"], d_begun_a, d_work, stream=stream,
                                       n=1, n_hs_slots=len(a_hs_slots), n_states=1, n_peers=n_peers, n_slots=len(a_slots),
                                       n_peer_slots=len(a_peer_keys), n_keys=n_keys)
        send(A, jobA1, NOW, oA1)
        # 4. B: the coalesced message's two packets arrive, the first from A0 and the second from A1
        d_arena2[:96].copy_(jobA1.d_arena[:96])
        d_arena2[SLOT:SLOT + 96].copy_(jobA1.d_arena[96:192])
        receive(d_arena2, 2, d_addr2, d_oob2, d_nn2, NOW, r2)
        send(B, jobB1, NOW, oB1, with_timers=True)  # data sent arms newHandshake
        # 5. B: 16 s later newHandshake fires: the next job's source is empty; a packet received afterwards restores it
        timers.expire_batch(dev, T2, B["timers"], B["rekey"], B["table"], None, B["kp"], B["slots"], B["peer_keys"], B["keys"],
                            B["key_peer"], exp["ka_peer"], exp["ka_count"], exp["ka_sizes"], exp["ka_status"], exp["n_ka"],
                            exp["actions"], d_work, stream=stream, n_peers=n_peers, n_slots=len(b_slots),
                            n_peer_slots=len(b_peer_keys), n_keys=n_keys, n_ka_max=1)
        d_flags_marked = B["timers"].clone()
        send(B, jobB2, T2, oB2)
        d_ep_cleared = B["ep"].clone()
        d_flags_cleared = B["timers"].clone()
        send(A, jobA2, T2, oA2)
        d_arena3[:96].copy_(jobA2.d_arena[:96])
        receive(d_arena3, 1, d_addr3, d_oob3, d_nn3, T2, r3)
        # 6. B: a job for the peer that never had an endpoint
        send(B, jobC, T2, oC)
        stream.synchronize()  # the only one since the chains began

    down = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    row = lambda t, i=0: down(t, ep.ENDPOINT_DTYPE)[i].tobytes()  # noqa: E731
    want = lambda dst, src: ep.row(dst[:-2], int.from_bytes(dst[-2:], "little"), src)[0].tobytes()  # noqa: E731
    tflags = lambda t, r: int(down(t, timers.TIMERS_DTYPE)["flags"][r])  # noqa: E731
    # 1. refused, initiated, addressed to the UAPI's endpoint
    assert job0.d_status.cpu().tolist() == [ERR_KEY_EXPIRED] and att["init_status"].cpu().tolist() == [HS_INITIATED]
    assert row(oI["dst"]) == want(B0, b"") and oI["v6"].cpu().tolist() == [0] and oI["status"].cpu().tolist() == [0]
    # 2. the split carried slot 2's message and address to slot 0, which keeps its own control buffer
    assert d_count1.cpu().tolist() == [1] and d_split1.cpu().tolist() == [0]
    assert d_n_out1.cpu().tolist() == [148, 0, 0, 0] and d_from1.cpu().tolist()[0] == 2
    h_ep1, h_out1 = ep.recv_host(addr1, down(d_from1, np.int32), down(d_n_out1, np.int32), oob1, OOB, nn1, n1, 1)
    assert down(d_ep1, np.uint8).tobytes() == h_ep1.tobytes() and down(d_addr_out1, np.uint8).tobytes() == h_out1.tobytes()
    assert row(d_ep1) == want(A0, S0) and not down(d_ep1, np.uint8)[64:].any()
    assert d_type_b1.cpu().tolist()[0] == 1 and d_screen.cpu().tolist()[0] == HS_PASS  # MAC2 holds for the cookie of A0
    assert d_limited.cpu().tolist()[0] == HS_PASS and d_accept.cpu().tolist()[0] == noise.HS_ACCEPTED
    assert len(rl.entries(down(B["rl"], rl.RL_ENTRY_DTYPE))) == 1
    assert d_resp_status.cpu().tolist() == [HS_RESPONDED] and d_begun_b.cpu().tolist() == [HS_BEGUN]
    assert row(oR["dst"]) == want(A0, S0) and oR["status"].cpu().tolist() == [0]  # to the initiation's source
    # 3. A learnt the sticky source the response arrived on, and its job goes to B0 as one IPv4 message
    assert d_finished.cpu().tolist() == [HS_FINISHED] and d_begun_a.cpu().tolist() == [HS_BEGUN]
    assert row(A["ep"], a_pr) == want(B0, S_A) and not down(A["claim"], np.uint32).any()
    assert row(oA1["dst"]) == want(B0, S_A) and oA1["v6"].cpu().tolist() == [0, MARK] and oA1["status"].cpu().tolist() == [0, MARK]
    assert jobA1.d_out_len.cpu().tolist() == [96, 96] and oA1["tx"].cpu().tolist() == [192, -1]
    assert (oA1["nm"].item(), oA1["first"].cpu().tolist()[0], oA1["mlen"].cpu().tolist()[0], oA1["gso"].cpu().tolist()[0]) == (1, 0, 192, 96)
    # 4. B roamed with A: both packets are valid, the tail's endpoint stands, and the next job goes there as IPv6
    assert min(r2["verdict"].cpu().tolist()) > 0 and r2["n_groups"].cpu().tolist() == [1]
    g2 = down(r2["groups"], WRITE_GROUP_DTYPE)[0]
    assert (int(g2["peer"]), int(g2["tail"]), int(g2["n_valid"])) == (a_at_b, 1, 2)
    assert row(oB1["dst"]) == want(A1, S1) and oB1["v6"].cpu().tolist()[0] == 1 and oB1["status"].cpu().tolist()[0] == 0
    assert (oB1["nm"].item(), oB1["mlen"].cpu().tolist()[0], oB1["gso"].cpu().tolist()[0]) == (1, 192, 96)
    # 5. newHandshake fired and marked the source; the job after it has none, nor has the table; the packet restores it
    assert tflags(d_flags_marked, b_pr) == ACTIVE | CLEAR_SRC and down(exp["actions"], np.uint32)[b_pr] & 1
    assert row(oB2["dst"]) == want(A1, b"") and oB2["v6"].cpu().tolist()[0] == 1 and oB2["status"].cpu().tolist()[0] == 0
    assert row(d_ep_cleared, b_pr) == want(A1, b"") and tflags(d_flags_cleared, b_pr) == ACTIVE
    assert oB2["nm"].item() == 1 and r3["verdict"].cpu().tolist()[0] > 0
    assert row(B["ep"], b_pr) == want(A1, S1) and tflags(B["timers"], b_pr) & CLEAR_SRC == 0
    # 6. no known endpoint for peer: no message, and the nonce is spent
    assert jobC.d_out_len.cpu().tolist() == [96] and down(jobC.d_job_key, np.uint32).tolist() == [4]
    assert oC["status"].cpu().tolist() == [ERR_NO_ENDPOINT] and not down(oC["dst"], np.uint8).any()
    assert jobC.d_nbufs.cpu().tolist() == [0] and oC["nm"].item() == 0 and oC["tx"].cpu().tolist() == [0]
    assert down(B["nonce"], np.uint64)[4] == 1
    # the tables at the end: B knows A alone, no claim is left
    h_b = down(B["ep"], ep.ENDPOINT_DTYPE)
    assert not np.delete(h_b, b_pr).view(np.uint8).any() and not down(B["claim"], np.uint32).any()
