"""The rate limiter in its place in the responder's chain, on one stream with
nothing read back in between:

wgcs_split_messages_batch -> wgcs_recv_classify_batch -> wgcs_handshake_screen_batch
(under_load = 1) -> wgcs_ratelimit_batch -> wgcs_handshake_consume_batch ->
wgcs_handshake_accept_batch -> wgcs_handshake_respond_batch

Eight authentic initiations with a valid MAC2 come from one source address in
one UDP-GRO run, each for a different peer (so that accept's per-peer flood
rule stays out of it), two from a second address, and one more carries a MAC2
made from another address's cookie.  The burst lets five of the eight through:
5 + 2 responses, three rows WGCS_ERR_RATE_LIMITED, one cookie reply.  The same
chain again 100 ms later lets exactly two more rows of the first address
through.  Every expectation is computed by the host forms and the restatements."""
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cookie_ref
import noise_accept_cases as cases
import noise_ref
from noise_accept_cases import NOW, T
from noise_accept_ref import HS_ACCEPTED, HS_CONSUMED
from noise_ref import ERR_INVALID_ARG, HS_NONE
from noise_resp_ref import HS_RESPONDED
from ratelimit_cases import COST, check_reachable
from test_gpu_cookie import SENTINEL, src_row, up
from wireguard_amd import cookie, noise, ratelimit as rl, router
from wireguard_amd.cookie import HS_COOKIE, HS_PASS
from wireguard_amd.noise import HS_INIT_DTYPE, HS_RESP_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

PITCH = 96
LIMITED = rl.ERR_RATE_LIMITED


def test_one_stream_chain_with_the_rate_limiter_between_screen_and_consume(dev):
    import path_ref
    from path_ref import FIRST_MSG_AT, MARK, N_MSGS

    rng = np.random.default_rng(2810)
    private = rng.bytes(32)
    responder, public = noise.responder_init(private)
    checker = cookie_ref.Checker(public, rng.bytes(32))
    src = dict(a=cookie_ref.src_bytes(bytes([203, 0, 113, 5]), 40001), b=cookie_ref.src_bytes(bytes.fromhex("20010db8" + "00" * 11 + "09"), 7),
               c=cookie_ref.src_bytes(bytes([203, 0, 113, 6]), 40001))
    names = [f"a{i}" for i in range(8)] + ["b0", "b1", "c"]
    ini = {}
    for i, k in enumerate(names):
        p = SimpleNamespace(private=rng.bytes(32), eph=rng.bytes(32), index=int(rng.integers(0, 2**32)), ts=T[1 + i % 3])
        p.public = noise_ref.public_key(p.private)
        msg = noise.create_initiation(p.private, public, p.eph, p.ts, p.index)[0]
        # MAC2 from the cookie of the address the message comes from; c's is made from a's cookie
        p.msg = cookie_ref.add_macs(checker.mac1_key, msg, checker.cookie(src["a" if k == "c" else k[0]]))[0]
        ini[k] = p
    n_ids = 40
    table = noise.peer_keys_build(responder, [ini[k].public for k in names], list(range(20, 20 + len(names))))
    n_peers = len(table)
    peer_rows = noise.peer_rows_build(table, n_ids)
    psk = np.zeros((n_peers, 32), np.uint8)
    peers = cases.peers_of(n_peers, seed=2811)
    peers["flags"] = 0

    s = path_ref.scenario(20261021, 4112, 4099)
    nb, stride, per = 2, s.stride, N_MSGS - FIRST_MSG_AT
    pitch, n = per * s.in_stride, 2 * N_MSGS
    land = np.full(nb * pitch, path_ref.LAND_SENTINEL, np.uint8)
    n_in, gso = np.zeros(n, np.int32), np.zeros(n, np.int32)
    batches = [([b"".join(ini[f"a{i}"].msg for i in range(8)), ini["b0"].msg + ini["b1"].msg], [148, 148], ["a", "b"]),
               ([ini["c"].msg, struct.pack("<I", 3) + rng.bytes(60)], [0, 0], ["c", "b"])]
    for b, (datagrams, sizes, _) in enumerate(batches):
        for k, (dg, g) in enumerate(zip(datagrams, sizes)):
            at = b * pitch + k * s.in_stride
            land[at:at + len(dg)] = np.frombuffer(dg, np.uint8)
            n_in[b * N_MSGS + FIRST_MSG_AT + k], gso[b * N_MSGS + FIRST_MSG_AT + k] = len(dg), g
    want = path_ref.recv_ref(s, land, n_in, gso)
    # the source of row q is the address of the datagram the split cuts it from
    srcs, nonces = [], [rng.bytes(24) for _ in range(n)]
    for q in range(n):
        b, k = divmod(q, N_MSGS)
        origin = int(want.src[q]) if want.src[q] >= 0 else k
        srcs.append(src[batches[b][2][max(origin - FIRST_MSG_AT, 0)]])
    src_rows = np.concatenate([src_row(x) for x in srcs])
    msgs_of = {q: want.arena_split[q * stride:q * stride + int(want.pkts["len"][q])].tobytes()
               for q in range(n) if want.type[q] in (1, 2)}
    rows = {k: next(q for q, m in msgs_of.items() if m == p.msg) for k, p in ini.items()}
    assert sorted(rows.values()) == sorted(msgs_of) and [rows[f"a{i}"] for i in range(8)] == sorted(rows[f"a{i}"] for i in range(8))
    screen = np.zeros(n, np.int32)
    reply = np.full(64 * n, SENTINEL, np.uint8)
    for q in range(n):
        v, r = cookie_ref.screen(checker, int(want.type[q]), msgs_of.get(q), srcs[q], True, nonces[q])
        screen[q] = v
        if r is not None:
            reply[64 * q:64 * q + 64] = np.frombuffer(r, np.uint8)
    assert (screen == HS_PASS).sum() == 10 and (screen == HS_COOKIE).sum() == 1 and screen[rows["c"]] == HS_COOKIE

    n_tickets = 9
    n_keys = 2 * n_tickets + 2

    def host_pass(tab, hs_peers, now, tickets):
        w = SimpleNamespace(stats=np.zeros(4, np.uint32))
        w.limited = rl.allow_host(screen, src_rows, tab, now, stats=w.stats)
        w.consumed = np.zeros(n, np.int32)
        w.init = np.full(n, 0xEE, np.uint8).repeat(128).view(HS_INIT_DTYPE)
        for q in range(n):
            if want.type[q] == 1 and w.limited[q] == HS_PASS:
                w.consumed[q], row = noise.consume_initiation(responder, table, msgs_of[q])
                w.init[q] = row[0]
        w.resp = np.zeros(n_tickets, HS_RESP_DTYPE)
        w.count, w.verdict = np.zeros(1, np.uint32), np.zeros(n, np.int32)
        noise.accept_host(w.init, w.consumed, now, table, peer_rows, hs_peers, tickets, w.resp, w.count, w.verdict)
        return w

    def device_pass(d, now, d_tickets):
        o = SimpleNamespace()
        i32 = lambda m, fill=MARK: torch.full((m,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
        o.arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
        o.n_out, o.frm, o.count, o.split_status = i32(n), i32(n), i32(nb), i32(nb)
        o.pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        o.type, o.screen, o.limited, o.consumed, o.verdict = i32(n), i32(n), i32(n), i32(n), i32(n)
        o.reply = torch.full((64 * n,), SENTINEL, dtype=torch.uint8, device="cuda")
        o.stats = torch.full((4,), 0x6E6E6E6E, dtype=torch.int32, device="cuda")
        o.init = torch.full((128 * n,), 0xEE, dtype=torch.uint8, device="cuda")
        o.resp = torch.full((80 * n_tickets,), SENTINEL, dtype=torch.uint8, device="cuda")
        o.n_resp, o.status = i32(1), i32(n_tickets)
        o.keys = torch.full((48 * n_keys,), 0xC3, dtype=torch.uint8, device="cuda")
        o.msgs = torch.full((PITCH * n_tickets,), SENTINEL, dtype=torch.uint8, device="cuda")
        stream = d.stream
        stream.synchronize()
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d.land.data_ptr(), s.in_stride, s.buf_len, d.n_in.data_ptr(),
                                               d.gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, o.arena.data_ptr(), stride,
                                               o.n_out.data_ptr(), o.frm.data_ptr(), o.count.data_ptr(),
                                               o.split_status.data_ptr(), stream.cuda_stream)
        assert rc == 0
        router.classify_batch(dev, o.arena, o.n_out, d.slots, o.pkts, o.type, stride=stride, stream=stream, n=n,
                              n_slots=len(s.slots))
        cookie.screen_batch(dev, o.arena, o.pkts, o.type, d.checker, d.src, o.screen, under_load=True, nonce=d.nonce,
                            reply=o.reply, stream=stream, n=n)
        rl.allow_batch(dev, o.screen, d.src, d.tab, now, o.limited, d.work, stats=o.stats, stream=stream, n=n,
                       n_slots=64)
        noise.consume_batch(dev, o.arena, o.pkts, o.type, o.limited, d.responder, d.table, o.consumed, o.init,
                            stream=stream, n=n, n_peers=n_peers)
        noise.accept_batch(dev, o.init, o.consumed, now, d.table, d.peer_rows, d.peers, d_tickets, o.resp, o.n_resp,
                           o.verdict, stream=stream, n=n, n_ids=n_ids, n_peers=n_peers, n_tickets=n_tickets)
        noise.respond_batch(dev, o.resp, o.init, None, d.table, d.psk, o.keys, o.msgs, o.status, stream=stream,
                            n=n_tickets, n_init=n, n_peers=n_peers, n_keys=n_keys)
        return o

    def compare(o, w):
        host = lambda t, dtype=None: t.cpu().numpy() if dtype is None else t.cpu().numpy().view(dtype)  # noqa: E731
        assert np.array_equal(host(o.type), want.type)
        assert np.array_equal(host(o.screen), screen) and np.array_equal(host(o.reply), reply)
        assert np.array_equal(host(o.limited), w.limited)
        assert host(o.stats, np.uint32).tolist() == w.stats.tolist()
        assert np.array_equal(host(o.consumed), w.consumed)
        assert host(o.init).tobytes() == w.init.tobytes()
        assert np.array_equal(host(o.verdict), w.verdict) and host(o.n_resp).item() == w.count[0]
        assert host(o.resp).tobytes() == w.resp.tobytes()
        return host(o.status)

    tab, hs_peers = rl.table(64), peers.copy()
    tickets = [cases.tickets_of(n_tickets, seed=2812), cases.tickets_of(n_tickets, seed=2813)]
    w1 = host_pass(tab, hs_peers, NOW, tickets[0])
    a_rows = [rows[f"a{i}"] for i in range(8)]
    assert w1.limited[a_rows].tolist() == [HS_PASS] * 5 + [LIMITED] * 3 and (w1.limited == LIMITED).sum() == 3
    assert w1.limited[rows["b0"]] == w1.limited[rows["b1"]] == HS_PASS and w1.limited[rows["c"]] == HS_COOKIE
    assert (w1.consumed == HS_CONSUMED).sum() == 7 and (w1.verdict == HS_ACCEPTED).sum() == 7 and w1.count[0] == 7
    assert (w1.consumed[a_rows[5:]] == HS_NONE).all()  # a refused row never reaches the Noise code
    assert w1.stats.tolist() == [7, 3, 0, 2]
    peers_after_1 = hs_peers.copy()
    w2 = host_pass(tab, hs_peers, NOW + 2 * COST, tickets[1])
    assert w2.limited[a_rows].tolist() == [HS_PASS] * 2 + [LIMITED] * 6  # exactly two more of the first address
    assert w2.limited[rows["b0"]] == w2.limited[rows["b1"]] == HS_PASS and w2.stats.tolist() == [4, 6, 0, 0]

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = SimpleNamespace(stream=stream, land=up(land), n_in=torch.from_numpy(n_in).cuda(), gso=torch.from_numpy(gso).cuda(),
                            slots=up(s.slots), checker=up(np.frombuffer(checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE)),
                            src=up(src_rows), nonce=up(np.frombuffer(b"".join(nonces), np.uint8)), responder=up(responder),
                            table=up(table), psk=up(psk), peer_rows=up(peer_rows), peers=up(peers), tab=up(rl.table(64)),
                            work=torch.full((rl.work_bytes(n),), 0x77, dtype=torch.uint8, device="cuda"))
        d_tickets = [up(t) for t in tickets]
        o1 = device_pass(d, NOW, d_tickets[0])
        stream.synchronize()
        status = compare(o1, w1)
        assert status.tolist() == [HS_RESPONDED] * 7 + [ERR_INVALID_ARG] * 2
        assert d.peers.cpu().numpy().tobytes() == peers_after_1.tobytes()
        o2 = device_pass(d, NOW + 2 * COST, d_tickets[1])
        stream.synchronize()
        compare(o2, w2)
    got_tab = d.tab.cpu().numpy().view(rl.RL_ENTRY_DTYPE)
    check_reachable(got_tab)
    assert rl.entries(got_tab) == rl.entries(tab) and len(rl.entries(tab)) == 2
    assert d.peers.cpu().numpy().tobytes() == hs_peers.tobytes()
