"""The device-resident handshake response on the GPU
(wgcs_handshake_respond_batch, hs_respond_kernel of noise_kernels.hip).

Message rows, the whole key table and the status array are compared byte for
byte with the host function wgcs_noise_create_response, which
tests/test_noise_resp_host.py and tests/test_noise_resp_ref.py pin to
tests/noise_resp_ref.py; every output is filled with a sentinel first and is
longer than the batch, so the rows and key slots that must stay untouched are
compared too.  The chain test runs split -> classify -> screen -> consume ->
respond -> seal on one stream and lets the restatement's initiator finish the
handshakes."""
import functools
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import aead_ref
import cookie_ref
import noise_ref
import noise_resp_ref
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, ERR_NO_PEER, HS_CONSUMED, HS_NONE, HS_PASS, LOW_ORDER_POINTS
from noise_resp_ref import HS_RESPONDED
from test_gpu_cookie import SENTINEL, flip, up
from wireguard_amd import _lib, cookie, noise, router, transport
from wireguard_amd.noise import HS_INIT_DTYPE, HS_RESP_DTYPE, PEER_KEY_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

N_PEERS = 37
STATUS_FILL = 12345
SPARE = 3           # rows of d_msgs / d_status and key slots past the batch: they keep their fill
PITCH = 96


def le(n: int) -> bytes:
    return n.to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def world():
    """A responder, 37 peers -- one whose public key is a low-order point among
    them --, their preshared keys, and a table of wgcs_hs_init rows with its
    gate: consumed initiations of several peers, rows that consume turned away,
    rows whose remote ephemeral is a low-order point, and a consumed row of the
    low-order peer."""
    rng = np.random.default_rng(494)
    w = SimpleNamespace(rng=rng)
    w.private = rng.bytes(32)
    w.responder, w.public = noise.responder_init(w.private)
    privs = [rng.bytes(32) for _ in range(N_PEERS - 1)]
    pubs = [noise.x25519(k, noise_ref.BASE_POINT) for k in privs]
    w.low_peer = 99
    w.table = noise.peer_keys_build(w.responder, pubs + [le(1)], [100 + i for i in range(N_PEERS - 1)] + [w.low_peer])
    assert len(w.table) == N_PEERS
    w.row_of_peer = {int(r["peer"]): i for i, r in enumerate(w.table)}
    w.psk = np.frombuffer(rng.bytes(32 * N_PEERS), np.uint8).reshape(N_PEERS, 32).copy()
    w.psk[::5] = 0  # peers without a preshared key among them
    init, gate, kind = [], [], []

    def consumed(i):
        msg = noise.create_initiation(privs[i], w.public, rng.bytes(32), rng.bytes(12), int(rng.integers(0, 2**32)))[0]
        v, row = noise.consume_initiation(w.responder, w.table, msg)
        assert v == HS_CONSUMED and int(row["peer"][0]) == 100 + i
        return row

    for i in (0, 1, 7, 18, 35, 35, 2):
        init.append(consumed(i)); gate.append(HS_CONSUMED); kind.append("good")
    for v in (ERR_AUTH, HS_NONE, HS_PASS, ERR_NO_PEER):  # rows the consume step or the host's rules turned away
        init.append(consumed(3)); gate.append(v); kind.append("gated")
    for u in LOW_ORDER_POINTS:
        row = consumed(4)
        row["ephemeral"][0] = np.frombuffer(u, np.uint8)
        init.append(row); gate.append(HS_CONSUMED); kind.append("low_eph")
    row = consumed(5)
    row["peer"] = w.low_peer  # what a consumed initiation of that peer would hold: its static key gives a zero secret
    init.append(row); gate.append(HS_CONSUMED); kind.append("low_static")
    w.init = np.concatenate(init)
    w.gate, w.kind = np.array(gate, np.int32), kind
    w.rows_of_kind = {k: [i for i, x in enumerate(kind) if x == k] for k in set(kind)}
    return w


@functools.lru_cache(maxsize=None)
def batch(n):
    """n descriptors that meet every row of the status table, with key rows 2j and 2j + 1."""
    w = world()
    rng = np.random.default_rng(3000 + n)
    n_init, n_keys = len(w.init), 2 * n + SPARE
    d = np.zeros(n, HS_RESP_DTYPE)
    good = w.rows_of_kind["good"]
    for j in range(n):
        k = j % 16 if n > 1 else 0
        i = good[j % len(good)]
        d["send_key"][j], d["recv_key"][j] = 2 * j, 2 * j + 1
        d["flags"][j] = j & 1 if k != 1 else 0xFFFFFFFE | (j >> 4 & 1)  # only bit 0 means anything
        if k == 8:
            i = (n_init, 0xFFFFFFFF, n_init + 7)[(j // 16) % 3]
        elif k == 9:
            d["send_key"][j] = (n_keys, 0xFFFFFFFF)[(j // 16) % 2]
        elif k == 10:
            d["recv_key"][j] = (n_keys, 0x80000000)[(j // 16) % 2]
        elif k == 11:
            d["recv_key"][j] = d["send_key"][j]
        elif k == 12:
            i = w.rows_of_kind["gated"][(j // 16) % 4]
        elif k == 13:
            i = w.rows_of_kind["low_eph"][(j // 16) % 5]
        elif k == 14:
            i = w.rows_of_kind["low_static"][0]
        d["init_row"][j] = i
        peer = w.row_of_peer[int(w.init["peer"][i])] if i < n_init else 0
        if k == 7:
            peer = (peer + 1 + (j // 16)) % N_PEERS  # another peer's row
        elif k == 15:
            peer = (N_PEERS, 0xFFFFFFFF)[(j // 16) % 2]
        d["peer_row"][j] = peer
        d["local_index"][j] = int(rng.integers(0, 2**32))
        d["ephemeral_private"][j] = np.frombuffer(rng.bytes(32), np.uint8)
        d["cookie"][j] = np.frombuffer(rng.bytes(16), np.uint8)
        d["pad"][j] = int(rng.integers(0, 2**32))  # not looked at
    return d, n_keys


@functools.lru_cache(maxsize=None)
def expect(n, use_gate, psk_mode):
    """(status, msgs, keys) as arrays with their fill, through wgcs_noise_create_response."""
    w = world()
    d, n_keys = batch(n)
    n_init = len(w.init)
    status = np.full(n + SPARE, STATUS_FILL, np.int32)
    msgs = np.full(PITCH * (n + SPARE), SENTINEL, np.uint8)
    keys = np.full(n_keys * 48, SENTINEL, np.uint8).view(AEAD_KEY_DTYPE)
    for j in range(n):
        i, p, s, r = (int(d[f][j]) for f in ("init_row", "peer_row", "send_key", "recv_key"))
        if i >= n_init or p >= N_PEERS or s >= n_keys or r >= n_keys or s == r:
            status[j] = ERR_INVALID_ARG
        elif use_gate and w.gate[i] != HS_CONSUMED:
            status[j] = HS_NONE
        elif w.init["peer"][i] != w.table["peer"][p]:
            status[j] = ERR_NO_PEER
        else:
            psk = w.psk[p].tobytes() if psk_mode == "random" else None
            cookie_ = d["cookie"][j].tobytes() if d["flags"][j] & 1 else None
            rc, msg, send, recv = noise.create_response(w.init[i:i + 1], w.table["public_key"][p].tobytes(),
                                                        d["ephemeral_private"][j].tobytes(), int(d["local_index"][j]),
                                                        psk, cookie_)
            msgs[PITCH * j:PITCH * (j + 1)] = np.frombuffer(msg + bytes(4), np.uint8)
            if rc == 0:
                status[j] = HS_RESPONDED
                keys[s] = (np.frombuffer(send, np.uint8), w.init["sender"][i], 0)
                keys[r] = (np.frombuffer(recv, np.uint8), 0, 0)
            else:
                assert rc == ERR_LOW_ORDER and not any(msg)
                status[j] = rc
    return status, msgs, keys.view(np.uint8).reshape(-1)


def run_respond(dev, n, use_gate, psk_mode, stream=None):
    w = world()
    d, n_keys = batch(n)
    d_resp, d_init, d_gate, d_table = up(d), up(w.init), up(w.gate), up(w.table)
    d_psk = {"null": None, "zero": torch.zeros(32 * N_PEERS, dtype=torch.uint8, device="cuda"),
             "random": up(w.psk)}[psk_mode]
    d_keys = torch.full((48 * n_keys,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_msgs = torch.full((PITCH * (n + SPARE),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + SPARE,), STATUS_FILL, dtype=torch.int32, device="cuda")
    noise.respond_batch(dev, d_resp, d_init, d_gate if use_gate else None, d_table, d_psk, d_keys, d_msgs, d_status,
                        stream=stream, n=n, n_init=len(w.init), n_peers=N_PEERS, n_keys=n_keys)
    torch.cuda.synchronize()
    for t, a, what in ((d_resp, d, "d_resp"), (d_init, w.init, "d_init"), (d_table, w.table, "d_table")):
        assert t.cpu().numpy().tobytes() == a.tobytes(), f"the respond step wrote {what}"
    return d_status.cpu().numpy(), d_msgs.cpu().numpy(), d_keys.cpu().numpy()


def check(got, want, n):
    (status, msgs, keys), (want_status, want_msgs, want_keys) = got, want
    bad = np.flatnonzero(status != want_status)
    assert len(bad) == 0, f"{len(bad)} statuses differ, first at row {bad[0]}: got {status[bad[0]]}, want {want_status[bad[0]]}"
    bad = np.flatnonzero(msgs != want_msgs)
    assert len(bad) == 0, f"d_msgs differs, first in row {bad[0] // PITCH} at byte {bad[0] % PITCH}"
    bad = np.flatnonzero(keys != want_keys)
    assert len(bad) == 0, f"d_keys differs, first in key row {bad[0] // 48} at byte {bad[0] % 48}"


@pytest.mark.parametrize("n", [1, 65, 257])
def test_respond_batch_matches_the_host_function(dev, n):
    d, n_keys = batch(n)
    want = expect(n, True, "random")
    got = run_respond(dev, n, True, "random")
    check(got, want, n)
    status, msgs, keys = got
    for j in range(n):  # what the table of include/wgcsum.h promises, row by row
        row, ks = msgs[PITCH * j:PITCH * (j + 1)], [keys[48 * k:48 * k + 48] for k in (2 * j, 2 * j + 1)]
        if status[j] == HS_RESPONDED:
            assert not row[92:].any() and row[76:92].any() == bool(d["flags"][j] & 1)
            assert ks[0][:32].any() and ks[1][:32].any() and not ks[0][36:].any() and not ks[1][32:].any()
        else:
            assert all((k == SENTINEL).all() for k in ks), "a failing row wrote key material"
            assert (row == (0 if status[j] == ERR_LOW_ORDER else SENTINEL)).all()
    if n == 1:
        assert status[0] == HS_RESPONDED
    if n == 257:
        w = world()
        for v in (HS_RESPONDED, HS_NONE, ERR_INVALID_ARG, ERR_NO_PEER, ERR_LOW_ORDER):
            assert (status[:n] == v).any(), v
        low = [j for j in range(n) if status[j] == ERR_LOW_ORDER]
        kinds = {w.kind[int(d["init_row"][j])] for j in low}
        assert kinds == {"low_eph", "low_static"}
        assert {int(d["init_row"][j]) for j in low} >= set(w.rows_of_kind["low_eph"])  # each of LOW_ORDER_POINTS
        responded = np.flatnonzero(status[:n] == HS_RESPONDED)
        assert {int(d["flags"][j]) & 1 for j in responded} == {0, 1}
        assert any(int(d["flags"][j]) > 1 for j in responded)
        psk_rows = {bool(w.psk[int(d["peer_row"][j])].any()) for j in responded}
        assert psk_rows == {False, True}


@pytest.mark.parametrize("n", [65, 257])
def test_null_gate_takes_every_descriptor_and_null_psk_is_the_zero_table(dev, n):
    w = world()
    d, _ = batch(n)
    want = expect(n, False, "null")
    got = run_respond(dev, n, False, "null")
    check(got, want, n)
    gated = [j for j in range(n) if int(d["init_row"][j]) in w.rows_of_kind["gated"]]
    assert gated and (got[0][gated] == HS_RESPONDED).all()
    check(run_respond(dev, n, False, "zero"), want, n)
    with_gate = run_respond(dev, n, True, "zero")
    check(with_gate, expect(n, True, "null"), n)
    assert (with_gate[0][gated] == HS_NONE).all()
    # a preshared key changes the message and the keys of the peers that have one
    assert not np.array_equal(expect(n, True, "random")[1], expect(n, True, "null")[1])


def test_respond_batch_arguments(dev):
    w = world()
    n = 65
    d, n_keys = batch(n)
    d_resp, d_init, d_gate, d_table, d_psk = up(d), up(w.init), up(w.gate), up(w.table), up(w.psk)
    d_keys = torch.full((48 * n_keys,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_msgs = torch.full((PITCH * (n + SPARE),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + SPARE,), STATUS_FILL, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(resp=d_resp, init=d_init, gate=d_gate, table=d_table, psk=d_psk, keys=d_keys, msgs=d_msgs,
                 status=d_status, n=n, n_init=len(w.init), n_peers=N_PEERS, n_keys=n_keys)
        a.update(kw)
        noise.respond_batch(dev, **a)

    call(n=0)  # a no-op
    call(n=0, resp=None, msgs=None, status=None)
    cases = [dict(resp=None), dict(msgs=None), dict(status=None), dict(n=(1 << 28) + 1),
             dict(resp=d_resp.data_ptr() + 2), dict(init=d_init.data_ptr() + 1), dict(gate=d_gate.data_ptr() + 2),
             dict(table=d_table.data_ptr() + 2), dict(psk=d_psk.data_ptr() + 1), dict(keys=d_keys.data_ptr() + 2),
             dict(msgs=d_msgs.data_ptr() + 1), dict(status=d_status.data_ptr() + 2)]
    for kw in cases:
        with pytest.raises(_lib.WgcsError) as ei:
            call(**kw)
        assert ei.value.code == ERR_INVALID_ARG, kw
    for k, name in ((3, "d_init"), (6, "d_table"), (9, "d_keys")):  # a table is required where its count says there is one
        args = [dev.h, d_resp.data_ptr(), n, d_init.data_ptr(), None, len(w.init), d_table.data_ptr(), None, N_PEERS,
                d_keys.data_ptr(), n_keys, d_msgs.data_ptr(), d_status.data_ptr(), None]
        args[k] = None
        assert dev.lib.wgcs_handshake_respond_batch(*args) == ERR_INVALID_ARG, name
    assert dev.lib.wgcs_handshake_respond_batch(None, d_resp.data_ptr(), n, d_init.data_ptr(), None, len(w.init),
                                                d_table.data_ptr(), None, N_PEERS, d_keys.data_ptr(), n_keys,
                                                d_msgs.data_ptr(), d_status.data_ptr(), None) == ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (d_status.cpu().numpy() == STATUS_FILL).all() and (d_msgs.cpu().numpy() == SENTINEL).all()
    assert (d_keys.cpu().numpy() == SENTINEL).all()
    # with empty tables every descriptor is out of range, and nothing is read
    call(n_init=0, init=None)
    torch.cuda.synchronize()
    assert (d_status.cpu().numpy()[:n] == ERR_INVALID_ARG).all() and (d_keys.cpu().numpy() == SENTINEL).all()


# ----------------------------------------------------------------------- chain
def test_one_stream_chain_from_split_to_the_first_sealed_packet(dev):
    """wgcs_split_messages_batch -> wgcs_recv_classify_batch -> wgcs_handshake_screen_batch ->
    wgcs_handshake_consume_batch -> (one row of its verdicts is masked, as the timestamp rule
    would) -> wgcs_handshake_respond_batch -> wgcs_aead_seal_batch under the send-key rows
    just written, all enqueued on one stream with no synchronisation between them.  The
    restatement's initiator then consumes each response, opens the sealed packet with its
    receive key and seals one back, which wgcs_aead_open_batch opens under the recv-key row."""
    import path_ref
    from path_ref import FIRST_MSG_AT, MARK, N_MSGS

    rng = np.random.default_rng(130)
    private = rng.bytes(32)
    responder, public = noise.responder_init(private)
    checker = cookie_ref.Checker(public)
    names = ["a", "b", "masked", "d"]
    ini = {k: SimpleNamespace(private=rng.bytes(32), eph=rng.bytes(32), index=int(rng.integers(0, 2**32)),
                              psk=rng.bytes(32) if k in ("a", "masked") else bytes(32)) for k in names}
    stranger = rng.bytes(32)
    for k, p in ini.items():
        p.public = noise_ref.public_key(p.private)
        p.msg, p.hash, p.chain = noise.create_initiation(p.private, public, p.eph, rng.bytes(12), p.index)
        p.msg = cookie_ref.add_macs(checker.mac1_key, p.msg)[0]
    others = [noise_ref.public_key(rng.bytes(32)) for _ in range(5)]
    table = noise.peer_keys_build(responder, [ini[k].public for k in names] + others, list(range(50, 50 + len(names) + 5)))
    n_peers = len(table)
    psk = np.zeros((n_peers, 32), np.uint8)
    for p in ini.values():
        p.peer_row = noise.peer_keys_find(table, p.public)
        psk[p.peer_row] = np.frombuffer(p.psk, np.uint8)
    # its timestamp does not open (with a MAC1 of its own, so that it passes the screen): ERR_AUTH, no response
    bad_ts = cookie_ref.add_macs(checker.mac1_key, flip(ini["a"].msg, 100))[0]
    unknown = cookie_ref.add_macs(checker.mac1_key, noise.create_initiation(stranger, public, rng.bytes(32), rng.bytes(12), 5)[0])[0]

    s = path_ref.scenario(20261020, 4112, 4099)
    nb, stride, per = 2, s.stride, N_MSGS - FIRST_MSG_AT
    pitch, n = per * s.in_stride, 2 * N_MSGS
    land = np.full(nb * pitch, path_ref.LAND_SENTINEL, np.uint8)
    n_in, gso = np.zeros(n, np.int32), np.zeros(n, np.int32)
    batches = [([ini["a"].msg + ini["b"].msg + bad_ts + ini["masked"].msg + unknown,
                 cookie_ref.handshake_message(rng, 2, checker.mac1_key)], [148, 0]),   # a UDP-GRO run, then a response
               ([ini["d"].msg, struct.pack("<I", 3) + rng.bytes(60)], [0, 0])]          # single datagrams
    for b, (datagrams, sizes) in enumerate(batches):
        for k, (dg, g) in enumerate(zip(datagrams, sizes)):
            at = b * pitch + k * s.in_stride
            land[at:at + len(dg)] = np.frombuffer(dg, np.uint8)
            n_in[b * N_MSGS + FIRST_MSG_AT + k], gso[b * N_MSGS + FIRST_MSG_AT + k] = len(dg), g
    want = path_ref.recv_ref(s, land, n_in, gso)
    row_of = {}
    for q in range(n):
        if want.type[q] == 1:
            msg = want.arena_split[q * stride:q * stride + 148].tobytes()
            row_of.update({k: q for k, p in ini.items() if p.msg == msg})
    assert sorted(row_of) == sorted(names)
    want_verdict = np.zeros(n, np.int32)
    want_init = np.full(n, 0xEE, np.uint8).repeat(128).view(HS_INIT_DTYPE)
    for q in range(n):
        if want.type[q] == 1:
            want_verdict[q], row = noise.consume_initiation(responder, table, want.arena_split[q * stride:q * stride + 148].tobytes())
            want_init[q] = row[0]
    assert sorted(np.flatnonzero(want_verdict == HS_CONSUMED)) == sorted(row_of.values())
    assert (want_verdict == ERR_AUTH).sum() == 1 and (want_verdict == ERR_NO_PEER).sum() == 1
    want_verdict[row_of["masked"]] = HS_NONE  # the host's mask

    # one descriptor per consumed row -- the masked one too -- and one packet to seal per descriptor
    n_keys, key_fill = 2 * len(names) + 2, 0xC3
    resp = np.zeros(len(names), HS_RESP_DTYPE)
    seal_pkts = np.zeros(len(names), AEAD_PKT_DTYPE)
    mtu, slot = 1420, 256
    seal_arena = np.full(len(names) * slot + 64, SENTINEL, np.uint8)
    for j, k in enumerate(names):
        p = ini[k]
        p.local_index, p.resp_eph, p.cookie = int(rng.integers(0, 2**32)), rng.bytes(32), rng.bytes(16) if j % 2 else None
        resp[j] = (row_of[k], p.peer_row, p.local_index, 2 * j + 1, 2 * j + 2, 0 if p.cookie is None else 1, 0,
                   np.frombuffer(p.resp_eph, np.uint8), np.frombuffer(p.cookie or bytes(16), np.uint8))
        length = 40 + 4 * j
        p.packet = bytes([0x45, 0, 0, length]) + rng.bytes(length - 4)  # an IPv4 header's first bytes: the trim keeps it all
        p.counter = (1 << 33) + j
        off = j * slot + 1 + j  # any byte offset
        seal_arena[off + 16:off + 16 + length] = np.frombuffer(p.packet, np.uint8)
        seal_pkts[j] = (off, p.counter, length, 2 * j + 1)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_land, d_n_in, d_gso = up(land), torch.from_numpy(n_in).cuda(), torch.from_numpy(gso).cuda()
        d_slots = up(s.slots)
        d_checker = up(np.frombuffer(checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE))
        d_responder, d_table, d_psk = up(responder), up(table), up(psk)
        d_arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
        i32 = lambda m, fill=MARK: torch.full((m,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
        d_n_out, d_from, d_count, d_split_status = i32(n), i32(n), i32(nb), i32(nb)
        d_pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        d_type, d_screen, d_verdict = i32(n), i32(n), i32(n)
        d_init = torch.full((128 * n,), 0xEE, dtype=torch.uint8, device="cuda")
        d_resp = up(resp)
        d_keys = torch.full((48 * n_keys,), key_fill, dtype=torch.uint8, device="cuda")
        d_msgs = torch.full((PITCH * len(names),), SENTINEL, dtype=torch.uint8, device="cuda")
        d_status = i32(len(names), STATUS_FILL)
        d_seal_arena, d_seal_pkts, d_out_len = up(seal_arena), up(seal_pkts), i32(len(names))
        masked_row = torch.tensor([row_of["masked"]], device="cuda")
        stream.synchronize()
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d_land.data_ptr(), s.in_stride, s.buf_len, d_n_in.data_ptr(),
                                               d_gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, d_arena.data_ptr(), stride,
                                               d_n_out.data_ptr(), d_from.data_ptr(), d_count.data_ptr(),
                                               d_split_status.data_ptr(), stream.cuda_stream)
        assert rc == 0
        router.classify_batch(dev, d_arena, d_n_out, d_slots, d_pkts, d_type, stride=stride, stream=stream, n=n,
                              n_slots=len(s.slots))
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_screen, under_load=False, stream=stream, n=n)
        noise.consume_batch(dev, d_arena, d_pkts, d_type, d_screen, d_responder, d_table, d_verdict, d_init,
                            stream=stream, n=n, n_peers=n_peers)
        d_verdict.index_fill_(0, masked_row, HS_NONE)  # the host's timestamp rule, enqueued on the same stream
        noise.respond_batch(dev, d_resp, d_init, d_verdict, d_table, d_psk, d_keys, d_msgs, d_status, stream=stream,
                            n=len(names), n_init=n, n_peers=n_peers, n_keys=n_keys)
        transport.seal_batch(dev, d_seal_arena, d_seal_pkts, d_keys, mtu, d_out_len, stream=stream, n=len(names),
                             n_keys=n_keys)
        stream.synchronize()
    assert np.array_equal(d_type.cpu().numpy(), want.type)
    assert np.array_equal(d_verdict.cpu().numpy(), want_verdict)
    assert d_init.cpu().numpy().tobytes() == want_init.tobytes()
    status, msgs = d_status.cpu().numpy(), d_msgs.cpu().numpy()
    keys = d_keys.cpu().numpy().view(AEAD_KEY_DTYPE)
    sealed, out_len = d_seal_arena.cpu().numpy(), d_out_len.cpu().numpy()
    assert status.tolist() == [HS_RESPONDED, HS_RESPONDED, HS_NONE, HS_RESPONDED]
    j = names.index("masked")
    assert (msgs[PITCH * j:PITCH * (j + 1)] == SENTINEL).all(), "the masked row has no response"
    assert (keys.view(np.uint8).reshape(n_keys, 48)[[0, 2 * j + 1, 2 * j + 2, n_keys - 1]] == key_fill).all()
    back = np.full(len(names) * slot, SENTINEL, np.uint8)
    back_pkts = np.zeros(len(names), AEAD_PKT_DTYPE)
    for j, k in enumerate(names):
        if k == "masked":
            back_pkts[j] = (j * slot, 0, 0, 0)  # too short to be looked at
            continue
        p = ini[k]
        msg = msgs[PITCH * j:PITCH * j + 92].tobytes()
        assert cookie_ref.Checker(p.public).check_mac1(msg), "CheckMAC1 on the initiator's side"
        assert msg[76:] == (bytes(16) if p.cookie is None else cookie_ref.mac128(p.cookie, msg[:76]))
        rc, sender, send, recv, _, _ = noise_resp_ref.consume_response(p.private, p.hash, p.chain, p.eph, p.index, msg, p.psk)
        assert (rc, sender) == (0, p.local_index), k
        assert keys[2 * j + 1].tobytes() == noise_resp_ref.aead_key_bytes(recv, p.index)
        assert keys[2 * j + 2].tobytes() == noise_resp_ref.aead_key_bytes(send, 0)
        # the packet the responder sealed under its fresh send key opens under the initiator's receive key
        off = int(seal_pkts["off"][j])
        assert out_len[j] == 32 + len(p.packet) + aead_ref.padding(len(p.packet), mtu)
        wire = sealed[off:off + out_len[j]].tobytes()
        assert wire == aead_ref.wg_seal(recv, p.index, p.counter, p.packet, mtu)
        ctr, plain = aead_ref.wg_open(recv, wire)
        assert ctr == p.counter and plain[:len(p.packet)] == p.packet
        # and one sealed back by the initiator opens on the device under the recv-key row
        p.reply = bytes([0x45, 0, 0, 28]) + rng.bytes(24)
        reply = aead_ref.wg_seal(send, p.local_index, 3 + j, p.reply, mtu)
        back[j * slot:j * slot + len(reply)] = np.frombuffer(reply, np.uint8)
        back_pkts[j] = (j * slot, 0, len(reply), 2 * j + 2)
    d_back, d_back_pkts = up(back), up(back_pkts)
    d_pkt_len = torch.full((len(names),), STATUS_FILL, dtype=torch.int32, device="cuda")
    d_counter = torch.zeros(len(names), dtype=torch.int64, device="cuda")
    transport.open_batch(dev, d_back, d_back_pkts, d_keys, d_pkt_len, d_counter, n=len(names), n_keys=n_keys)
    torch.cuda.synchronize()
    opened, pkt_len, counter = d_back.cpu().numpy(), d_pkt_len.cpu().numpy(), d_counter.cpu().numpy()
    for j, k in enumerate(names):
        if k == "masked":
            assert pkt_len[j] == -13  # WGCS_ERR_OUT_OF_RANGE: nothing read
            continue
        assert pkt_len[j] == 28 and counter[j] == 3 + j
        assert opened[j * slot + 16:j * slot + 16 + 28].tobytes() == ini[k].reply
