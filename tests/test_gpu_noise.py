"""Batched X25519 and the device-resident handshake consume step on the GPU
(wgcs_x25519_batch, wgcs_handshake_consume_batch, noise_kernels.hip).

X25519 rows are compared with tests/noise_ref.py, which tests/test_noise_ref.py
pins to RFC 7748 and to OpenSSL.  Consume rows are compared, verdict and every
byte of d_out, with the host function wgcs_noise_consume_initiation, which
tests/test_noise_host.py pins to noise_ref; a pool of distinct messages is made
once and the batches place them at every byte alignment of a sentinel arena
that is compared whole afterwards.  Output arrays are longer than the batch
and keep their fill outside it."""
import functools
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cookie_ref
import noise_ref
from noise_ref import (ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, ERR_NO_PEER, HS_CONSUMED, HS_NONE, HS_PASS,
                       LOW_ORDER_POINTS, P, PEER_NONE)
from test_gpu_cookie import SENTINEL, flip, up
from wireguard_amd import _lib, cookie, noise, router
from wireguard_amd.noise import HS_INIT_DTYPE, PEER_KEY_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

GUARD = 3                       # rows of sentinel before and after the X25519 outputs
OUT_FILL, VERDICT_FILL = 0xEE, 12345
SPARE = 3                       # rows of d_verdict / d_out past the batch: they keep their fill
HS_COOKIE, ERR_MAC1 = 2, -21


def le(n: int) -> bytes:
    return n.to_bytes(32, "little")


# ---------------------------------------------------------------------- X25519
RFC_ROWS = [("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
             "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
             "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"),
            ("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
             "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
             "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957")]


@functools.lru_cache(maxsize=None)
def special_rows():
    """(scalar, point) pairs: the RFC vectors, the low-order points with and
    without bit 255, non-canonical points, and the all-zero and all-ones scalars."""
    rng = np.random.default_rng(7748)
    k = rng.bytes(32)
    rows = [(bytes.fromhex(a), bytes.fromhex(b)) for a, b, _ in RFC_ROWS]
    rows += [(k, u) for u in LOW_ORDER_POINTS] + [(k, flip(u, 31, 7)) for u in LOW_ORDER_POINTS]
    rows += [(k, le(2**255 - 1)), (k, le(2**256 - 1)), (k, le(P + 2)), (k, le(2)), (k, le(18))]
    u = rng.bytes(32)
    rows += [(bytes(32), u), (b"\xff" * 32, u), (bytes(32), le(0)), (b"\xff" * 32, le(P - 1))]
    return rows


@functools.lru_cache(maxsize=None)
def x_rows(n):
    """n rows and their (out, status) by noise_ref: every special row where there is room, then random ones."""
    rng = np.random.default_rng(100 + n)
    rows = list(special_rows())[:n]
    rows += [(rng.bytes(32), rng.bytes(32)) for _ in range(n - len(rows))]
    order = rng.permutation(n)
    rows = [rows[i] for i in order]
    out = [noise_ref.x25519_raw(k, u) for k, u in rows]
    status = np.array([ERR_LOW_ORDER if o == bytes(32) else 0 for o in out], np.int32)
    return rows, b"".join(out), status


def run_x25519(dev, rows):
    n = len(rows)
    d_k, d_u = up(np.frombuffer(b"".join(k for k, _ in rows), np.uint8)), up(np.frombuffer(b"".join(u for _, u in rows), np.uint8))
    d_out = torch.full((32 * (n + 2 * GUARD),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n + 2 * GUARD,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    noise.x25519_batch(dev, d_k, d_u, d_out.data_ptr() + 32 * GUARD, d_status.data_ptr() + 4 * GUARD, n=n)
    torch.cuda.synchronize()
    out, status = d_out.cpu().numpy(), d_status.cpu().numpy()
    assert (out[:32 * GUARD] == SENTINEL).all() and (out[32 * (GUARD + n):] == SENTINEL).all(), "output guards"
    assert (status[:GUARD] == VERDICT_FILL).all() and (status[GUARD + n:] == VERDICT_FILL).all(), "status guards"
    return out[32 * GUARD:32 * (GUARD + n)].tobytes(), status[GUARD:GUARD + n]


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_x25519_batch_matches_the_reference(dev, n):
    rows, want_out, want_status = x_rows(n)
    out, status = run_x25519(dev, rows)
    bad = [q for q in range(n) if out[32 * q:32 * q + 32] != want_out[32 * q:32 * q + 32]]
    assert not bad, f"{len(bad)} rows differ, first {bad[0]}: scalar {rows[bad[0]][0].hex()} point {rows[bad[0]][1].hex()}"
    assert np.array_equal(status, want_status)
    assert (want_status == ERR_LOW_ORDER).sum() >= 10 and (want_status == 0).sum() >= 40


def test_x25519_batch_of_one_row(dev):
    """n = 1 for each special row: the RFC vectors as literals, the rest by noise_ref."""
    for a, b, want in RFC_ROWS:
        out, status = run_x25519(dev, [(bytes.fromhex(a), bytes.fromhex(b))])
        assert out.hex() == want and status[0] == 0
    for k, u in special_rows()[2:]:
        out, status = run_x25519(dev, [(k, u)])
        want = noise_ref.x25519_raw(k, u)
        assert out == want and status[0] == (ERR_LOW_ORDER if want == bytes(32) else 0), (k.hex(), u.hex())


def test_x25519_batch_arguments(dev):
    d = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    st = torch.zeros(64, dtype=torch.int32, device="cuda")
    noise.x25519_batch(dev, d, d, d, st, n=0)  # a no-op
    for args in ((None, d, d, st), (d, None, d, st), (d, d, None, st), (d, d, d, None),
                 (d.data_ptr() + 2, d, d, st), (d, d, d.data_ptr() + 1, st)):
        with pytest.raises(_lib.WgcsError) as ei:
            noise.x25519_batch(dev, *args, n=4)
        assert ei.value.code == ERR_INVALID_ARG
    with pytest.raises(_lib.WgcsError):
        noise.x25519_batch(dev, d, d, d, st, n=(1 << 28) + 1)
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any()


# --------------------------------------------------------------------- consume
@functools.lru_cache(maxsize=None)
def world():
    """A responder, 37 peers sorted by public key -- a not-running one and one
    whose public key is a low-order point among them --, the tables of 0, 1 and
    37 rows, and a pool of messages that meets every row of the verdict table."""
    rng = np.random.default_rng(405)
    w = SimpleNamespace(rng=rng)
    w.private = rng.bytes(32)
    w.responder, w.public = noise.responder_init(w.private)
    w.ref = noise_ref.Responder(w.private)
    assert w.responder.tobytes() == w.ref.tobytes()
    w.checker = cookie_ref.Checker(w.public)
    keys = sorted(((noise_ref.public_key(k), k) for k in (rng.bytes(32) for _ in range(36))), key=lambda p: p[0])
    low = le(1)  # 01 00 .. 00 sorts before every key that does not begin with a zero byte
    first, last, stopped = keys[0], keys[-1], keys[5]
    peers = [(pub, 100 + i, 0 if (pub, k) == stopped else 1) for i, (pub, k) in enumerate(keys)] + [(low, 99, 1)]
    w.tables = {37: noise.peer_keys_build(w.responder, [p[0] for p in peers], [p[1] for p in peers], [p[2] for p in peers]),
                1: noise.peer_keys_build(w.responder, [last[0]], [100 + 35]), 0: np.zeros(0, PEER_KEY_DTYPE)}
    assert w.tables[37].tobytes() == noise_ref.PeerTable(w.ref, peers).tobytes()
    # both ends of the table are hit: row 0 is `low` or `first`, row 36 is `last`
    assert w.tables[37]["public_key"][0].tobytes() in (low, first[0]) and w.tables[37]["public_key"][36].tobytes() == last[0]

    def make(private):
        return noise.create_initiation(private, w.public, rng.bytes(32), rng.bytes(12), int(rng.integers(0, 2**32)))[0]

    good = make(first[1])
    pool = [("first", good), ("last", make(last[1])), ("last", make(last[1]))]
    pool += [("mid", make(keys[i][1])) for i in (2, 9, 17, 18, 30)]
    pool += [("eph", flip(good, 8)), ("eph", flip(good, 39, 7)), ("static_ct", flip(good, 40)), ("static_ct", flip(good, 71, 7)),
             ("static_tag", flip(good, 72)), ("static_tag", flip(good, 87, 7)), ("ts_ct", flip(good, 88)),
             ("ts_ct", flip(good, 99, 7)), ("ts_tag", flip(good, 100)), ("ts_tag", flip(good, 115, 7))]
    pool += [("stranger", make(rng.bytes(32))), ("stopped", make(stopped[1]))]
    pool.append(("low_static", noise_ref.create_initiation(first[1], w.public, rng.bytes(32), rng.bytes(12), 77,
                                                           static_public=low, precomputed=rng.bytes(32))[0]))
    pool += [("low_eph", good[:8] + u + good[40:]) for u in LOW_ORDER_POINTS]
    pool += [("type_word", struct.pack("<I", 2) + good[4:]), ("type_word", struct.pack("<I", 0x01000001) + good[4:])]
    w.pool = [(kind, cookie_ref.add_macs(w.checker.mac1_key, m)[0]) for kind, m in pool]
    w.first_peer, w.last_peer, w.stopped_peer = 100, 100 + 35, 100 + 5
    return w


@functools.lru_cache(maxsize=None)
def host_consume(n_peers, msg):
    w = world()
    v, row = noise.consume_initiation(w.responder, w.tables[n_peers], msg)
    return v, row.tobytes()


def test_pool_meets_every_verdict_and_the_host_function_agrees_with_the_reference():
    w = world()
    table = noise_ref.PeerTable(w.ref, [(r["public_key"].tobytes(), int(r["peer"]), int(r["flags"])) for r in w.tables[37]])
    seen = {}
    for kind, msg in w.pool:
        v, row = host_consume(37, msg)
        wv, wrow = noise_ref.consume_initiation(w.ref, table, msg)
        assert v == wv and (wrow is None or row == wrow), kind
        seen.setdefault(kind, set()).add((v, struct.unpack_from("<I", row)[0]))
    assert seen["first"] == {(HS_CONSUMED, w.first_peer)} and seen["last"] == {(HS_CONSUMED, w.last_peer)}
    assert seen["eph"] == seen["static_ct"] == seen["static_tag"] == {(ERR_AUTH, PEER_NONE)}
    assert seen["ts_ct"] == seen["ts_tag"] == {(ERR_AUTH, w.first_peer)}
    assert seen["stranger"] == {(ERR_NO_PEER, PEER_NONE)} and seen["stopped"] == {(ERR_NO_PEER, w.stopped_peer)}
    assert seen["low_static"] == {(ERR_NO_PEER, 99)} and seen["low_eph"] == {(ERR_LOW_ORDER, PEER_NONE)}
    assert {v for v, _ in seen["type_word"]} == {ERR_INVALID_ARG}
    assert host_consume(1, w.pool[1][1])[0] == HS_CONSUMED and host_consume(1, w.pool[0][1])[0] == ERR_NO_PEER
    assert host_consume(0, w.pool[0][1])[0] == ERR_NO_PEER


@functools.lru_cache(maxsize=None)
def batch(n):
    """n rows over the pool, row q at a byte offset that is q mod 4 (mod 4), with
    rows of other types, other lengths and other gates among them."""
    w = world()
    rng = np.random.default_rng(2000 + n)
    chunks, pos, sel = [], 8, 0
    b = SimpleNamespace(n=n, type=np.zeros(n, np.int32), gate=np.zeros(n, np.int32), pkts=np.zeros(n, AEAD_PKT_DTYPE), msg=[])
    for q in range(n):
        kind = q % 12 if n > 1 else 0
        msg = w.pool[q % len(w.pool)][1]
        t, gate, length = 1, HS_PASS, 148
        if kind < 7:  # the rows that are consumed go through the pool in order
            msg = w.pool[sel % len(w.pool)][1]
            sel += 1
        if kind == 7:
            t, msg = 2, cookie_ref.handshake_message(rng, 2, w.checker.mac1_key)
            length = len(msg)
        elif kind == 8:
            t, gate, msg = 4, HS_NONE, struct.pack("<I", 4) + rng.bytes(28 + 16 * int(rng.integers(0, 8)))
            length = len(msg)
        elif kind == 9:
            gate = (HS_COOKIE, ERR_MAC1, HS_NONE, ERR_INVALID_ARG)[(q // 12) % 4]  # the screen or the rate limiter said no
        elif kind == 10:
            length = (147, 149, 0, 92)[(q // 12) % 4]
        elif kind == 11:
            t, gate = (0, 3, -13, 5)[(q // 12) % 4], HS_PASS  # not an initiation, whatever the gate holds
        pos = (pos + 3) // 4 * 4 + q % 4
        chunks.append((pos, msg))
        b.type[q], b.gate[q], b.pkts[q] = t, gate, (pos, 0, length, 0xFFFFFFFF)
        b.msg.append(msg)
        pos += max(len(msg), 149) + int(rng.integers(0, 24))
    b.arena = np.full(pos + 64, SENTINEL, np.uint8)
    for off, msg in chunks:
        b.arena[off:off + len(msg)] = np.frombuffer(msg, np.uint8)
    return b


def expect(b, n_peers, use_gate=True):
    verdict = np.full(b.n + SPARE, VERDICT_FILL, np.int32)
    out = np.full(128 * (b.n + SPARE), OUT_FILL, np.uint8)
    for q in range(b.n):
        if b.type[q] != 1 or (use_gate and b.gate[q] != HS_PASS):
            verdict[q] = HS_NONE
        elif b.pkts["len"][q] != 148:
            verdict[q] = ERR_INVALID_ARG
        else:
            verdict[q], row = host_consume(n_peers, b.msg[q])
            if verdict[q] != ERR_INVALID_ARG:
                out[128 * q:128 * q + 128] = np.frombuffer(row, np.uint8)
    return verdict, out


def run_consume(dev, b, n_peers, use_gate=True, stream=None):
    w = world()
    d_arena, d_pkts, d_type, d_gate = up(b.arena), up(b.pkts), up(b.type), up(b.gate)
    d_responder = up(w.responder)
    d_table = up(w.tables[n_peers]) if n_peers else None
    d_verdict = torch.full((b.n + SPARE,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    d_out = torch.full((128 * (b.n + SPARE),), OUT_FILL, dtype=torch.uint8, device="cuda")
    noise.consume_batch(dev, d_arena, d_pkts, d_type, d_gate if use_gate else None, d_responder, d_table, d_verdict,
                        d_out, stream=stream, n=b.n, n_peers=n_peers)
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), b.arena), "the consume step wrote the arena"
    return d_verdict.cpu().numpy(), d_out.cpu().numpy()


def check_consume(dev, b, n_peers, use_gate=True):
    verdict, out = run_consume(dev, b, n_peers, use_gate)
    want_verdict, want_out = expect(b, n_peers, use_gate)
    bad = np.flatnonzero(verdict != want_verdict)
    assert len(bad) == 0, (f"{n_peers} peers: {len(bad)} verdicts differ, first at row {bad[0]}: got {verdict[bad[0]]}, "
                           f"want {want_verdict[bad[0]]}")
    bad = np.flatnonzero(out != want_out)
    assert len(bad) == 0, f"{n_peers} peers: d_out differs, first in row {bad[0] // 128} at byte {bad[0] % 128}"
    rows = out.view(HS_INIT_DTYPE)
    for q in range(b.n):
        if verdict[q] in (ERR_LOW_ORDER, ERR_AUTH, ERR_NO_PEER):  # no key material for a row that failed
            assert not out[128 * q + 8:128 * q + 128].any() and rows["sender"][q] == struct.unpack_from("<I", b.msg[q], 4)[0]
        elif verdict[q] != HS_CONSUMED:
            assert (out[128 * q:128 * q + 128] == OUT_FILL).all()
    return verdict, rows


@pytest.mark.parametrize("n_peers", [0, 1, 37])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_consume_batch_matches_the_host_function(dev, n, n_peers):
    b = batch(n)
    verdict, rows = check_consume(dev, b, n_peers)
    if n == 257:
        for v in ((HS_CONSUMED, ERR_AUTH) if n_peers == 37 else (ERR_NO_PEER,)):  # every alignment of the dword loads
            assert {int(b.pkts["off"][q]) % 4 for q in range(n) if verdict[q] == v} == {0, 1, 2, 3}, v
        for v in (HS_NONE, ERR_INVALID_ARG, ERR_LOW_ORDER, ERR_AUTH, ERR_NO_PEER):
            assert (verdict[:n] == v).any(), v
    if n == 257 and n_peers == 37:
        w = world()
        assert (verdict[:n] == HS_CONSUMED).any()
        consumed = {int(rows["peer"][q]) for q in range(n) if verdict[q] == HS_CONSUMED}
        assert {w.first_peer, w.last_peer} <= consumed and len(consumed) >= 5
        auth_peers = {int(rows["peer"][q]) for q in range(n) if verdict[q] == ERR_AUTH}
        assert auth_peers == {PEER_NONE, w.first_peer}  # how a caller tells the two opens apart
        no_peer = {int(rows["peer"][q]) for q in range(n) if verdict[q] == ERR_NO_PEER}
        assert no_peer == {PEER_NONE, w.stopped_peer, 99}
    if n == 1 and n_peers == 37:
        assert verdict[0] == HS_CONSUMED


def test_null_gate_selects_exactly_the_type_1_rows(dev):
    b = batch(257)
    verdict, _ = check_consume(dev, b, 37, use_gate=False)
    assert np.array_equal(verdict[:b.n] != HS_NONE, b.type == 1)
    gated = np.flatnonzero((b.type == 1) & (b.gate != HS_PASS))
    assert len(gated) and (verdict[gated] != HS_NONE).all()


def test_consume_batch_arguments(dev):
    w, b = world(), batch(65)
    d_arena, d_pkts, d_type, d_gate = up(b.arena), up(b.pkts), up(b.type), up(b.gate)
    d_responder, d_table = up(w.responder), up(w.tables[37])
    d_verdict = torch.full((b.n + SPARE,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    d_out = torch.full((128 * (b.n + SPARE),), OUT_FILL, dtype=torch.uint8, device="cuda")
    noise.consume_batch(dev, d_arena, d_pkts, d_type, d_gate, d_responder, d_table, d_verdict, d_out, n=0)  # a no-op
    cases = [dict(gate=d_verdict), dict(verdict=d_verdict.data_ptr() + 2), dict(out=d_out.data_ptr() + 1),
             dict(responder=None), dict(out=None), dict(n=(1 << 28) + 1), dict(pkts=d_pkts.data_ptr() + 4)]
    for kw in cases:
        a = dict(arena=d_arena, pkts=d_pkts, types=d_type, gate=d_gate, responder=d_responder, table=d_table,
                 verdict=d_verdict, out=d_out, n=b.n, n_peers=37)
        a.update(kw)
        with pytest.raises(_lib.WgcsError) as ei:
            noise.consume_batch(dev, **a)
        assert ei.value.code == ERR_INVALID_ARG, kw
    with pytest.raises(_lib.WgcsError):  # a table is required where n_peers says there is one
        dev._check(dev.lib.wgcs_handshake_consume_batch(dev.h, d_arena.data_ptr(), d_pkts.data_ptr(), d_type.data_ptr(),
                                                        None, b.n, d_responder.data_ptr(), None, 37,
                                                        d_verdict.data_ptr(), d_out.data_ptr(), None))
    torch.cuda.synchronize()
    assert (d_verdict.cpu().numpy() == VERDICT_FILL).all() and (d_out.cpu().numpy() == OUT_FILL).all()


# ----------------------------------------------------------------------- chain
def test_receive_chain_split_classify_screen_consume(dev):
    """wgcs_split_messages_batch -> wgcs_recv_classify_batch ->
    wgcs_handshake_screen_batch (not under load) -> wgcs_handshake_consume_batch
    on one stream with no host step in between: the transport scenario of
    tests/test_gpu_path.py with a batch of handshakes after each of its batches,
    initiations made by create_initiation + add_macs among them, single
    datagrams and a UDP-GRO run."""
    import path_ref
    from path_ref import FIRST_MSG_AT, MARK, N_MSGS

    w = world()
    rng = np.random.default_rng(4113)
    ref = path_ref.run_reference(20261019, 4112, 4099)
    s = ref.s
    per = N_MSGS - FIRST_MSG_AT
    nb0 = len(ref.n_in) // N_MSGS
    nb, stride, pitch = 2 * nb0, s.stride, per * s.in_stride
    n = nb * N_MSGS
    by_kind = {}
    for kind, msg in w.pool:
        by_kind.setdefault(kind, []).append(msg)

    def hs_batch(kind, land, n_in, gso):
        if kind == 0:  # a GRO run: a good initiation, a stranger's, one with a bad MAC1, one whose timestamp
            # does not open; then a response
            run = by_kind["first"][0] + by_kind["stranger"][0] + flip(by_kind["last"][0], 120) + by_kind["ts_tag"][0]
            datagrams, sizes = [run, cookie_ref.handshake_message(rng, 2, w.checker.mac1_key)], [148, 0]
        else:          # single datagrams: a good initiation and a cookie reply
            datagrams, sizes = [by_kind["last"][1], struct.pack("<I", 3) + rng.bytes(60)], [0, 0]
        for k, (dg, g) in enumerate(zip(datagrams, sizes)):
            land[k * s.in_stride:k * s.in_stride + len(dg)] = np.frombuffer(dg, np.uint8)
            n_in[FIRST_MSG_AT + k], gso[FIRST_MSG_AT + k] = len(dg), g

    land = np.full(nb * pitch, path_ref.LAND_SENTINEL, np.uint8)
    n_in, gso = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for b0 in range(nb0):
        part = ref.land[b0 * pitch:(b0 + 1) * pitch]
        land[2 * b0 * pitch:2 * b0 * pitch + len(part)] = part
        n_in[2 * b0 * N_MSGS:(2 * b0 + 1) * N_MSGS] = ref.n_in[b0 * N_MSGS:(b0 + 1) * N_MSGS]
        gso[2 * b0 * N_MSGS:(2 * b0 + 1) * N_MSGS] = ref.gso[b0 * N_MSGS:(b0 + 1) * N_MSGS]
        at, row = (2 * b0 + 1) * pitch, (2 * b0 + 1) * N_MSGS
        hs_batch(b0 % 2, land[at:at + pitch], n_in[row:row + N_MSGS], gso[row:row + N_MSGS])
    want = path_ref.recv_ref(s, land, n_in, gso)
    want_screen = np.full(n + SPARE, VERDICT_FILL, np.int32)
    want_verdict = np.full(n + SPARE, VERDICT_FILL, np.int32)
    want_out = np.full(128 * (n + SPARE), OUT_FILL, np.uint8)
    for q in range(n):
        t, length = int(want.type[q]), int(want.pkts["len"][q])
        msg = want.arena_split[q * stride:q * stride + length].tobytes() if t in (1, 2) else None
        want_screen[q] = cookie_ref.screen(w.checker, t, msg, b"", False, None)[0]
        if t != 1 or want_screen[q] != HS_PASS:
            want_verdict[q] = HS_NONE
        else:
            want_verdict[q], row = host_consume(37, msg)
            want_out[128 * q:128 * q + 128] = np.frombuffer(row, np.uint8)
    assert {1, 2, 3, 4} <= set(want.type.tolist())
    for v in (HS_NONE, HS_CONSUMED, ERR_NO_PEER, ERR_AUTH):
        assert (want_verdict[:n] == v).any(), v
    bad_mac1 = np.flatnonzero(want_screen[:n] == ERR_MAC1)
    assert len(bad_mac1) and (want_verdict[bad_mac1] == HS_NONE).all()

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_land, d_n_in, d_gso = up(land), torch.from_numpy(n_in).cuda(), torch.from_numpy(gso).cuda()
        d_slots = up(s.slots)
        d_checker = up(np.frombuffer(w.checker.tobytes(), cookie.COOKIE_CHECKER_DTYPE))
        d_responder, d_table = up(w.responder), up(w.tables[37])
        d_arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
        i32 = lambda m, fill=MARK: torch.full((m,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
        d_n_out, d_from, d_count, d_status = i32(n), i32(n), i32(nb), i32(nb)
        d_pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        d_type, d_screen, d_verdict = i32(n), i32(n + SPARE, VERDICT_FILL), i32(n + SPARE, VERDICT_FILL)
        d_out = torch.full((128 * (n + SPARE),), OUT_FILL, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d_land.data_ptr(), s.in_stride, s.buf_len, d_n_in.data_ptr(),
                                               d_gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, d_arena.data_ptr(), stride,
                                               d_n_out.data_ptr(), d_from.data_ptr(), d_count.data_ptr(),
                                               d_status.data_ptr(), stream.cuda_stream)
        assert rc == 0
        router.classify_batch(dev, d_arena, d_n_out, d_slots, d_pkts, d_type, stride=stride, stream=stream, n=n,
                              n_slots=len(s.slots))
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_screen, under_load=False, stream=stream, n=n)
        noise.consume_batch(dev, d_arena, d_pkts, d_type, d_screen, d_responder, d_table, d_verdict, d_out,
                            stream=stream, n=n, n_peers=37)
        stream.synchronize()
    assert np.array_equal(d_type.cpu().numpy(), want.type)
    assert np.array_equal(d_pkts.cpu().numpy().view(AEAD_PKT_DTYPE), want.pkts)
    assert np.array_equal(d_arena.cpu().numpy(), want.arena_split), "screen and consume only read the arena"
    assert np.array_equal(d_screen.cpu().numpy(), want_screen)
    assert np.array_equal(d_verdict.cpu().numpy(), want_verdict)
    assert np.array_equal(d_out.cpu().numpy(), want_out)
    assert np.array_equal(d_land.cpu().numpy(), land), "the landing buffers are only read"
