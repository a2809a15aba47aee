"""The device-resident handshake screen on the GPU (wgcs_handshake_screen_batch,
cookie_kernels.hip) against tests/cookie_ref.py, which tests/test_cookie_ref.py
pins to published vectors.

All comparisons are exact.  The kernel writes nothing to the arena: it is
filled with a sentinel around its messages and compared whole afterwards, and
so are d_verdict and d_reply, which are longer than the batch.  Messages sit at
odd byte offsets, and some at offsets that are 2 mod 4 (the chain's are
16-byte aligned), so every alignment of the kernel's dword loads occurs.
References are computed once per size and shared."""
import functools
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cookie_ref
from cookie_ref import ERR_INVALID_ARG, ERR_MAC1, HS_COOKIE, HS_NONE, HS_PASS
from wireguard_amd import _lib, cookie, router, transport
from wireguard_amd.cookie import COOKIE_CHECKER_DTYPE, SRC_ADDR_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

SENTINEL, REPLY_FILL, VERDICT_FILL = 0xA5, 0xEE, 12345
SPARE = 3  # rows of d_verdict / d_reply past the batch: they keep their fill
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]
PUB = bytes(range(100, 132))
SECRET = bytes(range(7, 39))
REF = cookie_ref.Checker(PUB, SECRET)


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def flip(b: bytes, i: int, bit: int = 0) -> bytes:
    return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]


def src_row(b: bytes) -> np.ndarray:
    """One SRC_ADDR_DTYPE row holding b, of any length up to 18 (the bad rows too)."""
    row = np.zeros(1, SRC_ADDR_DTYPE)
    row["b"][0, :len(b)] = np.frombuffer(b, np.uint8)
    row["len"] = len(b)
    return row


class Rows:
    """A batch under construction: messages at odd offsets of a sentinel arena."""

    def __init__(self, rng):
        self.rng, self.chunks, self.pos = rng, [], 1
        self.type, self.pkts, self.src, self.msg, self.nonce = [], [], [], [], []

    def add(self, type_, msg, src, length=None, even=False):
        """`msg`: the bytes in the arena (None: the row points at no message);
        `length`: d_pkts[q].len where it is not len(msg); `even`: at an offset
        that is 2 mod 4, the one alignment the odd offsets leave out."""
        off = 0
        if msg is not None:
            self.pos |= 1
            if even:
                self.pos = (self.pos | 3) + 3
            off = self.pos
            self.chunks.append((off, msg))
            self.pos += len(msg) + int(self.rng.integers(0, 40))
        length = (len(msg) if msg is not None else 0) if length is None else length
        self.type.append(type_)
        self.pkts.append((off, 0, length, 0xFFFFFFFF))
        self.src.append(src)
        self.msg.append(msg if msg is not None and length == len(msg) else None)
        self.nonce.append(self.rng.bytes(24))

    def finish(self):
        n = len(self.type)
        arena = np.full(self.pos + 64, SENTINEL, np.uint8)
        for off, msg in self.chunks:
            arena[off:off + len(msg)] = np.frombuffer(msg, np.uint8)
        b = SimpleNamespace(n=n, arena=arena, type=np.array(self.type, np.int32).reshape(n),
                            pkts=np.array(self.pkts, AEAD_PKT_DTYPE).reshape(n), msg=self.msg, src_bytes=self.src,
                            nonce_bytes=self.nonce)
        b.src = np.concatenate([src_row(s) for s in self.src]) if n else np.zeros(0, SRC_ADDR_DTYPE)
        b.nonce = np.frombuffer(b"".join(self.nonce), np.uint8)
        return b


def expect(b, under_load):
    """(d_verdict, d_reply) whole, spare rows and fills included."""
    verdict = np.full(b.n + SPARE, VERDICT_FILL, np.int32)
    reply = np.full(64 * (b.n + SPARE), REPLY_FILL, np.uint8)
    for q in range(b.n):
        v, r = cookie_ref.screen(REF, int(b.type[q]), b.msg[q], b.src_bytes[q], under_load, b.nonce_bytes[q])
        verdict[q] = v
        if r is not None:
            reply[64 * q:64 * q + 64] = np.frombuffer(r, np.uint8)
    return verdict, reply


def launch(dev, b, under_load, stream=None):
    d = SimpleNamespace()
    d.arena, d.pkts, d.type = up(b.arena), up(b.pkts) if b.n else up(np.zeros(1, AEAD_PKT_DTYPE)), up(b.type)
    d.checker = up(np.frombuffer(REF.tobytes(), COOKIE_CHECKER_DTYPE))
    d.src = up(b.src) if b.n else up(np.zeros(1, SRC_ADDR_DTYPE))
    d.nonce = up(b.nonce) if b.n else up(np.zeros(24, np.uint8))
    d.verdict = torch.full((b.n + SPARE,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    d.reply = torch.full((64 * (b.n + SPARE),), REPLY_FILL, dtype=torch.uint8, device="cuda")
    cookie.screen_batch(dev, d.arena, d.pkts, d.type, d.checker, d.src, d.verdict, under_load=under_load, nonce=d.nonce,
                        reply=d.reply, stream=stream, n=b.n)
    torch.cuda.synchronize()
    return d


def check(dev, b, under_load, want=None):
    d = launch(dev, b, under_load)
    verdict, reply = d.verdict.cpu().numpy(), d.reply.cpu().numpy()
    want_verdict, want_reply = want or expect(b, under_load)
    bad = np.flatnonzero(verdict != want_verdict)
    assert len(bad) == 0, (f"under_load={under_load}: {len(bad)} verdicts differ, first at row {bad[0]} (type "
                           f"{b.type[bad[0]] if bad[0] < b.n else None}): got {verdict[bad[0]]}, want {want_verdict[bad[0]]}")
    bad = np.flatnonzero(reply != want_reply)
    assert len(bad) == 0, f"under_load={under_load}: reply bytes differ, first in row {bad[0] // 64} at byte {bad[0] % 64}"
    assert np.array_equal(d.arena.cpu().numpy(), b.arena), "the screen wrote the arena"
    return verdict, reply


SOURCES = [cookie_ref.src_bytes(bytes([198, 51, 100, 7]), 51820),
           cookie_ref.src_bytes(bytes.fromhex("20010db80000000000000000deadbeef"), 40000),
           cookie_ref.src_bytes(bytes(4), 0), cookie_ref.src_bytes(b"\xff" * 16, 65535)]


@functools.lru_cache(maxsize=None)
def mixed(n):
    """n rows that cycle through every kind of row the screen can meet, with v4
    and v6 sources, and the references for both load states."""
    rng = np.random.default_rng(1000 + n)
    rows = Rows(rng)
    for q in range(n):
        kind, src = q % 11, SOURCES[(q // 2) % len(SOURCES)]
        other = SOURCES[(q // 2 + 1) % len(SOURCES)]
        if kind in (0, 5):    # an initiation with MAC1 only
            rows.add(1, cookie_ref.handshake_message(rng, 1, REF.mac1_key), src, even=kind == 5)
        elif kind == 1:       # a response with MAC1 only
            rows.add(2, cookie_ref.handshake_message(rng, 2, REF.mac1_key), src)
        elif kind == 2:       # an initiation with the MAC2 of its source
            rows.add(1, cookie_ref.handshake_message(rng, 1, REF.mac1_key, REF.cookie(src)), src)
        elif kind == 3:       # a response with the MAC2 of its source
            rows.add(2, cookie_ref.handshake_message(rng, 2, REF.mac1_key, REF.cookie(src)), src, even=True)
        elif kind == 4:       # a MAC2 made for another source
            rows.add(1 + q % 2, cookie_ref.handshake_message(rng, 1 + q % 2, REF.mac1_key, REF.cookie(other)), src)
        elif kind == 6:       # forged: random MACs
            rows.add(1 + q % 2, struct.pack("<I", 1 + q % 2) + rng.bytes(cookie_ref.SIZE_OF_TYPE[1 + q % 2] - 4), src)
        elif kind == 7:       # a cookie reply stays with the host
            rows.add(3, struct.pack("<I", 3) + rng.bytes(60), src)
        elif kind == 8:       # a transport row
            rows.add(4, struct.pack("<I", 4) + rng.bytes(28 + 16 * int(rng.integers(0, 8))), src)
        elif kind == 9:       # classify's 0: a runt, an unknown type, an unlisted receiver
            rows.add(0, rng.bytes(int(rng.integers(1, 200))), src)
        else:                 # classify's refusal: len 0, nothing to read
            rows.add(_lib.ERR_OUT_OF_RANGE, None, src)
    b = rows.finish()
    return b, expect(b, False), expect(b, True)


@pytest.mark.parametrize("n", SIZES)
def test_mixed_rows_match_the_reference(dev, n):
    b, want_rest, want_load = mixed(n)
    check(dev, b, False, want_rest)
    verdict, reply = check(dev, b, True, want_load)
    if n >= 11:
        for v in (HS_NONE, HS_PASS, HS_COOKIE, ERR_MAC1):
            assert (want_load[0][:n] == v).any(), v
        assert not (want_rest[0][:n] == HS_COOKIE).any()
    # every reply opens on the host and yields the cookie of its row's source
    for q in np.flatnonzero(verdict[:n] == HS_COOKIE):
        r = reply[64 * q:64 * q + 64].tobytes()
        assert r[:4] == struct.pack("<I", 3) and r[4:8] == b.msg[q][4:8] and r[8:32] == b.nonce_bytes[q]
        assert cookie.consume_reply(REF.cookie_key, b.msg[q][-32:-16], r) == REF.cookie(b.src_bytes[q])


def test_under_load_zero_takes_no_source_nonce_or_reply(dev):
    b, want_rest, _ = mixed(65)
    d_arena, d_pkts, d_type = up(b.arena), up(b.pkts), up(b.type)
    d_checker = up(np.frombuffer(REF.tobytes(), COOKIE_CHECKER_DTYPE))
    d_verdict = torch.full((b.n + SPARE,), VERDICT_FILL, dtype=torch.int32, device="cuda")
    cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_verdict, under_load=False, n=b.n)
    torch.cuda.synchronize()
    assert np.array_equal(d_verdict.cpu().numpy(), want_rest[0])
    # under load the three arrays are required, and nothing is enqueued without them
    with pytest.raises(_lib.WgcsError) as ei:
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_verdict, under_load=True, n=b.n)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.WgcsError) as ei:  # a misaligned d_verdict
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_verdict.data_ptr() + 2, n=b.n)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.WgcsError) as ei:
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, None, d_verdict, n=(1 << 28) + 1)
    assert ei.value.code == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert np.array_equal(d_verdict.cpu().numpy(), want_rest[0])


def test_single_bit_flips_name_their_verdict(dev):
    rng = np.random.default_rng(272)
    v4, v6 = SOURCES[0], SOURCES[1]
    cases = []  # (type, message, the source the row carries, verdict at rest, verdict under load)
    for type_, src in ((1, v4), (2, v6), (1, v6), (2, v4)):
        size = cookie_ref.SIZE_OF_TYPE[type_]
        good = cookie_ref.handshake_message(rng, type_, REF.mac1_key, REF.cookie(src))
        cases.append((type_, good, src, HS_PASS, HS_PASS))
        # the first and the last byte MAC1 covers (0 and 115 / 0 and 59), the first and the last of its field
        for i, bit in ((0, 0), (0, 7), (size - 33, 0), (size - 33, 7), (size - 32, 0), (size - 17, 7)):
            cases.append((type_, flip(good, i, bit), src, ERR_MAC1, ERR_MAC1))
        # the first and the last byte of the MAC2 field
        for i, bit in ((size - 16, 0), (size - 1, 7)):
            cases.append((type_, flip(good, i, bit), src, HS_PASS, HS_COOKIE))
        # a port off by one, an address off in its last byte
        port_at, addr_last = len(src) - 2, len(src) - 3
        cases.append((type_, good, flip(src, port_at, 0), HS_PASS, HS_COOKIE))
        cases.append((type_, good, flip(src, port_at + 1, 0), HS_PASS, HS_COOKIE))
        cases.append((type_, good, flip(src, addr_last, 0), HS_PASS, HS_COOKIE))
        cases.append((type_, good, flip(src, 0, 7), HS_PASS, HS_COOKIE))
    rows = Rows(rng)
    for type_, msg, src, _, _ in cases:
        rows.add(type_, msg, src)
    b = rows.finish()
    for under_load, col in ((False, 3), (True, 4)):
        verdict, _ = check(dev, b, under_load)
        assert verdict[:b.n].tolist() == [c[col] for c in cases]


def test_bad_rows_are_refused_untouched(dev):
    rng = np.random.default_rng(147)
    src = SOURCES[0]
    rows, named = Rows(rng), []
    init = cookie_ref.handshake_message(rng, 1, REF.mac1_key)
    resp = cookie_ref.handshake_message(rng, 2, REF.mac1_key)
    for type_, msg, length in ((1, init, 147), (2, resp, 93), (1, init, 92), (2, resp, 148), (1, init, 0), (2, resp, 149)):
        rows.add(type_, msg, src, length=length)
        named.append((ERR_INVALID_ARG, ERR_INVALID_ARG))
    for bad_src in (b"", src[:4], src + bytes(11)):  # a source len of 0, 4 and 17
        for type_, msg in ((1, init), (2, resp)):
            rows.add(type_, msg, bad_src)
            named.append((HS_PASS, ERR_INVALID_ARG))
    # MAC1 comes first, as in the reference: a forged message is ERR_MAC1 whatever its source row holds
    rows.add(1, flip(init, 5), b"")
    named.append((ERR_MAC1, ERR_MAC1))
    rows.add(1, init, src)
    named.append((HS_PASS, HS_COOKIE))
    b = rows.finish()
    for under_load, col in ((False, 0), (True, 1)):
        verdict, reply = check(dev, b, under_load)
        assert verdict[:b.n].tolist() == [x[col] for x in named]
        untouched = [q for q in range(b.n) if verdict[q] != HS_COOKIE]
        assert all((reply[64 * q:64 * q + 64] == REPLY_FILL).all() for q in untouched)


def test_cookie_round_trip_on_the_device(dev):
    """The loopback of tests/test_cookie_ref.py with the kernel as the screen."""
    rng = np.random.default_rng(99)
    src, port_off, addr_off = SOURCES[1], flip(SOURCES[1], 16), flip(SOURCES[1], 15)
    body = struct.pack("<I", 1) + rng.bytes(112) + bytes(32)
    msg, last_mac1 = cookie.add_macs(REF.mac1_key, body)
    rows = Rows(rng)
    rows.add(1, msg, src)
    b = rows.finish()
    assert check(dev, b, False)[0][0] == HS_PASS
    verdict, reply = check(dev, b, True)
    assert verdict[0] == HS_COOKIE
    got = cookie.consume_reply(REF.cookie_key, last_mac1, reply[:64].tobytes())
    assert got == REF.cookie(src)
    msg2, _ = cookie.add_macs(REF.mac1_key, body, got)
    rows = Rows(rng)
    for s in (src, port_off, addr_off):
        rows.add(1, msg2, s)
    b = rows.finish()
    assert check(dev, b, True)[0][:3].tolist() == [HS_PASS, HS_COOKIE, HS_COOKIE]
    # a new secret: the old cookie no longer passes
    d = launch(dev, b, True)
    newer = cookie_ref.Checker(PUB, rng.bytes(32))
    d.checker.copy_(up(np.frombuffer(newer.tobytes(), COOKIE_CHECKER_DTYPE)))
    cookie.screen_batch(dev, d.arena, d.pkts, d.type, d.checker, d.src, d.verdict, under_load=True, nonce=d.nonce,
                        reply=d.reply, n=b.n)
    torch.cuda.synchronize()
    assert d.verdict.cpu().numpy()[:3].tolist() == [HS_COOKIE] * 3
    r = d.reply.cpu().numpy()[:64].tobytes()
    assert cookie.consume_reply(REF.cookie_key, msg2[-32:-16], r) == newer.cookie(src)


# ----------------------------------------------------------------------- chain
def chain_case():
    """The receive scenario of tests/test_gpu_path.py (transport messages, one
    forged initiation among them) with a batch of handshakes after each of its
    batches -- single datagrams and a UDP-GRO run of initiations -- and what the
    chain leaves of it: path_ref.recv_ref for the split, classify and open,
    cookie_ref for the screen."""
    import path_ref
    from path_ref import FIRST_MSG_AT, N_MSGS

    ref = path_ref.run_reference(20261019, 4112, 4099)
    s, rng = ref.s, np.random.default_rng(4112)
    per = N_MSGS - FIRST_MSG_AT  # landing buffers per batch
    nb0 = len(ref.n_in) // N_MSGS
    nb = 2 * nb0
    n, stride, pitch = nb * N_MSGS, s.stride, per * s.in_stride
    hs_src = [SOURCES[0], SOURCES[1]]  # the one source of every row of a handshake batch, by its kind

    def hs_batch(kind, land, n_in, gso):
        if kind == 0:  # a GRO run of three initiations (the second with its MAC2, the third forged), then a response
            run = b"".join([cookie_ref.handshake_message(rng, 1, REF.mac1_key),
                            cookie_ref.handshake_message(rng, 1, REF.mac1_key, REF.cookie(hs_src[0])),
                            flip(cookie_ref.handshake_message(rng, 1, REF.mac1_key), 9)])
            datagrams, sizes = [run, cookie_ref.handshake_message(rng, 2, REF.mac1_key)], [148, 0]
        else:          # a response with its MAC2, and a cookie reply
            datagrams = [cookie_ref.handshake_message(rng, 2, REF.mac1_key, REF.cookie(hs_src[1])),
                         struct.pack("<I", 3) + rng.bytes(60)]
            sizes = [0, 0]
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
    # The source of row q is the address of the datagram the split cuts it from: the host knows it before the
    # launch, from recvmmsg's counts and GRO sizes alone.
    srcs, nonces = [], []
    for q in range(n):
        b, k = divmod(q, N_MSGS)
        origin = int(want.src[q]) if want.src[q] >= 0 else k
        srcs.append(hs_src[(b // 2) % 2] if b % 2 else SOURCES[(b + origin) % len(SOURCES)])
        nonces.append(rng.bytes(24))
    want.screen_verdict = np.full(n + SPARE, VERDICT_FILL, np.int32)
    want.screen_reply = np.full(64 * (n + SPARE), REPLY_FILL, np.uint8)
    for q in range(n):
        t, length = int(want.type[q]), int(want.pkts["len"][q])
        msg = want.arena_split[q * stride:q * stride + length].tobytes() if t in (1, 2) else None
        v, r = cookie_ref.screen(REF, t, msg, srcs[q], True, nonces[q])
        want.screen_verdict[q] = v
        if r is not None:
            want.screen_reply[64 * q:64 * q + 64] = np.frombuffer(r, np.uint8)
    assert {1, 2, 3, 4} <= set(want.type.tolist())
    for v in (HS_NONE, HS_PASS, HS_COOKIE, ERR_MAC1):
        assert (want.screen_verdict[:n] == v).any(), v
    return SimpleNamespace(s=s, land=land, n_in=n_in, gso=gso, nb=nb, n=n, want=want, nonces=nonces,
                           src_rows=np.concatenate([src_row(x) for x in srcs]))


def test_receive_chain_with_handshakes(dev):
    """wgcs_split_messages_batch -> wgcs_recv_classify_batch -> wgcs_handshake_screen_batch
    and wgcs_aead_open_batch over the same rows, on one stream with no host step
    in between."""
    import path_ref
    from path_ref import FIRST_MSG_AT, MARK, N_MSGS

    c = chain_case()
    s, land, n_in, gso, nb, n, want, nonces, src_rows = c.s, c.land, c.n_in, c.gso, c.nb, c.n, c.want, c.nonces, c.src_rows
    stride = s.stride
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_land, d_n_in, d_gso = up(land), torch.from_numpy(n_in).cuda(), torch.from_numpy(gso).cuda()
        d_slots, d_keys = up(s.slots), up(s.keys)
        d_checker, d_src = up(np.frombuffer(REF.tobytes(), COOKIE_CHECKER_DTYPE)), up(src_rows)
        d_nonce = up(np.frombuffer(b"".join(nonces), np.uint8))
        d_arena = torch.full((n * stride,), path_ref.RECV_SENTINEL, dtype=torch.uint8, device="cuda")
        i32 = lambda m, fill=MARK: torch.full((m,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
        d_n_out, d_from, d_count, d_status = i32(n), i32(n), i32(nb), i32(nb)
        d_pkts = torch.full((n * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        d_type, d_len, d_verdict = i32(n), i32(n), i32(n + SPARE, VERDICT_FILL)
        d_counter = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_reply = torch.full((64 * (n + SPARE),), REPLY_FILL, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        rc = dev.lib.wgcs_split_messages_batch(dev.h, d_land.data_ptr(), s.in_stride, s.buf_len, d_n_in.data_ptr(),
                                               d_gso.data_ptr(), N_MSGS, FIRST_MSG_AT, nb, d_arena.data_ptr(), stride,
                                               d_n_out.data_ptr(), d_from.data_ptr(), d_count.data_ptr(),
                                               d_status.data_ptr(), stream.cuda_stream)
        assert rc == 0
        router.classify_batch(dev, d_arena, d_n_out, d_slots, d_pkts, d_type, stride=stride, stream=stream, n=n,
                              n_slots=len(s.slots))
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_checker, d_src, d_verdict, under_load=True, nonce=d_nonce,
                            reply=d_reply, stream=stream, n=n)
        transport.open_batch(dev, d_arena, d_pkts, d_keys, d_len, d_counter, stream=stream, n=n, n_keys=len(s.keys))
        stream.synchronize()

    def host(t, dtype=None):
        a = t.cpu().numpy()
        return a if dtype is None else a.view(dtype)
    assert np.array_equal(host(d_count), want.count) and np.array_equal(host(d_status), want.split_status)
    assert np.array_equal(host(d_n_out), want.n_out) and np.array_equal(host(d_from), want.src)
    assert np.array_equal(host(d_type), want.type)
    assert np.array_equal(host(d_pkts, AEAD_PKT_DTYPE), want.pkts)
    assert np.array_equal(host(d_len), want.pkt_len)
    assert np.array_equal(host(d_counter, np.uint64), want.counter)
    # the transport rows hold their plaintext, everything else of the arena is as the split left it
    assert np.array_equal(host(d_arena), want.arena_opened)
    # the screen, from the bytes the split wrote
    assert np.array_equal(host(d_verdict), want.screen_verdict)
    assert np.array_equal(host(d_reply), want.screen_reply)
    assert np.array_equal(host(d_land), land), "the landing buffers are only read"
