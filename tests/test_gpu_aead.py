"""The transport AEAD on the GPU (wgcs_aead_seal / wgcs_aead_open and their
batch forms, aead_kernels.hip) against the committed golden vectors (made by
OpenSSL) and the RFC 8439 restatement of tests/aead_ref.py.

Every comparison is bit-exact over the whole arena, which is filled with a
sentinel first: a byte outside a packet's extent that changes fails the test."""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

import aead_ref
from wireguard_amd import _lib, transport
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_aead_golden  # noqa: E402

SENTINEL = 0xA5
COUNTERS = [0, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
SWEEP_LENS = [0, 1, 15, 16, 17, 47, 48, 63, 64, 65, 239, 240, 241, 255, 256, 257, 1023, 1024, 1025, 1419, 1420, 1424,
              1500, 3000, 4095, 4096, 4097, 65487]


def make_keys(rng, n=3):
    keys = np.zeros(n, AEAD_KEY_DTYPE)
    for k in range(n):
        keys[k]["key"] = np.frombuffer(rng.bytes(32), np.uint8)
        keys[k]["remote_index"] = 0x01020304 * (k + 1) + 0xF0000000 * (k == 2)
    return keys


def key_bytes(keys, k) -> bytes:
    return keys[k]["key"].tobytes()


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def run_seal(dev, arena, pkts, keys, mtu, n=None, n_keys=None):
    d_arena, d_pkts, d_keys = up(arena), up(pkts), up(keys)
    rows = len(pkts) if n is None else n
    d_out = torch.full((max(len(pkts), 1),), 12345, dtype=torch.int32, device="cuda")
    transport.seal_batch(dev, d_arena, d_pkts, d_keys, mtu, d_out, n=rows, n_keys=len(keys) if n_keys is None else n_keys)
    dev.sync()
    return d_arena.cpu().numpy(), d_out.cpu().numpy()[:len(pkts)]


def run_open(dev, arena, pkts, keys, n=None, n_keys=None):
    d_arena, d_pkts, d_keys = up(arena), up(pkts), up(keys)
    rows = len(pkts) if n is None else n
    d_len = torch.full((max(len(pkts), 1),), 12345, dtype=torch.int32, device="cuda")
    d_ctr = torch.full((max(len(pkts), 1),), -7, dtype=torch.int64, device="cuda")
    transport.open_batch(dev, d_arena, d_pkts, d_keys, d_len, d_ctr, n=rows, n_keys=len(keys) if n_keys is None else n_keys)
    dev.sync()
    return d_arena.cpu().numpy(), d_len.cpu().numpy()[:len(pkts)], d_ctr.cpu().numpy().view(np.uint64)[:len(pkts)]


def first_diff(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.flatnonzero(got != want)
    return "equal" if len(bad) == 0 else f"{len(bad)} bytes differ, first at {int(bad[0])}, last at {int(bad[-1])}"


def pack(items, aligns=None):
    """Lay packets of the given extents out back to back (a gap of < 16 sentinel
    bytes where an alignment is asked for).  Returns (arena, offsets)."""
    offs, cur = [], 3
    for k, ext in enumerate(items):
        if aligns is not None:
            cur += (aligns[k] - cur) % 16
        offs.append(cur)
        cur += ext
    return np.full(cur + 5, SENTINEL, np.uint8), offs


def put(arena, off, b: bytes):
    arena[off:off + len(b)] = np.frombuffer(b, np.uint8)


@pytest.fixture(scope="module")
def golden():
    with open(make_aead_golden.OUT) as f:
        return json.load(f)["cases"]


def check_golden_msg(rec, msg: bytes):
    if "msg_hex" in rec:
        assert msg.hex() == rec["msg_hex"]
    else:
        assert len(msg) == rec["msg_len"] and msg[-16:].hex() == rec["tag"]
        assert msg[16:32].hex() == rec["ct_first"] and msg[-32:-16].hex() == rec["ct_last"]
        assert hashlib.sha256(msg).hexdigest() == rec["msg_sha256"]


def test_golden_per_call(dev, golden):
    for rec in golden:
        key = bytes.fromhex(rec["key"])
        packet, _ = make_aead_golden.expand(rec)
        msg = transport.seal(dev, key, rec["remote_index"], rec["counter"], packet, rec["mtu"])
        check_golden_msg(rec, msg)
        padded = packet + b"\0" * aead_ref.padding(len(packet), rec["mtu"])
        counter, got, err = transport.open_(dev, key, msg)
        want = aead_ref.trim(padded)
        assert counter == rec["counter"]
        if want < 0:
            assert err is not None and err.code == _lib.ERR_PACKET_TOO_SHORT and got == padded
        else:
            assert err is None and got == padded[:want]
        bad = bytearray(msg)
        bad[-1] ^= 1
        counter, got, err = transport.open_(dev, key, bytes(bad))
        assert err is not None and err.code == _lib.ERR_AUTH and got is None and counter == rec["counter"]


def test_per_call_argument_errors(dev):
    key = bytes(32)
    k = np.frombuffer(key, np.uint8)
    import ctypes as C
    buf = np.full(64, SENTINEL, np.uint8)
    out = C.c_size_t(99)
    # 20 bytes pad to 32 under mtu 0: 64 bytes needed, 63 given
    rc = dev.lib.wgcs_aead_seal(dev.h, k.ctypes.data, 1, 2, buf.ctypes.data, 20, 63, 0, C.byref(out))
    assert rc == _lib.ERR_OUT_OF_RANGE and (buf == SENTINEL).all()
    ctr, n = C.c_uint64(0), C.c_int(0)
    rc = dev.lib.wgcs_aead_open(dev.h, k.ctypes.data, buf.ctypes.data, 31, C.byref(ctr), C.byref(n))
    assert rc == _lib.ERR_OUT_OF_RANGE and (buf == SENTINEL).all()


def test_golden_batch(dev, golden):
    """All golden cases in one seal batch (grouped by mtu), then one open batch."""
    keys = np.zeros(len(golden), AEAD_KEY_DTYPE)
    sealed = {}
    for mtu in (0, 1420, 1500):
        idx = [i for i, r in enumerate(golden) if r["mtu"] == mtu]
        packets = [make_aead_golden.expand(golden[i])[0] for i in idx]
        exts = [32 + len(p) + aead_ref.padding(len(p), mtu) for p in packets]
        arena, offs = pack(exts)
        pkts = np.zeros(len(idx), AEAD_PKT_DTYPE)
        for j, i in enumerate(idx):
            keys[i]["key"] = np.frombuffer(bytes.fromhex(golden[i]["key"]), np.uint8)
            keys[i]["remote_index"] = golden[i]["remote_index"]
            pkts[j] = (offs[j], golden[i]["counter"], len(packets[j]), i)
            put(arena, offs[j] + 16, packets[j])
        got, out_len = run_seal(dev, arena, pkts, keys, mtu)
        assert list(out_len) == exts
        for j, i in enumerate(idx):
            sealed[i] = got[offs[j]:offs[j] + exts[j]].tobytes()
            check_golden_msg(golden[i], sealed[i])
            got[offs[j]:offs[j] + exts[j]] = SENTINEL
        assert (got == SENTINEL).all(), "a byte outside the messages changed"
    msgs = [sealed[i] for i in range(len(golden))]
    arena, offs = pack([len(m) for m in msgs])
    pkts = np.zeros(len(msgs), AEAD_PKT_DTYPE)
    want = arena.copy()
    for i, m in enumerate(msgs):
        pkts[i] = (offs[i], 0xDEAD, len(m), i)  # the descriptor's counter is not used by open
        put(arena, offs[i], m)
        packet = make_aead_golden.expand(golden[i])[0]
        put(want, offs[i], m[:16] + packet + bytes(len(m) - 32 - len(packet)) + m[-16:])
    got, pkt_len, counter = run_open(dev, arena, pkts, keys)
    assert np.array_equal(got, want), first_diff(got, want)
    assert [int(c) for c in counter] == [r["counter"] for r in golden]
    assert list(pkt_len) == [aead_ref.trim(want[offs[i] + 16:offs[i] + len(m) - 16].tobytes())
                             for i, m in enumerate(msgs)]


@pytest.mark.parametrize("mtu", [0, 1420, 1500])
def test_seal_batch_sweep(dev, mtu):
    """Every length at every off & 15, packed back to back, against the restatement."""
    rng = np.random.default_rng(1000 + mtu)
    keys = make_keys(rng)
    plain = {n: rng.bytes(n) for n in SWEEP_LENS}
    ref = {}
    for li, n in enumerate(SWEEP_LENS):  # one reference message per length, shared by the 16 alignments
        k, counter = li % 3, COUNTERS[li % len(COUNTERS)]
        ref[n] = (k, counter, aead_ref.wg_seal(key_bytes(keys, k), int(keys[k]["remote_index"]), counter, plain[n], mtu))
    order = [(n, a) for a in range(16) for n in SWEEP_LENS]
    arena, offs = pack([len(ref[n][2]) for n, _ in order], aligns=[a for _, a in order])
    pkts = np.zeros(len(order), AEAD_PKT_DTYPE)
    want = arena.copy()
    for i, (n, a) in enumerate(order):
        assert offs[i] % 16 == a
        k, counter, msg = ref[n]
        pkts[i] = (offs[i], counter, n, k)
        put(arena, offs[i] + 16, plain[n])
        put(want, offs[i], msg)
    got, out_len = run_seal(dev, arena, pkts, keys, mtu)
    assert list(out_len) == [len(ref[n][2]) for n, _ in order]
    assert np.array_equal(got, want), first_diff(got, want)


def ip_packet(rng, n: int) -> bytes:
    """n random bytes dressed as IPv4 / IPv6 with a length field that fits, or
    left as they are when too short for a header."""
    b = bytearray(rng.bytes(n))
    if n >= 40 and n % 2:
        b[0] = 0x60 | (b[0] & 15)
        b[4:6] = (n - 40).to_bytes(2, "big")
    elif n >= 20:
        b[0] = 0x45
        b[2:4] = n.to_bytes(2, "big")
    return bytes(b)


def test_random_corpus_seal_then_open(dev):
    rng = np.random.default_rng(512)
    keys = make_keys(rng)
    n = 512
    lens = [int(x) for x in rng.integers(0, 2048, n)]
    mtu = 1420
    packets = [ip_packet(rng, ln) for ln in lens]
    exts = [32 + ln + aead_ref.padding(ln, mtu) for ln in lens]
    arena, offs = pack(exts)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    want = arena.copy()
    for i in range(n):
        k = i % 3
        counter = int(rng.integers(0, 2**64, dtype=np.uint64))
        pkts[i] = (offs[i], counter, lens[i], k)
        put(arena, offs[i] + 16, packets[i])
        put(want, offs[i], aead_ref.wg_seal(key_bytes(keys, k), int(keys[k]["remote_index"]), counter, packets[i], mtu))
    got, out_len = run_seal(dev, arena, pkts, keys, mtu)
    assert list(out_len) == exts
    assert np.array_equal(got, want), first_diff(got, want)
    # open the sealed arena: plaintexts (zero padded) come back, lengths are trimmed
    opk = pkts.copy()
    opk["len"] = exts
    opk["counter"] = 0
    want_open = got.copy()
    for i in range(n):
        put(want_open, offs[i] + 16, packets[i] + bytes(exts[i] - 32 - lens[i]))
    got2, pkt_len, counter = run_open(dev, got, opk, keys)
    assert np.array_equal(got2, want_open), first_diff(got2, want_open)
    assert np.array_equal(counter, pkts["counter"])
    assert list(pkt_len) == [aead_ref.trim(packets[i] + bytes(exts[i] - 32 - lens[i])) for i in range(n)]
    assert sum(1 for x in pkt_len if x > 0) > 400  # the corpus really exercises the trim


def raw_msg(key: bytes, remote_index: int, counter: int, plaintext: bytes) -> bytes:
    """A transport message around exactly `plaintext` (no padding added)."""
    return struct.pack("<IIQ", 4, remote_index, counter) + aead_ref.aead_seal(key, aead_ref.wg_nonce(counter), plaintext)


def test_open_negative_cases(dev):
    rng = np.random.default_rng(77)
    keys = make_keys(rng)
    good = ip_packet(rng, 336)

    def fresh(n=336, k=0, counter=5):
        return bytearray(raw_msg(key_bytes(keys, k), 9, counter, ip_packet(rng, n) if n != 336 else good))
    cases = []  # (message, key index, expect_auth_failure)

    def flip(pos, bit=0):
        m = fresh()
        m[pos] ^= 1 << bit
        cases.append((bytes(m), 0, True))
    cases.append((bytes(fresh()), 0, False))
    flip(16)        # first ciphertext byte
    flip(-17, 7)    # last ciphertext byte
    for w in range(4):
        flip(-16 + 4 * w + w, w)  # a byte of each 16-byte tag word
    flip(8)         # the counter field
    flip(15, 7)
    cases.append((bytes(fresh(k=1)), 1, False))
    cases.append((bytes(fresh()), 2, True))   # wrong key index
    cases.append((bytes(fresh()[:-1]), 0, True))  # truncated by one byte
    ka = fresh(n=0)
    ka[-3] ^= 0x10
    cases.append((bytes(ka), 0, True))        # a keepalive with a bad tag
    cases.append((bytes(fresh(n=0, counter=2**64 - 1)), 0, False))
    cases.append((bytes(fresh(n=1421, k=2, counter=2**32)), 2, False))
    arena, offs = pack([len(m) for m, _, _ in cases])
    pkts = np.zeros(len(cases), AEAD_PKT_DTYPE)
    want = arena.copy()
    want_len, want_ctr = [], []
    for i, (m, k, bad) in enumerate(cases):
        pkts[i] = (offs[i], 0, len(m), k)
        put(arena, offs[i], m)
        ctr, pt = aead_ref.wg_open(key_bytes(keys, k), m)
        assert (pt is None) == bad
        put(want, offs[i], m[:16] + (bytes(len(m) - 32) if bad else pt) + m[-16:])
        want_len.append(_lib.ERR_AUTH if bad else aead_ref.trim(pt))
        want_ctr.append(ctr)
    got, pkt_len, counter = run_open(dev, arena, pkts, keys)
    assert list(pkt_len) == want_len
    assert [int(c) for c in counter] == want_ctr
    assert np.array_equal(got, want), first_diff(got, want)
    assert want_len.count(_lib.ERR_AUTH) == 11 and want_len[0] == 336 and 0 in want_len


def test_open_length_trim(dev):
    rng = np.random.default_rng(4)
    keys = make_keys(rng)

    def v4(total, n):
        b = bytearray(rng.bytes(n))
        b[0] = 0x45
        b[2:4] = total.to_bytes(2, "big")
        return bytes(b)

    def v6(payload, n):
        b = bytearray(rng.bytes(n))
        b[0] = 0x6A
        b[4:6] = payload.to_bytes(2, "big")
        return bytes(b)

    def ver(nibble, n):
        b = bytearray(rng.bytes(n))
        b[0] = (nibble << 4) | 5
        return bytes(b)
    T = _lib.ERR_PACKET_TOO_SHORT
    cases = [
        (v4(100, 100), 100), (v4(60, 100), 60), (v4(101, 100), T), (v4(19, 100), T), (v4(20, 100), 20),
        (v6(60, 100), 100), (v6(10, 100), 50), (v6(61, 100), T), (v6(65535, 100), 39), (v6(0, 40), 40),
        (ver(0, 64), T), (ver(5, 64), T), (ver(15, 64), T),
        (v4(19, 19), T), (v4(20, 20), 20), (v6(0, 39), T), (v6(65535, 39), T), (b"", 0),
        (v4(1420, 1424), 1420), (v6(1380, 1424), 1420),
    ]
    for p, want in cases:
        assert aead_ref.trim(p) == want
    msgs = [raw_msg(key_bytes(keys, i % 3), 1, 1000 + i, p) for i, (p, _) in enumerate(cases)]
    arena, offs = pack([len(m) for m in msgs])
    pkts = np.zeros(len(cases), AEAD_PKT_DTYPE)
    want = arena.copy()
    for i, m in enumerate(msgs):
        pkts[i] = (offs[i], 0, len(m), i % 3)
        put(arena, offs[i], m)
        put(want, offs[i], m[:16] + cases[i][0] + m[-16:])
    got, pkt_len, counter = run_open(dev, arena, pkts, keys)
    assert list(pkt_len) == [w for _, w in cases]
    assert [int(c) for c in counter] == [1000 + i for i in range(len(cases))]
    assert np.array_equal(got, want), first_diff(got, want)


def test_descriptor_errors_touch_nothing(dev):
    rng = np.random.default_rng(9)
    keys = make_keys(rng)
    arena = np.full(4096, SENTINEL, np.uint8)
    good = raw_msg(key_bytes(keys, 1), 3, 8, ip_packet(rng, 64))
    put(arena, 2000, good)
    # open: len 65536, len 31, key index = n_keys, and one good message among them
    pkts = np.zeros(4, AEAD_PKT_DTYPE)
    pkts[0] = (100, 0, 65536, 0)
    pkts[1] = (200, 0, 31, 0)
    pkts[2] = (2000, 0, len(good), 3)
    pkts[3] = (2000, 0, len(good), 1)
    want = arena.copy()
    put(want, 2000, good[:16] + aead_ref.wg_open(key_bytes(keys, 1), good)[1] + good[-16:])
    got, pkt_len, counter = run_open(dev, arena, pkts, keys)
    assert list(pkt_len) == [_lib.ERR_OUT_OF_RANGE, _lib.ERR_OUT_OF_RANGE, _lib.ERR_INVALID_ARG, 64]
    assert [int(c) for c in counter] == [0, 0, 0, 8]
    assert np.array_equal(got, want), first_diff(got, want)
    # seal: len 65536 and key index = n_keys touch nothing; len 0 beside them seals
    arena = np.full(4096, SENTINEL, np.uint8)
    pkts = np.zeros(3, AEAD_PKT_DTYPE)
    pkts[0] = (100, 1, 65536, 0)
    pkts[1] = (300, 1, 40, 3)
    pkts[2] = (501, 7, 0, 2)
    want = arena.copy()
    put(want, 501, aead_ref.wg_seal(key_bytes(keys, 2), int(keys[2]["remote_index"]), 7, b"", 1420))
    got, out_len = run_seal(dev, arena, pkts, keys, 1420)
    assert list(out_len) == [_lib.ERR_OUT_OF_RANGE, _lib.ERR_INVALID_ARG, 32]
    assert np.array_equal(got, want), first_diff(got, want)
    # n == 0 is accepted and does nothing, whatever the pointers
    got, out_len = run_seal(dev, arena, pkts, keys, 1420, n=0)
    assert np.array_equal(got, arena) and (out_len == 12345).all()
    got, pkt_len, _ = run_open(dev, arena, pkts, keys, n=0)
    assert np.array_equal(got, arena) and (pkt_len == 12345).all()
    assert dev.lib.wgcs_aead_seal_batch(dev.h, None, None, None, 0, 0, 0, None, None) == 0
    assert dev.lib.wgcs_aead_open_batch(dev.h, None, None, None, 0, 0, None, None, None) == 0


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1025])
def test_packet_counts(dev, n):
    """Row, wave and workgroup boundaries: 4 packets fill a wave, 16 a workgroup."""
    rng = np.random.default_rng(n)
    keys = make_keys(rng)
    lens = [int(x) for x in rng.integers(0, 200, n)]
    lens[-1] = 177
    packets = [ip_packet(rng, ln) for ln in lens]
    exts = [32 + ln + aead_ref.padding(ln, 0) for ln in lens]
    arena, offs = pack(exts)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    want = arena.copy()
    for i in range(n):
        pkts[i] = (offs[i], i, lens[i], i % 3)
        put(arena, offs[i] + 16, packets[i])
        put(want, offs[i], aead_ref.wg_seal(key_bytes(keys, i % 3), int(keys[i % 3]["remote_index"]), i, packets[i], 0))
    got, out_len = run_seal(dev, arena, pkts, keys, 0)
    assert list(out_len) == exts
    assert np.array_equal(got, want), first_diff(got, want)
    opk = pkts.copy()
    opk["len"] = exts
    want_open = got.copy()
    for i in range(n):
        put(want_open, offs[i] + 16, packets[i] + bytes(exts[i] - 32 - lens[i]))
    got2, pkt_len, counter = run_open(dev, got, opk, keys)
    assert np.array_equal(got2, want_open), first_diff(got2, want_open)
    assert list(counter) == list(range(n))
    assert list(pkt_len) == [aead_ref.trim(packets[i] + bytes(exts[i] - 32 - lens[i])) for i in range(n)]
