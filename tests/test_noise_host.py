"""The scalar code of X25519 and of the handshake consume step
(wireguard_amd/csrc/wgcs_x25519.h, wgcs_noise.h and the host functions of
noise.cpp) as host code under AddressSanitizer + UBSan, against
tests/noise_ref.py (CPU only).

tests/noise_host/noise_host.cpp is a stand-alone program that includes the
headers the kernel includes and links noise.cpp as it is.  Every input sits in
a heap buffer of exactly its size, so a byte read outside a key, a point, a
table or a message is a sanitizer report, and an unsigned overflow of a limb
or a shift out of range is a UBSan one, not a wrong result that happens to be
right."""
import hashlib
import hmac
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import aead_ref
import noise_ref
from noise_ref import (ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, ERR_NO_PEER, HS_CONSUMED, LOW_ORDER_POINTS, P,
                       PEER_NONE)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "wireguard_amd", "csrc")
SRC = os.path.join(HERE, "noise_host", "noise_host.cpp")
GOLDEN = os.path.join(HERE, "golden", "x25519_vectors.json")
FILL = b"\xee" * 128  # what the program fills a wgcs_hs_init with before the call


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("noise") / "noise_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC, os.path.join(CSRC, "noise.cpp")],
                   check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[-2:] == ["noise_host:", "ok"]
    got = out[:-2]
    assert len(got) == len(lines)
    return got


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def le(n: int) -> bytes:
    return n.to_bytes(32, "little")


def flip(b: bytes, i: int, bit: int = 0) -> bytes:
    return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]


RFC_1 = ("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4",
         "e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c",
         "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")
RFC_2 = ("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d",
         "e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493",
         "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957")


def test_x25519_rfc_vectors_and_iteration(prog):
    lines = [f"x {k} {u}" for k, u, _ in (RFC_1, RFC_2)] + ["xiter 1", "xiter 1000"]
    want = [RFC_1[2], RFC_2[2], "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079",
            "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"]
    assert run(prog, lines) == want


def test_x25519_golden_file(prog):
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 200
    assert run(prog, [f"x {c['scalar']} {c['u']}" for c in cases]) == [c["out"] for c in cases]


def test_x25519_edge_points_and_scalars(prog):
    rng = np.random.default_rng(25519)
    lines, want = [], []
    scalars = [rng.bytes(32), bytes(32), b"\xff" * 32, bytes.fromhex(RFC_1[0])]
    for k in scalars:
        for u in LOW_ORDER_POINTS:  # u = 0, 1, p - 1, p, p + 1
            assert noise_ref.x25519(k, u) is None
            lines.append(f"x {k.hex()} {u.hex()}")
            want.append("low")
            lines.append(f"x {k.hex()} {flip(u, 31, 7).hex()}")  # bit 255 is ignored
            want.append("low")
        # u = 2^255 - 1 is 18 after reduction, p + 2 is 2, and bit 255 changes nothing
        pairs = [(le(2**255 - 1), le(18)), (le(2**256 - 1), le(18)), (le(P + 2), le(2)), (le(P + 2 + 2**255), le(2))]
        u = rng.bytes(32)
        pairs.append((flip(u, 31, 7), bytes(u[:31]) + bytes([u[31] & 0x7F])))
        for u, reduced in pairs:
            out = noise_ref.x25519(k, u)
            assert out is not None and out == noise_ref.x25519(k, reduced)
            lines.append(f"x {k.hex()} {u.hex()}")
            want.append(out.hex())
        for u in (le(2), le(9), le(P - 2), le(2**254), rng.bytes(32)):
            lines.append(f"x {k.hex()} {u.hex()}")
            want.append(noise_ref.x25519_raw(k, u).hex())
    assert run(prog, lines) == want


def _hmac(key, *parts):
    return hmac.new(key, b"".join(parts), lambda: hashlib.blake2s(digest_size=32)).digest()


def test_hmac_and_kdfs_against_hashlib(prog):
    rng = np.random.default_rng(5869)
    lines, want = [], []
    for n in (0, 1, 32, 33, 63, 64):
        for key in (rng.bytes(32), bytes(32), b"\xff" * 32):
            data = rng.bytes(n) if n else b""
            lines.append(f"hmac {key.hex()} {hx(data)}")
            want.append(_hmac(key, data).hex())
            prk = _hmac(key, data)
            t0 = _hmac(prk, b"\x01")
            t1 = _hmac(prk, t0, b"\x02")
            t2 = _hmac(prk, t1, b"\x03")
            lines += [f"kdf1 {key.hex()} {hx(data)}", f"kdf2 {key.hex()} {hx(data)}", f"kdf3 {key.hex()} {hx(data)}"]
            want += [t0.hex(), (t0 + t1).hex(), (t0 + t1 + t2).hex()]
            assert (t0, t1, t2) == noise_ref.kdf3(key, data) and t0 == noise_ref.kdf1(key, data)
    for _ in range(4):
        key, in0, in1 = rng.bytes(32), rng.bytes(32), rng.bytes(1)
        lines.append(f"hmac2 {key.hex()} {in0.hex()} {in1.hex()}")
        want.append(_hmac(key, in0, in1).hex())
    for n in (0, 1, 12, 28, 31, 32, 33, 34, 48):
        h, data = rng.bytes(32), rng.bytes(n) if n else b""
        lines.append(f"mixhash {h.hex()} {hx(data)}")
        want.append(hashlib.blake2s(h + data, digest_size=32).hexdigest())
    assert run(prog, lines) == want


def test_initial_values_and_aead(prog):
    assert noise_ref.INITIAL_CHAIN_KEY == hashlib.blake2s(b"Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s").digest()
    rng = np.random.default_rng(8439)
    lines, want = [], []
    for trial in range(8):
        key, ad = rng.bytes(32), rng.bytes(32)
        if trial == 0:
            key, ad = b"\xff" * 32, b"\xff" * 32
        for n in (0, 12, 32):
            pt = (b"\xff" * n if trial == 0 else rng.bytes(n)) if n else b""
            sealed = aead_ref.aead_seal(key, bytes(12), pt, ad)
            lines.append(f"seal {key.hex()} {hx(pt)} {ad.hex()}")
            want.append(sealed.hex())
            lines.append(f"open {key.hex()} {sealed.hex()} {ad.hex()}")
            want.append(hx(pt))
            bads = [flip(sealed, n), flip(sealed, n + 15, 7)] + ([flip(sealed, 0), flip(sealed, n - 1, 7)] if n else [])
            for bad in bads:
                lines.append(f"open {key.hex()} {bad.hex()} {ad.hex()}")
                want.append("fail")
            lines.append(f"open {key.hex()} {sealed.hex()} {flip(ad, 31, 7).hex()}")
            want.append("fail")
            lines.append(f"open {flip(key, 0).hex()} {sealed.hex()} {ad.hex()}")
            want.append("fail")
    assert run(prog, lines) == want


class World:
    """A responder, a table of peers -- a not-running one and one whose public
    key is a low-order point among them -- and an initiator with an entry."""

    def __init__(self, seed, n_peers=37):
        rng = self.rng = np.random.default_rng(seed)
        self.ref = noise_ref.Responder(rng.bytes(32))
        self.init_private = rng.bytes(32)
        self.init_public = noise_ref.public_key(self.init_private)
        self.stopped_private = rng.bytes(32)
        self.low_public = le(1)
        peers = [(self.init_public, 7, 1), (noise_ref.public_key(self.stopped_private), 8, 0), (self.low_public, 9, 1)]
        peers += [(noise_ref.public_key(rng.bytes(32)), 100 + i, 1) for i in range(n_peers - 3)]
        self.peers = peers
        self.table = noise_ref.PeerTable(self.ref, peers)

    def initiation(self, private=None, **kw):
        rng = self.rng
        return noise_ref.create_initiation(self.init_private if private is None else private, self.ref.public,
                                           rng.bytes(32), rng.bytes(12), int(rng.integers(0, 2**32)), **kw)


def test_responder_and_peer_table(prog):
    w = World(405)
    r, keys = w.ref.tobytes(), [p[0] for p in w.peers]
    ids = b"".join(struct.pack("<I", p[1]) for p in w.peers)
    flags = b"".join(struct.pack("<I", p[2]) for p in w.peers)
    table = w.table.tobytes()
    sorted_keys = [row[0] for row in w.table.rows]
    assert sorted_keys == sorted(keys) and w.table.rows[w.table.find(w.low_public)][1] == bytes(32)
    absent = w.rng.bytes(32)
    lines = [f"init {w.ref.private.hex()}",
             f"build {r.hex()} {b''.join(keys).hex()} {ids.hex()} {flags.hex()}",
             f"build {r.hex()} - - -",                                          # n = 0
             f"build {r.hex()} {keys[0].hex()} {ids[:4].hex()} -",              # n = 1, flags NULL: running
             f"build {r.hex()} {(keys[0] + keys[1] + keys[0]).hex()} {ids[:12].hex()} -",   # a duplicate key
             f"build {r.hex()} {keys[0].hex()} {struct.pack('<I', PEER_NONE).hex()} -",
             f"find {table.hex()} {sorted_keys[0].hex()}", f"find {table.hex()} {sorted_keys[-1].hex()}",
             f"find {table.hex()} {sorted_keys[17].hex()}", f"find {table.hex()} {absent.hex()}",
             f"find {table.hex()} {bytes(32).hex()}", f"find {table.hex()} {'ff' * 32}",
             f"find - {absent.hex()}", f"find {table[:72].hex()} {sorted_keys[0].hex()}",
             f"find {table[:72].hex()} {sorted_keys[1].hex()}"]
    one = noise_ref.PeerTable(w.ref, [(keys[0], w.peers[0][1], 1)]).tobytes()
    want = [(r + w.ref.public).hex(), table.hex(), "-", one.hex(), str(ERR_INVALID_ARG), str(ERR_INVALID_ARG),
            "0", "36", "17", "-1", "-1", "-1", "-1", "0", "-1"]
    assert run(prog, lines) == want


def test_create_and_consume_round_trip_and_every_failure(prog):
    w = World(457)
    r, table = w.ref.tobytes().hex(), w.table.tobytes().hex()
    lines, want = [], []

    def case(msg, verdict=None, other_table=None):
        t = w.table if other_table is None else other_table
        v, row = noise_ref.consume_initiation(w.ref, t, msg)
        assert verdict is None or v == verdict, (v, verdict)
        lines.append(f"consume {r} {hx(t.tobytes())} {msg.hex()}")
        want.append(f"{v}:{(FILL if row is None else row).hex()}")
        return row

    for _ in range(3):
        rng = w.rng
        eph, ts, sender = rng.bytes(32), rng.bytes(12), int(rng.integers(0, 2**32))
        msg, h, chain = noise_ref.create_initiation(w.init_private, w.ref.public, eph, ts, sender)
        lines.append(f"create {w.init_private.hex()} {w.ref.public.hex()} {eph.hex()} {ts.hex()} "
                     f"{struct.pack('<I', sender).hex()}")
        want.append((msg + h + chain).hex())
        row = case(msg, HS_CONSUMED)
        assert row == noise_ref.hs_init_bytes(7, sender, ts, h, chain, msg[8:40])
        # MACs are not the consume step's: any bytes there give the same row
        assert case(msg[:116] + rng.bytes(32), HS_CONSUMED) == row
    good = w.initiation()[0]
    # a flipped byte in each field: first and last byte of each
    for i in (8, 39):
        case(flip(good, i), ERR_AUTH)             # ephemeral: another shared secret, the static field does not open
    for i in (40, 71, 72, 87):
        row = case(flip(good, i, 7), ERR_AUTH)    # static ciphertext, static tag
        assert row[:4] == struct.pack("<I", PEER_NONE) and row[8:] == bytes(120)
    for i in (88, 99, 100, 115):
        row = case(flip(good, i), ERR_AUTH)       # timestamp ciphertext, timestamp tag: the peer is known by then
        assert row[:4] == struct.pack("<I", 7) and row[8:] == bytes(120)
    stranger = w.initiation(private=w.rng.bytes(32))[0]
    row = case(stranger, ERR_NO_PEER)             # an unknown static key
    assert row[:4] == struct.pack("<I", PEER_NONE) and row[8:] == bytes(120)
    row = case(w.initiation(private=w.stopped_private)[0], ERR_NO_PEER)  # a peer that is not running
    assert row[:4] == struct.pack("<I", 8)
    # an initiator whose public key is a low-order point: its row's shared secret is zero
    row = case(w.initiation(static_public=w.low_public, precomputed=w.rng.bytes(32))[0], ERR_NO_PEER)
    assert row[:4] == struct.pack("<I", 9) and row[8:] == bytes(120)
    for u in LOW_ORDER_POINTS:
        case(good[:8] + u + good[40:], ERR_LOW_ORDER)  # a low-order ephemeral
    case(struct.pack("<I", 2) + good[4:], ERR_INVALID_ARG)   # a wrong type word
    case(struct.pack("<I", 0x101) + good[4:], ERR_INVALID_ARG)
    case(good[:147], ERR_INVALID_ARG)
    case(good + b"\0", ERR_INVALID_ARG)
    # tables of 0 and 1 rows
    case(good, ERR_NO_PEER, noise_ref.PeerTable(w.ref, []))
    case(good, HS_CONSUMED, noise_ref.PeerTable(w.ref, [w.peers[0]]))
    case(stranger, ERR_NO_PEER, noise_ref.PeerTable(w.ref, [w.peers[0]]))
    # the sender's side refuses a low-order remote static key
    lines.append(f"create {w.init_private.hex()} {le(1).hex()} {w.rng.bytes(32).hex()} {bytes(12).hex()} 00000000")
    want.append(str(ERR_LOW_ORDER))
    assert run(prog, lines) == want
