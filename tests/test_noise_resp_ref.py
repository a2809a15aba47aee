"""tests/noise_resp_ref.py against a step-by-step rebuild from hashlib and hmac,
and the host functions of the C ABI (wgcs_noise_create_response,
wgcs_noise_consume_response) against it through wireguard_amd.noise (CPU only).

A handshake runs initiator create_initiation -> responder consume_initiation ->
create_response -> initiator consume_response, with and without a preshared
key and a cookie; both sides must end with one hash and one chaining key and
with crossed transport keys."""
import hashlib
import hmac
import os
import struct
import subprocess

import numpy as np
import pytest

import aead_ref
import cookie_ref
import noise_ref
import noise_resp_ref
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, HS_CONSUMED, LOW_ORDER_POINTS
from wireguard_amd import _lib, noise

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def b2s(data: bytes) -> bytes:
    return hashlib.blake2s(data, digest_size=32).digest()


def hm(key: bytes, data: bytes) -> bytes:
    return hmac.new(key, data, lambda: hashlib.blake2s(digest_size=32)).digest()


def flip(b: bytes, i: int, bit: int = 0) -> bytes:
    return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]


class World:
    """A responder with one peer, the initiator, and a consumed initiation."""

    def __init__(self, seed: int):
        rng = self.rng = np.random.default_rng(seed)
        self.ref = noise_ref.Responder(rng.bytes(32))
        self.init_private = rng.bytes(32)
        self.init_public = noise_ref.public_key(self.init_private)
        self.table = noise_ref.PeerTable(self.ref, [(self.init_public, 7, 1)])
        self.init_eph, self.init_index = rng.bytes(32), int(rng.integers(0, 2**32))
        self.initiation, self.i_hash, self.i_chain = noise_ref.create_initiation(
            self.init_private, self.ref.public, self.init_eph, rng.bytes(12), self.init_index)
        verdict, self.row = noise_ref.consume_initiation(self.ref, self.table, self.initiation)
        assert verdict == HS_CONSUMED and self.row[32:64] == self.i_hash and self.row[64:96] == self.i_chain
        self.resp_eph, self.resp_index = rng.bytes(32), int(rng.integers(0, 2**32))


@pytest.mark.parametrize("with_cookie", [False, True], ids=["no_cookie", "cookie"])
@pytest.mark.parametrize("with_psk", [False, True], ids=["no_psk", "psk"])
def test_round_trip_and_every_step_rebuilt_from_hashlib(with_psk, with_cookie):
    w = World(494 + 2 * with_psk + with_cookie)
    psk = w.rng.bytes(32) if with_psk else None
    cookie = w.rng.bytes(16) if with_cookie else None
    status, msg, send, recv, r_hash, r_chain = noise_resp_ref.create_response(w.row, w.init_public, w.resp_eph,
                                                                              w.resp_index, psk, cookie)
    assert status == 0 and len(msg) == 92
    # ---- the responder's side again, straight from hashlib / hmac (noise.go:508-545)
    eph = noise_ref.x25519_raw(w.resp_eph, noise_ref.BASE_POINT)
    h = b2s(w.i_hash + eph)
    c = hm(hm(w.i_chain, eph), b"\x01")
    for point in (w.initiation[8:40], w.init_public):
        c = hm(hm(c, noise_ref.x25519_raw(w.resp_eph, point)), b"\x01")
    prk = hm(c, psk or bytes(32))
    c = hm(prk, b"\x01")
    tau = hm(prk, c + b"\x02")
    key = hm(prk, tau + b"\x03")
    h = b2s(h + tau)
    empty = aead_ref.aead_seal(key, bytes(12), b"", h)
    assert len(empty) == 16
    h = b2s(h + empty)
    assert msg[:60] == struct.pack("<III", 2, w.resp_index, w.init_index) + eph + empty
    assert (r_hash, r_chain) == (h, c)
    prk = hm(c, b"")
    t0 = hm(prk, b"\x01")
    t1 = hm(prk, t0 + b"\x02")
    assert (recv, send) == (t0, t1)  # KDF2(&decryptKey, &encryptKey, ...), noise.go:646-651
    # ---- AddMACs
    k1 = hashlib.blake2s(b"mac1----" + w.init_public, digest_size=32).digest()
    mac1 = hashlib.blake2s(msg[:60], key=k1, digest_size=16).digest()
    assert msg[60:76] == mac1
    assert msg[76:] == (hashlib.blake2s(msg[:76], key=cookie, digest_size=16).digest() if with_cookie else bytes(16))
    # the initiator checks MAC1 with the checker of its own public key, as CheckMAC1 does
    assert cookie_ref.Checker(w.init_public).check_mac1(msg)
    assert not cookie_ref.Checker(w.ref.public).check_mac1(msg)
    # ---- the initiator's side
    status, sender, i_send, i_recv, i_hash, i_chain = noise_resp_ref.consume_response(
        w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, msg, psk)
    assert status == 0 and sender == w.resp_index
    assert (i_hash, i_chain) == (r_hash, r_chain)
    assert i_send == recv and i_recv == send and send != recv
    # the other preshared key does not authenticate
    other = bytes(32) if with_psk else w.rng.bytes(32)
    assert noise_resp_ref.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, msg,
                                           other)[0] == ERR_AUTH


def failures(w, msg):
    """(name, message, status) for every way consume_response says no."""
    out = [("eph_first", flip(msg, 12), ERR_AUTH), ("eph_last", flip(msg, 43, 6), ERR_AUTH),
           ("tag_first", flip(msg, 44), ERR_AUTH), ("tag_last", flip(msg, 59, 7), ERR_AUTH),
           ("type", flip(msg, 0), ERR_INVALID_ARG), ("type_high", flip(msg, 3, 7), ERR_INVALID_ARG),
           ("receiver", flip(msg, 8), ERR_INVALID_ARG), ("receiver_high", flip(msg, 11, 7), ERR_INVALID_ARG),
           ("short", msg[:91], ERR_INVALID_ARG), ("long", msg + b"\0", ERR_INVALID_ARG)]
    out += [(f"low_order_{i}", msg[:12] + u + msg[44:], ERR_LOW_ORDER) for i, u in enumerate(LOW_ORDER_POINTS)]
    return out


@pytest.mark.parametrize("with_psk", [False, True], ids=["no_psk", "psk"])
def test_every_failure_of_consume_response(with_psk):
    w = World(573 + with_psk)
    psk = w.rng.bytes(32) if with_psk else None
    msg = noise_resp_ref.create_response(w.row, w.init_public, w.resp_eph, w.resp_index, psk, w.rng.bytes(16))[1]
    for name, bad, want in failures(w, msg):
        got = noise_resp_ref.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, bad, psk)
        assert got == (want, None, bytes(32), bytes(32), None, None), name
        rc, sender, send, recv = noise.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index,
                                                        bad, psk)
        assert (rc, sender, send, recv) == (want, None, bytes(32), bytes(32)), name
    # MACs are the screen's: any bytes there consume alike
    ok = noise.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index,
                                msg[:60] + w.rng.bytes(32), psk)
    assert ok[0] == 0 and ok == noise.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index,
                                                       msg, psk)
    # another handshake's state
    assert noise.consume_response(w.init_private, w.i_hash, flip(w.i_chain, 0), w.init_eph, w.init_index, msg,
                                  psk)[0] == ERR_AUTH
    assert noise.consume_response(w.init_private, w.i_hash, w.i_chain, w.rng.bytes(32), w.init_index, msg,
                                  psk)[0] == ERR_AUTH


@pytest.mark.parametrize("with_cookie", [False, True], ids=["no_cookie", "cookie"])
@pytest.mark.parametrize("with_psk", [False, True], ids=["no_psk", "psk"])
def test_host_functions_match_the_restatement(with_psk, with_cookie):
    w = World(646 + 2 * with_psk + with_cookie)
    r, pub = noise.responder_init(w.ref.private)
    table = noise.peer_keys_build(r, [w.init_public], [7])
    verdict, row = noise.consume_initiation(r, table, w.initiation)
    assert verdict == HS_CONSUMED and row.tobytes() == w.row
    for _ in range(3):
        psk = w.rng.bytes(32) if with_psk else None
        cookie = w.rng.bytes(16) if with_cookie else None
        eph, index = w.rng.bytes(32), int(w.rng.integers(0, 2**32))
        want = noise_resp_ref.create_response(w.row, w.init_public, eph, index, psk, cookie)
        got = noise.create_response(row, w.init_public, eph, index, psk, cookie)
        assert got == want[:4] and got[0] == 0
        want_i = noise_resp_ref.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, got[1], psk)
        got_i = noise.consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, w.init_index, got[1], psk)
        assert got_i == want_i[:4] and got_i[0] == 0
        assert got_i[1] == index and got_i[2] == got[3] and got_i[3] == got[2]
    # an explicit all-zero preshared key is no preshared key
    assert noise.create_response(row, w.init_public, eph, index, bytes(32), cookie) == \
        noise.create_response(row, w.init_public, eph, index, None, cookie)


def test_low_order_inputs_of_create_response():
    w = World(520)
    r, _ = noise.responder_init(w.ref.private)
    row = np.frombuffer(w.row, noise.HS_INIT_DTYPE).copy()
    zeros = (ERR_LOW_ORDER, bytes(92), bytes(32), bytes(32))
    for u in LOW_ORDER_POINTS:
        bad = row.copy()
        bad["ephemeral"][0] = np.frombuffer(u, np.uint8)       # sharedSecret(hs.remoteEphemeral), noise.go:520-523
        assert noise_resp_ref.create_response(bad.tobytes(), w.init_public, w.resp_eph, 1)[:4] == zeros
        assert noise.create_response(bad, w.init_public, w.resp_eph, 1) == zeros
        assert noise_resp_ref.create_response(w.row, u, w.resp_eph, 1)[:4] == zeros   # hs.remoteStatic, :525-528
        assert noise.create_response(row, u, w.resp_eph, 1, cookie=bytes(16)) == zeros
    # optional outputs and NULL arguments on the raw ABI
    L = _lib.load()
    import ctypes as C
    msg = C.create_string_buffer(92)
    assert L.wgcs_noise_create_response(row.ctypes.data, w.init_public, None, w.resp_eph, 5, None, msg, None, None) == 0
    assert msg.raw == noise.create_response(row, w.init_public, w.resp_eph, 5)[1]
    for args in ((None, w.init_public, None, w.resp_eph, 5, None, msg, None, None),
                 (row.ctypes.data, None, None, w.resp_eph, 5, None, msg, None, None),
                 (row.ctypes.data, w.init_public, None, None, 5, None, msg, None, None),
                 (row.ctypes.data, w.init_public, None, w.resp_eph, 5, None, None, None, None)):
        assert L.wgcs_noise_create_response(*args) == ERR_INVALID_ARG
    good = msg.raw
    assert L.wgcs_noise_consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, None, w.init_index, good, 92,
                                         None, None, None) == 0
    for k in range(4):
        args = [w.init_private, w.i_hash, w.i_chain, w.init_eph, None, w.init_index, good, 92, None, None, None]
        args[k] = None
        assert L.wgcs_noise_consume_response(*args) == ERR_INVALID_ARG
    assert L.wgcs_noise_consume_response(w.init_private, w.i_hash, w.i_chain, w.init_eph, None, w.init_index, None, 92,
                                         None, None, None) == ERR_INVALID_ARG
    with pytest.raises(ValueError):
        noise.create_response(row, w.init_public, bytes(31), 1)
    with pytest.raises(ValueError):
        noise.create_response(row, w.init_public, w.resp_eph, 1, cookie=bytes(15))


def test_respond_row_of_the_restatement_orders_its_conditions():
    w = World(130)
    other = noise_ref.hs_init_bytes(8, 1, bytes(12), w.row[32:64], w.row[64:96], w.row[96:128])
    rows, table = [w.row, other], w.table.rows
    d = dict(init_row=0, peer_row=0, local_index=9, send_key=2, recv_key=3, flags=0, ephemeral_private=w.resp_eph,
             cookie=bytes(16))
    status, msg, keys = noise_resp_ref.respond_row(d, rows, [HS_CONSUMED, HS_CONSUMED], table, None, 4)
    want = noise_resp_ref.create_response(w.row, w.init_public, w.resp_eph, 9)
    assert status == noise_resp_ref.HS_RESPONDED and msg == want[1] + bytes(4)
    assert keys == {2: want[2] + struct.pack("<I", w.init_index) + bytes(12), 3: want[3] + bytes(16)}
    for change in (dict(init_row=2), dict(peer_row=1), dict(send_key=4), dict(recv_key=4), dict(recv_key=2)):
        assert noise_resp_ref.respond_row({**d, **change}, rows, [0, 0], table, None, 4) == (ERR_INVALID_ARG, None, {})
    assert noise_resp_ref.respond_row(d, rows, [noise_ref.ERR_AUTH, HS_CONSUMED], table, None, 4) == (0, None, {})
    assert noise_resp_ref.respond_row({**d, "init_row": 1}, rows, None, table, None, 4) == (noise_ref.ERR_NO_PEER, None, {})
    # the gate comes before the peer comparison
    assert noise_resp_ref.respond_row({**d, "init_row": 1}, rows, [HS_CONSUMED, 0], table, None, 4)[0] == 0


def test_constants_and_layout_of_the_descriptor(tmp_path):
    assert (noise.HS_RESPONDED, _lib.HS_RESPONDED, _lib.HS_RESP_COOKIE) == (4, 4, 1)
    src = tmp_path / "t.c"
    src.write_text('#include "wgcsum.h"\n#include <stddef.h>\n'
                   '_Static_assert(sizeof(wgcs_hs_resp) == 80 && offsetof(wgcs_hs_resp, init_row) == 0 && '
                   'offsetof(wgcs_hs_resp, peer_row) == 4 && offsetof(wgcs_hs_resp, local_index) == 8 && '
                   'offsetof(wgcs_hs_resp, send_key) == 12 && offsetof(wgcs_hs_resp, recv_key) == 16 && '
                   'offsetof(wgcs_hs_resp, flags) == 20 && offsetof(wgcs_hs_resp, pad) == 24 && '
                   'offsetof(wgcs_hs_resp, ephemeral_private) == 32 && offsetof(wgcs_hs_resp, cookie) == 64, "hs_resp");\n'
                   '_Static_assert(_Alignof(wgcs_hs_resp) == 4, "alignment");\n'
                   '_Static_assert(sizeof(wgcs_hs_init) == 128 && sizeof(wgcs_aead_key) == 48 && '
                   'offsetof(wgcs_aead_key, remote_index) == 32, "neighbours keep their layout");\n'
                   '_Static_assert(WGCS_HS_RESPONDED == 4 && WGCS_HS_CONSUMED == 3 && WGCS_HS_RESP_COOKIE == 1, "codes");\n'
                   "int main(void) { return 0; }\n")
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)
    want = {"init_row": 0, "peer_row": 4, "local_index": 8, "send_key": 12, "recv_key": 16, "flags": 20, "pad": 24,
            "ephemeral_private": 32, "cookie": 64}
    assert {name: noise.HS_RESP_DTYPE.fields[name][1] for name in want} == want and noise.HS_RESP_DTYPE.itemsize == 80
