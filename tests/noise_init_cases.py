"""Cases for the handshake initiator (test infrastructure only), shared by
tests/test_noise_init_ref.py (CPU) and tests/test_gpu_noise_init.py (GPU): an
initiator with 37 peers, batches of wgcs_hs_start descriptors that meet every
row of wgcs_handshake_initiate_batch's status table, and receive batches of
responses that meet every row of wgcs_handshake_finish_batch's.

The responders are played by the host functions of the C ABI
(wgcs_noise_consume_initiation, wgcs_noise_create_response), which
tests/test_noise_ref.py and tests/test_noise_resp_ref.py pin to the
restatements; everything is generated from seeds."""
from __future__ import annotations

import functools
import struct
from types import SimpleNamespace

import numpy as np

import noise_ref
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, HS_CONSUMED, HS_NONE, HS_PASS, LOW_ORDER_POINTS
from wireguard_amd import noise, router
from wireguard_amd.noise import HS_START_DTYPE, HS_STATE_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

HS_INITIATED, HS_FINISHED, ERR_NO_HANDSHAKE = 5, 6, -24
N_PEERS = 37
SENTINEL, STATUS_FILL = 0xA5, 12345
SPARE = 3  # rows of every output past the batch and past each table: they keep their fill
PITCH, WORK = 160, 64
RESP_PITCH = 97  # responses sit at 1 + 97 q: every alignment of the dword loads


def le(n: int) -> bytes:
    return n.to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def world():
    """The initiator (private key, its wgcs_noise_responder row, public key), 36
    peers whose private keys the tests hold plus one whose public key is a
    low-order point, the initiator's peer table and the preshared keys by table
    row (every fifth peer has none)."""
    rng = np.random.default_rng(344)
    w = SimpleNamespace()
    w.private = rng.bytes(32)
    w.responder, w.public = noise.responder_init(w.private)
    privs = [rng.bytes(32) for _ in range(N_PEERS - 1)]
    pubs = [noise.x25519(k, noise_ref.BASE_POINT) for k in privs]
    w.low_peer = 99
    w.table = noise.peer_keys_build(w.responder, pubs + [le(1)], [100 + i for i in range(N_PEERS - 1)] + [w.low_peer])
    w.row_of_peer = {int(r["peer"]): i for i, r in enumerate(w.table)}
    w.low_row = w.row_of_peer[w.low_peer]
    assert not w.table["shared"][w.low_row].any()
    w.private_of_row = {w.row_of_peer[100 + i]: privs[i] for i in range(N_PEERS - 1)}
    w.good_rows = sorted(w.private_of_row)
    w.psk = np.frombuffer(rng.bytes(32 * N_PEERS), np.uint8).reshape(N_PEERS, 32).copy()
    w.psk[::5] = 0
    return w


@functools.lru_cache(maxsize=None)
def peer_side(row: int):
    """The peer of table row `row` as a responder that knows the initiator."""
    w = world()
    responder, public = noise.responder_init(w.private_of_row[row])
    assert public == w.table["public_key"][row].tobytes()
    return responder, noise.peer_keys_build(responder, [w.public], [1])


def _fresh_indices(rng, n):
    out = set()
    while len(out) < n:
        out.add(int(rng.integers(1, 2**32 - 1)))
    return sorted(out, key=lambda _: rng.random())


@functools.lru_cache(maxsize=None)
def start_batch(n: int, plain: bool = False):
    """(n wgcs_hs_start descriptors, n_states, n_keys): state row j and key rows 2j
    and 2j + 1 for descriptor j.  Unless `plain`, they cycle through every row of
    the status table: each index out of range (by one, by far and 0xFFFFFFFF),
    send_key == recv_key, the low-order peer, flag words with junk above bit 0,
    the cookie on and off."""
    w = world()
    rng = np.random.default_rng(5000 + 2 * n + plain)
    n_states, n_keys = n, 2 * n
    d = np.zeros(n, HS_START_DTYPE)
    index = _fresh_indices(rng, n)
    for j in range(n):
        k, c = (j % 16, j // 16) if n > 1 and not plain else (0, 0)
        d["state_row"][j], d["send_key"][j], d["recv_key"][j] = j, 2 * j, 2 * j + 1
        d["peer_row"][j] = w.good_rows[(7 * j + 3) % len(w.good_rows)]
        d["flags"][j] = j & 1 if k != 1 else 0xFFFFFFFE | (c & 1)  # only bit 0 means anything
        if k == 8:
            d["state_row"][j] = (n_states, 0xFFFFFFFF, n_states + 7)[c % 3]
        elif k == 9:
            d["peer_row"][j] = (N_PEERS, 0xFFFFFFFF)[c % 2]
        elif k == 10:
            d["send_key"][j] = (n_keys, 0xFFFFFFFF)[c % 2]
        elif k == 11:
            d["recv_key"][j] = (n_keys, 0x80000000)[c % 2]
        elif k == 12:
            d["recv_key"][j] = d["send_key"][j]
        elif k == 13:
            d["peer_row"][j] = w.low_row
        d["local_index"][j] = index[j]
        d["timestamp"][j] = np.frombuffer(rng.bytes(12), np.uint8)
        d["ephemeral_private"][j] = np.frombuffer(rng.bytes(32), np.uint8)
        d["cookie"][j] = np.frombuffer(rng.bytes(16), np.uint8)
        d["pad0"][j] = np.frombuffer(rng.bytes(4), np.uint8)  # not looked at
        d["pad1"][j] = np.frombuffer(rng.bytes(8), np.uint8)
    return d, n_states, n_keys


def initiate_outputs(n: int, n_states: int):
    """(states, msgs, status) filled with their sentinels, SPARE rows longer than the tables."""
    return (np.full((n_states + SPARE) * 128, SENTINEL, np.uint8).view(HS_STATE_DTYPE),
            np.full((n + SPARE) * PITCH, SENTINEL, np.uint8), np.full(n + SPARE, STATUS_FILL, np.int32))


@functools.lru_cache(maxsize=None)
def initiate_expect(n: int, plain: bool = False):
    """What wgcs_handshake_initiate_host leaves for start_batch(n, plain)."""
    w = world()
    d, n_states, n_keys = start_batch(n, plain)
    states, msgs, status = initiate_outputs(n, n_states)
    noise.initiate_host(d, w.public, w.table, states[:n_states], msgs, status, n_keys)
    return states, msgs, status


def response_to(msg148: bytes, peer_row: int, eph: bytes, index: int, cookie: bytes | None) -> bytes:
    """The peer of `peer_row` consumes the initiation and answers it."""
    w = world()
    responder, table = peer_side(peer_row)
    verdict, init = noise.consume_initiation(responder, table, msg148)
    assert verdict == HS_CONSUMED
    psk = w.psk[peer_row].tobytes()
    rc, msg, _, _ = noise.create_response(init, w.public, eph, index, psk if any(psk) else None, cookie)
    assert rc == 0
    return msg


def flip(b: bytes, i: int, bit: int = 0) -> bytes:
    return b[:i] + bytes([b[i] ^ (1 << bit)]) + b[i + 1:]


# what each kind of row must report
KIND_VERDICT = {"good": HS_FINISHED, "type_word": ERR_INVALID_ARG, "length": ERR_INVALID_ARG, "peer_row": ERR_INVALID_ARG,
                "key_row": ERR_INVALID_ARG, "unknown": ERR_NO_HANDSHAKE, "zeroed": ERR_NO_HANDSHAKE,
                "slot_past": ERR_NO_HANDSHAKE, "other_index": ERR_NO_HANDSHAKE, "low_order": ERR_LOW_ORDER,
                "tag": ERR_AUTH, "gated": HS_NONE, "type_1": HS_NONE, "forged": ERR_AUTH, "first": HS_FINISHED,
                "copy": ERR_NO_HANDSHAKE}
CYCLE = {3: ("type_word", "length", "peer_row", "key_row"), 5: ("unknown", "zeroed", "slot_past", "other_index"),
         7: ("low_order",), 8: ("tag",), 10: ("gated",), 11: ("type_1",), 13: ("forged",), 14: ("first",), 15: ("copy",)}


@functools.lru_cache(maxsize=None)
def finish_case(n: int):
    """A receive batch of n rows for wgcs_handshake_finish_batch over states that
    wgcs_handshake_initiate_host made from plain descriptors, one handshake per
    row that needs one: the inputs, the kind of every row and the few words of
    the state table that are edited after the initiate step (a zeroed state, a
    peer row and a key row out of range)."""
    w = world()
    rng = np.random.default_rng(7000 + n)
    kinds = []
    for q in range(n):
        names = CYCLE.get(q % 16, ("good",)) if n > 1 else ("good",)
        kinds.append(names[(q // 16) % len(names)])
    if n >= 290:
        kinds[n - 1] = "late_copy"  # of row 0's response, from another workgroup
    needs = [k not in ("unknown", "slot_past", "type_1", "copy", "first", "late_copy") for k in kinds]
    hs_of_row, h = [], 0
    for q, k in enumerate(kinds):
        if k in ("first", "copy"):
            hs_of_row.append(hs_of_row[q - 1])  # the triple forged / first / copy shares one handshake
        elif k == "late_copy":
            hs_of_row.append(hs_of_row[0])
        elif needs[q]:
            hs_of_row.append(h)
            h += 1
        else:
            hs_of_row.append(None)
    n_hs = h + 1  # one more, which no response names: it stays in flight
    d, n_states, n_keys = start_batch(n_hs, plain=True)
    states, msgs, status = (a.copy() for a in initiate_expect(n_hs, plain=True))
    assert (status[:n_hs] == HS_INITIATED).all()
    edits = []  # (state row, field, value), applied to the table between the two steps
    index_of, key_of = list(d["local_index"]), list(range(n_hs))
    past_index, stray_index, unknown_index = (int(x) for x in _fresh_indices(rng, 3))
    assert not {past_index, stray_index, unknown_index} & set(int(x) for x in index_of)
    index_of += [past_index, stray_index]
    key_of += [n_states + 5, n_hs - 1]  # a row past the table, and the row of a handshake under another index
    slots = router.session_table(np.array(index_of, np.uint32), np.array(key_of, np.uint32))
    arena = np.full(1 + RESP_PITCH * n + 64, SENTINEL, np.uint8)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    types, gate = np.full(n, 2, np.int32), np.full(n, HS_PASS, np.int32)
    sender = np.zeros(n, np.uint32)
    low = 0
    for q, k in enumerate(kinds):
        hs = hs_of_row[q]
        if k in ("copy", "late_copy"):
            src = 0 if k == "late_copy" else q - 1
            msg = arena[int(pkts["off"][src]):int(pkts["off"][src]) + 92].tobytes()
            sender[q] = sender[src]
        elif hs is None:
            receiver = unknown_index if k != "slot_past" else past_index
            msg = struct.pack("<III", 2, int(rng.integers(0, 2**32)), receiver) + rng.bytes(80)
        elif k == "forged":
            msg = bytes(92)  # the row that follows writes it
        else:
            sender[q] = int(rng.integers(0, 2**32))
            cookie = rng.bytes(16) if q & 1 else None
            msg = response_to(msgs[PITCH * hs:PITCH * hs + 148].tobytes(), int(d["peer_row"][hs]), rng.bytes(32),
                              int(sender[q]), cookie)
            if k == "first":  # the authentic response of the handshake whose forged copy sits one row lower
                arena[int(pkts["off"][q - 1]):int(pkts["off"][q - 1]) + 92] = np.frombuffer(flip(msg, 50, 3), np.uint8)
        length = 92
        if k == "type_word":
            msg = struct.pack("<I", (1, 0x102, 4)[(q // 16) % 3]) + msg[4:]
        elif k == "length":
            length = (91, 93, 148)[(q // 16) % 3]
        elif k == "peer_row":
            edits.append((hs, "peer_row", (N_PEERS, 0xFFFFFFFF)[(q // 64) % 2]))
        elif k == "key_row":
            edits.append((hs, ("send_key", "recv_key")[(q // 64) % 2], n_keys))
        elif k == "zeroed":
            edits.append((hs, "state", 0))
        elif k == "other_index":
            msg = msg[:8] + struct.pack("<I", stray_index) + msg[12:]
        elif k == "low_order":
            msg = msg[:12] + LOW_ORDER_POINTS[low % len(LOW_ORDER_POINTS)] + msg[44:]
            low += 1
        elif k == "tag":
            msg = flip(msg, 44 + q % 16, q % 8)
        elif k == "gated":
            gate[q] = (HS_NONE, 2, -21)[(q // 16) % 3]  # not this step's, a cookie reply was sent, MAC1 failed
        elif k == "type_1":
            types[q] = (1, 0, 4, 3)[(q // 16) % 4]
        off = 1 + RESP_PITCH * q
        if k != "forged":  # written by the row that follows
            arena[off:off + 92] = np.frombuffer(msg[:92], np.uint8)
        pkts[q] = (off, 0, length, 0xFFFFFFFF)
    for row, field, value in edits:
        states[field][row] = value
    want = np.array([KIND_VERDICT["copy" if k == "late_copy" else k] for k in kinds], np.int32)
    return SimpleNamespace(n=n, kinds=kinds, hs_of_row=hs_of_row, n_hs=n_hs, start=d, n_states=n_states, n_keys=n_keys,
                           states=states, msgs=msgs, edits=edits, slots=slots, arena=arena, pkts=pkts, types=types,
                           gate=gate, sender=sender, want=want)


def finish_outputs(c):
    """(keys, work, verdict) filled with their sentinels, SPARE rows longer than the batch and the table."""
    return (np.full((c.n_keys + SPARE) * 48, SENTINEL, np.uint8).view(AEAD_KEY_DTYPE),
            np.full((c.n + SPARE) * WORK, SENTINEL, np.uint8), np.full(c.n + SPARE, STATUS_FILL, np.int32))


def finish_expect(c, states=None, keys=None, use_gate=True, psk="table"):
    """What wgcs_handshake_finish_host leaves for the case: (states, keys, work, verdict)."""
    w = world()
    states = (c.states if states is None else states).copy()
    fresh_keys, work, verdict = finish_outputs(c)
    keys = fresh_keys if keys is None else keys.copy()
    noise.finish_host(c.arena, c.pkts, c.types, c.gate if use_gate else None, w.responder, c.slots, states[:c.n_states],
                      w.psk if psk == "table" else None, keys[:c.n_keys], work, verdict, n_peers=N_PEERS)
    return states, keys, work, verdict
