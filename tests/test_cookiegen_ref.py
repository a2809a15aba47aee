"""The host forms of the cookie generator (wgcs_cookie_gen_build, _initiated_host,
_responded_host, _consume_host, _age_host; wireguard_amd/csrc/cookiegen.cpp over
wgcs_cookiegen.h) against tests/cookiegen_ref.py, the literal restatement of
CookieGenerator and of receive.go:246-269 that takes message after message
(CPU only).

The batch forms decide the rows of one peer by a claim and a commit; the
restatement knows neither.  Every comparison here is therefore also the proof
that claim and commit leave what taking the rows in turn leaves.  Every table
and every verdict is compared whole."""
import struct

import numpy as np

import cookie_ref
import cookiegen_ref as ref
from cookiegen_cases import REFRESH, SECOND, UNKNOWN, World, arena_of, lookup_world, sent_arrays, sent_status
from wireguard_amd import _lib, cookiegen as cg, noise, rekey, router
from wireguard_amd._lib import (ERR_AUTH, ERR_INVALID_ARG, ERR_NO_HANDSHAKE, ERR_NO_PEER, HS_CONSUMED, HS_COOKIE_KEPT,
                                HS_INITIATED, HS_NONE, HS_PEER_COOKIE, HS_PEER_SEEN, HS_RESP_COOKIE, HS_RESPONDED,
                                HS_START_COOKIE)

NOW = 1000 * SECOND


def same(a, b):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sent(w: World, kind: str, peer_row, status=None):
    """One initiated / responded call on the host form and on the restatement; gen compared whole."""
    status = [sent_status(kind)] * len(peer_row) if status is None else status
    d, st, msgs, mac1s = sent_arrays(w.rng, kind, peer_row, status)
    (cg.initiated_host if kind == "init" else cg.responded_host)(d, st, msgs, w.gen)
    w.ref_sent(d["peer_row"], st, sent_status(kind), mac1s)
    same(w.gen, w.want_gen())
    return mac1s


def consume(w: World, rows, now: int, tail: int = 8):
    """One consume call on the host form and on the restatement; every output compared whole."""
    arena, pkts = arena_of([m for _, m in rows], tail)
    types = np.array([t for t, _ in rows], np.int32)
    before, arena0 = w.peers.copy(), arena.copy()
    work = np.full(cg.CONSUME_WORK_BYTES * len(rows), 0xEE, np.uint8)
    got = cg.consume_host(arena, pkts, types, now, w.hs_slots, w.states, w.slots, w.key_peer, w.peer_rows, w.gen, w.peers,
                          work=work)
    want = w.ref_consume(rows, now)
    assert got.tolist() == want.tolist()
    same(w.gen, w.want_gen())
    same(w.peers, w.want_peers(before))
    assert not work.any() and (arena == arena0).all()
    return got.tolist()


def age(w: World, now: int):
    before, gen0 = w.peers.copy(), w.gen.copy()
    cg.age_host(now, w.gen, w.peers)
    w.ref_age(now)
    same(w.peers, w.want_peers(before))
    same(w.gen, gen0)


def test_constants_symbols_and_layout():
    assert (HS_COOKIE_KEPT, cg.COOKIE_GEN_HAS_MAC1, cg.COOKIE_REFRESH_NS) == (ref.HS_COOKIE_KEPT, 1, ref.COOKIE_REFRESH_NS)
    assert (ERR_INVALID_ARG, ERR_AUTH, ERR_NO_PEER, ERR_NO_HANDSHAKE) == (ref.ERR_INVALID_ARG, ref.ERR_AUTH,
                                                                         ref.ERR_NO_PEER, ref.ERR_NO_HANDSHAKE)
    assert HS_COOKIE_KEPT not in (HS_NONE, 1, 2, HS_CONSUMED, HS_RESPONDED, HS_INITIATED, 6, 7, 8, 9)
    f = cg.COOKIE_GEN_DTYPE.fields
    assert [f[k][1] for k in ("cookie_key", "last_mac1", "cookie_set_at_ns", "flags", "claim")] == [0, 32, 48, 56, 60]
    L = _lib.load()
    for name in ("wgcs_cookie_gen_build", "wgcs_cookie_initiated_batch", "wgcs_cookie_responded_batch",
                 "wgcs_cookie_consume_batch", "wgcs_cookie_age_batch", "wgcs_cookie_initiated_host",
                 "wgcs_cookie_responded_host", "wgcs_cookie_consume_host", "wgcs_cookie_age_host"):
        assert name in _lib.declared_symbols() and hasattr(L, name)


def test_gen_build_is_init():
    w = World(np.random.default_rng(1), n_peers=4)
    same(w.gen, w.want_gen())
    for r, pk in enumerate(w.pubs):
        assert w.gen["cookie_key"][r].tobytes() == cookie_ref.hash256(b"cookie--" + pk)
    assert len(cg.gen_build(np.zeros(0, noise.PEER_KEY_DTYPE))) == 0


# ---------------------------------------------------------------- lookup
def test_reply_found_through_the_handshake_table_and_through_the_keypair_table():
    w = lookup_world(np.random.default_rng(2))
    sent(w, "init", [0, 3, 4, 2, 1])
    got = consume(w, [(3, w.reply(0x1001, 0)), (3, w.reply(0x3001, 2)), (3, w.reply(0x1002, 3)),
                      (3, w.reply(0x1003, 4)), (3, w.reply(0x3002, 1))], NOW)
    assert got == [HS_COOKIE_KEPT] * 5
    assert (w.peers["flags"] & HS_PEER_COOKIE).all() and (w.gen["cookie_set_at_ns"] == NOW).all()
    assert (w.peers["flags"] & HS_PEER_SEEN).tolist() == [1, 0, 1, 0, 1]  # the other bit stays


def test_state_row_reused_under_another_index():
    w = lookup_world(np.random.default_rng(3))
    sent(w, "init", [1])
    assert consume(w, [(3, w.reply(0x2001, 1)), (3, w.reply(0x2002, 1))], NOW) == [ERR_NO_PEER, HS_COOKIE_KEPT]


def test_no_keypair_slot_unknown_receiver_and_rows_past_the_tables():
    w = lookup_world(np.random.default_rng(4))
    sent(w, "init", [0, 1, 2, 3, 4])
    rows = [(3, w.reply(i, 0)) for i in (0x4001, UNKNOWN, 0x1004, 0x3003, 0x3004)]
    assert consume(w, rows, NOW) == [ERR_NO_PEER] * 5
    assert not (w.peers["flags"] & HS_PEER_COOKIE).any()


def test_empty_tables():
    w = World(np.random.default_rng(5)).finish()
    sent(w, "init", [0])
    assert consume(w, [(3, w.reply(1, 0)), (4, bytes(64))], NOW) == [ERR_NO_PEER, HS_NONE]
    w.hs_slots = w.slots = np.zeros(0, router.SESSION_SLOT_DTYPE)  # slot counts of 0
    w.states, w.key_peer = w.states[:0], w.key_peer[:0]
    assert consume(w, [(3, w.reply(0, 0)), (4, bytes(64))], NOW) == [ERR_NO_PEER, HS_NONE]
    assert consume(w, [], NOW) == []


# ---------------------------------------------------------------- messages
def test_length_and_type_word():
    w = lookup_world(np.random.default_rng(6))
    sent(w, "init", [0])
    good = w.reply(0x1001, 0)
    wrong_word = struct.pack("<I", 1) + good[4:]
    rows = [(3, good[:63]), (3, good + b"\0"), (1, good), (3, wrong_word), (2, good), (4, good), (0, good), (-1, good),
            (3, b"")]
    assert consume(w, rows, NOW) == [ERR_INVALID_ARG, ERR_INVALID_ARG, HS_NONE, ERR_INVALID_ARG, HS_NONE, HS_NONE,
                                     HS_NONE, HS_NONE, ERR_INVALID_ARG]
    assert consume(w, [(3, good)], NOW, tail=0) == [HS_COOKIE_KEPT]  # the message ends with the arena


def test_no_last_mac1():
    w = lookup_world(np.random.default_rng(7))
    assert consume(w, [(3, w.reply(0x1001, 0)), (3, w.reply(0x3001, 2))], NOW) == [ERR_NO_HANDSHAKE] * 2


def test_reply_for_the_previous_message_and_a_flipped_tag_bit():
    w = lookup_world(np.random.default_rng(8))
    first = sent(w, "init", [0])[0]
    sent(w, "init", [0])
    stale = w.reply(0x1001, 0, mac1=first)  # sealed over the MAC1 of the peer's previous message
    good = w.reply(0x1001, 0)
    flipped = good[:63] + bytes([good[63] ^ 0x80])
    wrong_key = w.reply(0x1001, 1, mac1=w.ref[0].last_mac1)  # another peer's cookie key
    assert consume(w, [(3, stale), (3, flipped), (3, wrong_key)], NOW) == [ERR_AUTH] * 3
    assert not (w.peers["flags"] & HS_PEER_COOKIE).any()
    assert consume(w, [(3, stale), (3, good), (3, flipped)], NOW + 5) == [ERR_AUTH, HS_COOKIE_KEPT, ERR_AUTH]


# ---------------------------------------------------------------- ordering
def test_three_valid_replies_for_one_peer_the_highest_row_stands():
    w = lookup_world(np.random.default_rng(9))
    sent(w, "init", [3, 0])
    cookies = [bytes([c]) * 16 for c in (1, 2, 3)]
    rows = [(3, w.reply(0x1002, 3, cookies[0])), (3, w.reply(0x1001, 0)), (3, w.reply(0x1002, 3, cookies[1])),
            (4, bytes(64)), (3, w.reply(0x1002, 3, cookies[2])), (3, w.reply(UNKNOWN, 3))]
    assert consume(w, rows, NOW) == [HS_COOKIE_KEPT, HS_COOKIE_KEPT, HS_COOKIE_KEPT, HS_NONE, HS_COOKIE_KEPT, ERR_NO_PEER]
    assert w.peers["cookie"][3].tobytes() == cookies[2] and not w.gen["claim"].any()


def test_several_descriptors_for_one_peer_the_highest_stands():
    w = World(np.random.default_rng(10)).finish()
    for kind in ("init", "resp"):
        ok, other = sent_status(kind), HS_INITIATED + HS_RESPONDED - sent_status(kind)
        mac1s = sent(w, kind, [2, 0, 2, 7, 2, 4, 2], [ok, ok, ok, ok, ok, -1, other])
        assert w.gen["last_mac1"][2].tobytes() == mac1s[4]  # rows 5 and 6 take no part, row 3 is past the table
        assert w.gen["flags"].tolist() == [1, 0, 1, 0, 0] and not w.gen["claim"].any()
    sent(w, "init", [])


def test_a_response_and_an_initiation_to_one_peer_the_later_call_stands():
    w = lookup_world(np.random.default_rng(11))
    r = sent(w, "resp", [2])[0]
    i = sent(w, "init", [2])[0]
    assert w.gen["last_mac1"][2].tobytes() == i
    assert consume(w, [(3, w.reply(0x3001, 2, mac1=r)), (3, w.reply(0x3001, 2, mac1=i))], NOW) == [ERR_AUTH, HS_COOKIE_KEPT]
    r = sent(w, "resp", [2])[0]
    assert w.gen["last_mac1"][2].tobytes() == r
    assert consume(w, [(3, w.reply(0x3001, 2, mac1=i)), (3, w.reply(0x3001, 2, mac1=r))], NOW) == [ERR_AUTH, HS_COOKIE_KEPT]


# ---------------------------------------------------------------- ageing
def test_ageing():
    w = lookup_world(np.random.default_rng(12))
    sent(w, "init", [0, 3])
    consume(w, [(3, w.reply(0x1001, 0)), (3, w.reply(0x1002, 3))], NOW)
    age(w, NOW + REFRESH)  # exactly 120 s: kept
    assert (w.peers["flags"] & HS_PEER_COOKIE).tolist() == [2, 0, 0, 2, 0]
    age(w, NOW - 500 * SECOND)  # a clock that went back
    age(w, -(2**62))
    assert (w.peers["flags"] & HS_PEER_COOKIE).tolist() == [2, 0, 0, 2, 0]
    consume(w, [(3, w.reply(0x1002, 3))], NOW + 7)  # row 3 is refreshed, row 0 is not
    age(w, NOW + REFRESH + 1)  # 120 s + 1 ns: cleared, the other bit preserved
    assert w.peers["flags"].tolist() == [HS_PEER_SEEN, 0, HS_PEER_SEEN, HS_PEER_COOKIE, HS_PEER_SEEN]
    assert w.peers["cookie"][0].any()  # the bytes stay, as in the reference
    age(w, NOW + 10 * REFRESH)  # the bit not set: rows 0..2 and 4 untouched, row 3 cleared
    assert not (w.peers["flags"] & HS_PEER_COOKIE).any()
    cg.age_host(NOW, np.zeros(0, cg.COOKIE_GEN_DTYPE), np.zeros(0, noise.HS_PEER_DTYPE))


# ---------------------------------------------------------------- argument checks of the host forms
def test_host_forms_refuse_bad_arguments():
    L = _lib.load()
    w = lookup_world(np.random.default_rng(13))
    d, st, msgs, _ = sent_arrays(w.rng, "init", [0], [HS_INITIATED])
    g, p = w.gen.ctypes.data, w.peers.ctypes.data
    assert L.wgcs_cookie_initiated_host(None, st.ctypes.data, msgs.ctypes.data, 1, g, 5) == ERR_INVALID_ARG
    assert L.wgcs_cookie_initiated_host(d.ctypes.data, st.ctypes.data, msgs.ctypes.data, 1, None, 5) == ERR_INVALID_ARG
    assert L.wgcs_cookie_initiated_host(d.ctypes.data, st.ctypes.data, msgs.ctypes.data, 1, g + 2, 4) == ERR_INVALID_ARG
    assert L.wgcs_cookie_responded_host(d.ctypes.data, st.ctypes.data, msgs.ctypes.data, (1 << 28) + 1, g, 5) == ERR_INVALID_ARG
    assert L.wgcs_cookie_initiated_host(None, None, None, 0, None, 0) == 0
    assert L.wgcs_cookie_age_host(0, None, p, 5) == ERR_INVALID_ARG
    assert L.wgcs_cookie_age_host(0, g, p + 1, 4) == ERR_INVALID_ARG
    a, v, wk = np.zeros(64, np.uint8), np.zeros(1, np.int32), np.zeros(16, np.uint8)
    pk, ty = np.zeros(1, cg.AEAD_PKT_DTYPE), np.zeros(1, np.int32)
    args = [a.ctypes.data, pk.ctypes.data, ty.ctypes.data, 1, 0, w.hs_slots.ctypes.data, len(w.hs_slots),
            w.states.ctypes.data, len(w.states), w.slots.ctypes.data, len(w.slots), w.key_peer.ctypes.data,
            len(w.key_peer), w.peer_rows.ctypes.data, len(w.peer_rows), g, p, 5, wk.ctypes.data, v.ctypes.data]
    assert L.wgcs_cookie_consume_host(*args) == 0
    for i, bad in ((0, None), (6, 3), (10, 12), (15, None), (18, None), (19, None), (3, (1 << 28) + 1)):
        assert L.wgcs_cookie_consume_host(*(args[:i] + [bad] + args[i + 1:])) == ERR_INVALID_ARG, i
    same(w.gen, w.want_gen())


# ---------------------------------------------------------------- random sequences
def _accept(w: World, rng, now: int, seq: list):
    """accept_host over an initiation per chosen peer: the cookie it puts into a descriptor is the restatement's."""
    rows = [r for r in range(w.n_peers) if rng.random() < 0.6]
    init = np.zeros(len(rows), noise.HS_INIT_DTYPE)
    init["peer"] = [w.ids[r] for r in rows]
    init["sender"] = rng.integers(1, 2**32, len(rows), dtype=np.uint64).astype(np.uint32)
    seq[0] += 1
    init["timestamp"][:, 4:] = np.frombuffer(struct.pack(">Q", seq[0]), np.uint8)  # strictly later than the last
    tickets = np.zeros(len(rows), noise.HS_TICKET_DTYPE)
    resp, count = np.zeros(len(rows), noise.HS_RESP_DTYPE), np.zeros(1, np.uint32)
    verdict = np.zeros(len(rows), np.int32)
    noise.accept_host(init, np.full(len(rows), HS_CONSUMED, np.int32), now, w.table, w.peer_rows, w.peers, tickets, resp,
                      count, verdict)
    return [_check_descriptor(w, resp[j], HS_RESP_COOKIE, now) for j in range(int(count[0]))]


def _start(w: World, rng, now: int):
    """rekey.start_host for the peers that want a handshake: the same check on its descriptors."""
    rk = rekey.rekey_table(w.n_peers, now)
    rk["want"] = [rekey.REKEY_WANT_NO_KEYPAIR if rng.random() < 0.6 else 0 for _ in range(w.n_peers)]
    tickets = np.zeros(w.n_peers, noise.HS_START_DTYPE)
    start, start_peer = np.zeros(w.n_peers, noise.HS_START_DTYPE), np.zeros(w.n_peers, np.uint32)
    count, status, reasons = np.zeros(1, np.uint32), np.zeros(w.n_peers, np.int32), np.zeros(w.n_peers, np.uint32)
    rekey.start_host(now, rk, w.peers, tickets, start, start_peer, count, status, reasons)
    assert start["peer_row"][:int(count[0])].tolist() == start_peer[:int(count[0])].tolist()
    return [_check_descriptor(w, start[k], HS_START_COOKIE, now) for k in range(int(count[0]))]


def _check_descriptor(w: World, d, bit: int, now: int):
    want = w.ref[int(d["peer_row"])].cookie_for(now)  # what AddMACs would use at `now`
    assert bool(int(d["flags"]) & bit) == (want is not None)
    assert d["cookie"].tobytes() == (want or bytes(16))
    return want is not None


def test_random_sequences():
    seen_verdicts, seen_paths, descriptors, with_cookie = set(), set(), 0, 0
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        w = lookup_world(rng)
        hs = {i: r for i, r in w.index_table.items() if i < 0x3000}
        kp = {i: r for i, r in w.index_table.items() if i >= 0x3000}
        now, seq = NOW + seed, [seed]
        for _ in range(int(rng.integers(6, 13))):
            # the clock never goes back here
            now += int(rng.choice([0, 1, SECOND, 50 * SECOND, REFRESH, REFRESH + 1], p=[.2, .2, .25, .2, .075, .075]))
            what = rng.choice(["init", "resp", "consume", "consume", "age+accept", "age+start"])
            if what in ("init", "resp"):
                n = int(rng.integers(0, 7))
                sent(w, what, rng.integers(0, w.n_peers + 1, n), rng.choice([sent_status(what), HS_NONE, -1], n, p=[.8, .1, .1]))
            elif what == "consume":
                rows = []
                for _ in range(int(rng.integers(0, 5))):
                    kind = rng.choice(["hs", "kp", "nopeer", "badlen", "other", "stale"], p=[.3, .3, .1, .1, .1, .1])
                    if kind in ("hs", "kp"):
                        index, row = list((hs if kind == "hs" else kp).items())[int(rng.integers(0, 3 if kind == "hs" else 2))]
                        rows.append((3, w.reply(index, row, fast=True)))
                        seen_paths.add(kind)
                    elif kind == "nopeer":
                        rows.append((3, w.reply(int(rng.choice([0x4001, UNKNOWN, 0x2001])), 0, fast=True)))
                    elif kind == "badlen":
                        rows.append((3, rng.bytes(int(rng.choice([0, 63, 65, 148])))))
                    elif kind == "other":
                        rows.append((int(rng.choice([0, 1, 2, 4])), rng.bytes(64)))
                    else:
                        row = int(rng.integers(0, 3))
                        rows.append((3, w.reply(0x1001 + row if row < 2 else 0x1003, [0, 3, 4][row], mac1=rng.bytes(16), fast=True)))
                seen_verdicts.update(consume(w, rows, now))
            else:
                age(w, now)
                before = w.peers.copy()
                carried = _accept(w, rng, now, seq) if what == "age+accept" else _start(w, rng, now)
                descriptors, with_cookie = descriptors + len(carried), with_cookie + sum(carried)
                same(w.peers["cookie"], before["cookie"])
                assert ((w.peers["flags"] ^ before["flags"]) & HS_PEER_COOKIE == 0).all()
    # a condition on the generator: every verdict class and both lookup paths occur
    assert seen_verdicts == {HS_NONE, HS_COOKIE_KEPT, ERR_INVALID_ARG, ERR_NO_PEER, ERR_NO_HANDSHAKE, ERR_AUTH}
    assert set(map(str, seen_paths)) == {"hs", "kp"} and descriptors > 100 and with_cookie > 20
