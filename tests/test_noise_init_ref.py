"""The host forms of the handshake initiator (wgcs_handshake_initiate_host,
wgcs_handshake_finish_host of noise.cpp) through wireguard_amd.noise against
the restatements tests/noise_ref.py, tests/noise_resp_ref.py and
tests/cookie_ref.py (CPU only).

The batches are those of tests/noise_init_cases.py, which the GPU tests use
too: every row of both status tables, with and without a preshared key and a
cookie.  Every output is filled with a sentinel and longer than its batch."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cookie_ref
import noise_init_cases as cases
import noise_ref
import noise_resp_ref
from noise_init_cases import (ERR_NO_HANDSHAKE, HS_FINISHED, HS_INITIATED, N_PEERS, PITCH, SENTINEL, SPARE, STATUS_FILL, WORK,
                              world)
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, HS_NONE
from wireguard_amd import _lib, noise
from wireguard_amd.transport import AEAD_KEY_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILL128 = bytes([SENTINEL]) * 128


def state_bytes(state, local, peer, remote, send, recv, h=bytes(32), chain=bytes(32), eph=bytes(32)) -> bytes:
    """One wgcs_hs_state row outside a finish call."""
    return struct.pack("<8I", state, local, peer, remote, send, recv, 0xFFFFFFFF, 0) + h + chain + eph


def test_initial_hash_and_chain_key_words_of_the_kernel():
    """noise_initial holds the two constants as literals: an initiation is built on them with no table to read."""
    w = world()
    d, n_states, n_keys = cases.start_batch(1)
    states, _, status = cases.initiate_expect(1)
    assert status[0] == HS_INITIATED
    p = int(d["peer_row"][0])
    _, h, chain = noise_ref.create_initiation(w.private, w.table["public_key"][p].tobytes(),
                                              d["ephemeral_private"][0].tobytes(), d["timestamp"][0].tobytes(),
                                              int(d["local_index"][0]))
    assert states["hash"][0].tobytes() == h and states["chain_key"][0].tobytes() == chain


@pytest.mark.parametrize("n", [1, 40])
def test_initiate_host_matches_the_restatement(n):
    w = world()
    d, n_states, n_keys = cases.start_batch(n)
    states, msgs, status = cases.initiate_expect(n)
    touched = set()
    for j in range(n):
        s, p, a, b = (int(d[f][j]) for f in ("state_row", "peer_row", "send_key", "recv_key"))
        row = msgs[PITCH * j:PITCH * (j + 1)].tobytes()
        if s >= n_states or p >= N_PEERS or a >= n_keys or b >= n_keys or a == b:
            assert status[j] == ERR_INVALID_ARG and row == bytes([SENTINEL]) * PITCH, j
            continue
        remote = w.table["public_key"][p].tobytes()
        eph, ts, index = d["ephemeral_private"][j].tobytes(), d["timestamp"][j].tobytes(), int(d["local_index"][j])
        want = noise_ref.create_initiation(w.private, remote, eph, ts, index)
        if want is None:
            assert p == w.low_row and status[j] == ERR_LOW_ORDER and row == bytes(PITCH), j
            continue
        msg, h, chain = want
        cookie = d["cookie"][j].tobytes() if d["flags"][j] & 1 else None
        msg, mac1 = cookie_ref.add_macs(noise_resp_ref.mac1_key(remote), msg, cookie)
        assert status[j] == HS_INITIATED and row == msg + bytes(12), j
        assert row[116:132] == mac1 and any(row[132:148]) == (cookie is not None)
        assert states[s].tobytes() == state_bytes(1, index, p, 0, a, b, h, chain, eph), j
        # the host function of one message, which runs the third ladder, gives the same bytes
        assert noise.create_initiation(w.private, remote, eph, ts, index) == (want[0], h, chain)
        touched.add(s)
    for s in range(n_states + SPARE):
        assert s in touched or states[s].tobytes() == FILL128, f"state row {s} was written"
    assert (msgs[PITCH * n:] == SENTINEL).all() and (status[n:] == STATUS_FILL).all()
    if n > 1:
        seen = set(status[:n].tolist())
        assert seen == {HS_INITIATED, ERR_INVALID_ARG, ERR_LOW_ORDER}
        ok = np.flatnonzero(status[:n] == HS_INITIATED)
        assert {int(d["flags"][j]) & 1 for j in ok} == {0, 1} and any(int(d["flags"][j]) > 1 for j in ok)


@pytest.mark.parametrize("n", [1, 96])
def test_finish_host_matches_the_restatement(n):
    w = world()
    c = cases.finish_case(n)
    states, keys, work, verdict = cases.finish_expect(c)
    assert verdict[:n].tolist() == c.want.tolist(), [(q, c.kinds[q], int(verdict[q])) for q in range(n)
                                                     if verdict[q] != c.want[q]][:5]
    assert (verdict[n:] == STATUS_FILL).all()
    assert not work[:WORK * n].any() and (work[WORK * n:] == SENTINEL).all()
    want_states = c.states.copy()
    want_keys = np.full((c.n_keys + SPARE) * 48, SENTINEL, np.uint8).view(AEAD_KEY_DTYPE)
    with_psk = set()
    for q in np.flatnonzero(verdict[:n] == HS_FINISHED):
        hs = c.hs_of_row[q]
        st = c.states[hs]
        p = int(st["peer_row"])
        psk = w.psk[p].tobytes()
        with_psk.add(any(psk))
        msg = c.arena[int(c.pkts["off"][q]):int(c.pkts["off"][q]) + 92].tobytes()
        rc, sender, send, recv, _, _ = noise_resp_ref.consume_response(
            w.private, st["hash"].tobytes(), st["chain_key"].tobytes(), st["ephemeral_private"].tobytes(),
            int(st["local_index"]), msg, psk)
        assert (rc, sender) == (0, int(c.sender[q])), q
        want_keys[int(st["send_key"])] = np.frombuffer(noise_resp_ref.aead_key_bytes(send, sender), AEAD_KEY_DTYPE)[0]
        want_keys[int(st["recv_key"])] = np.frombuffer(noise_resp_ref.aead_key_bytes(recv, 0), AEAD_KEY_DTYPE)[0]
        want_states[hs] = np.frombuffer(state_bytes(0, int(st["local_index"]), p, sender, int(st["send_key"]),
                                                    int(st["recv_key"])), noise.HS_STATE_DTYPE)[0]
    assert keys.tobytes() == want_keys.tobytes()
    assert states.tobytes() == want_states.tobytes()
    if n > 1:
        assert with_psk == {False, True}
        assert set(c.kinds) == set(cases.KIND_VERDICT), "every row of the table"
        low = [c.arena[int(c.pkts["off"][q]) + 12:int(c.pkts["off"][q]) + 44].tobytes()
               for q in range(n) if c.kinds[q] == "low_order"]
        assert set(low) == set(noise_ref.LOW_ORDER_POINTS)
        q = c.kinds.index("forged")
        assert verdict[q:q + 3].tolist() == [ERR_AUTH, HS_FINISHED, ERR_NO_HANDSHAKE]
    # the restatement says the same of the rows that reach the cryptography
    for q in range(n):
        if c.kinds[q] in ("low_order", "tag", "forged"):
            st = c.states[c.hs_of_row[q]]
            msg = c.arena[int(c.pkts["off"][q]):int(c.pkts["off"][q]) + 92].tobytes()
            got = noise_resp_ref.consume_response(w.private, st["hash"].tobytes(), st["chain_key"].tobytes(),
                                                  st["ephemeral_private"].tobytes(), int(st["local_index"]), msg,
                                                  w.psk[int(st["peer_row"])].tobytes())
            assert got[0] == verdict[q], (q, c.kinds[q])


def test_finish_host_again_without_gate_and_without_psk():
    w = world()
    c = cases.finish_case(96)
    states, keys, work, verdict = cases.finish_expect(c)
    # again on the finished states: what was finished finds a zeroed handshake, nothing moves
    states2, keys2, work2, verdict2 = cases.finish_expect(c, states=states, keys=keys)
    was = verdict[:c.n] == HS_FINISHED
    assert (verdict2[:c.n][was] == ERR_NO_HANDSHAKE).all()
    assert states2.tobytes() == states.tobytes() and keys2.tobytes() == keys.tobytes() and not work2[:WORK * c.n].any()
    forged = np.array([k == "forged" for k in c.kinds])  # its handshake is gone now: the state check comes first
    assert (verdict2[:c.n][forged] == ERR_NO_HANDSHAKE).all()
    assert np.array_equal(verdict2[:c.n][~was & ~forged], verdict[:c.n][~was & ~forged])
    # a NULL gate takes every row of type 2: the gated rows are authentic responses
    no_gate = cases.finish_expect(c, use_gate=False)[3]
    gated = [q for q in range(c.n) if c.kinds[q] == "gated"]
    assert gated and (verdict[gated] == HS_NONE).all() and (no_gate[gated] == HS_FINISHED).all()
    # a NULL psk table is the zero key for every peer: only the peers without one authenticate
    no_psk = cases.finish_expect(c, psk=None)[3]
    for q in np.flatnonzero(was):
        has = w.psk[int(c.states["peer_row"][c.hs_of_row[q]])].any()
        assert no_psk[q] == (ERR_AUTH if has else HS_FINISHED), q


def test_arguments_of_the_host_forms():
    w = world()
    L = _lib.load()
    c = cases.finish_case(1)
    d, n_states, n_keys = cases.start_batch(1)
    states, msgs, status = cases.initiate_outputs(1, n_states)
    pub = w.public
    good = [d.ctypes.data, 1, pub, w.table.ctypes.data, N_PEERS, n_keys, states.ctypes.data, n_states, msgs.ctypes.data,
            status.ctypes.data]
    assert L.wgcs_handshake_initiate_host(*good) == 0 and status[0] == HS_INITIATED
    for k in (0, 2, 3, 6, 8, 9):
        bad = list(good)
        bad[k] = None
        assert L.wgcs_handshake_initiate_host(*bad) == ERR_INVALID_ARG, k
    assert L.wgcs_handshake_initiate_host(*(good[:1] + [(1 << 28) + 1] + good[2:])) == ERR_INVALID_ARG
    assert L.wgcs_handshake_initiate_host(None, 0, None, None, 0, 0, None, 0, None, None) == 0  # n == 0: a no-op
    # with empty tables every descriptor is out of range, and nothing is read
    status[:] = STATUS_FILL
    assert L.wgcs_handshake_initiate_host(d.ctypes.data, 1, pub, None, 0, n_keys, None, 0, msgs.ctypes.data,
                                          status.ctypes.data) == 0
    assert status[0] == ERR_INVALID_ARG
    keys, work, verdict = cases.finish_outputs(c)
    st = c.states.copy()
    good = [c.arena.ctypes.data, c.pkts.ctypes.data, c.types.ctypes.data, c.gate.ctypes.data, 1, w.responder.ctypes.data,
            c.slots.ctypes.data, len(c.slots), st.ctypes.data, c.n_states, w.psk.ctypes.data, N_PEERS, keys.ctypes.data,
            c.n_keys, work.ctypes.data, verdict.ctypes.data]
    for k in (0, 1, 2, 5, 6, 8, 12, 14, 15):
        bad = list(good)
        bad[k] = None
        assert L.wgcs_handshake_finish_host(*bad) == ERR_INVALID_ARG, k
    for change in ({4: (1 << 28) + 1}, {7: 3}, {3: verdict.ctypes.data}):
        bad = list(good)
        for k, v in change.items():
            bad[k] = v
        assert L.wgcs_handshake_finish_host(*bad) == ERR_INVALID_ARG, change
    assert (verdict == STATUS_FILL).all() and st.tobytes() == c.states.tobytes()
    assert L.wgcs_handshake_finish_host(*good) == 0 and verdict[0] == HS_FINISHED
    # no slots at all: no handshake is found, and the table is not read
    verdict[:] = STATUS_FILL
    args = list(good)
    args[6], args[7] = None, 0
    assert L.wgcs_handshake_finish_host(*args) == 0 and verdict[0] == ERR_NO_HANDSHAKE
    with pytest.raises(ValueError):
        noise.initiate_host(d, bytes(31), w.table, states[:n_states], msgs, status, n_keys)
    with pytest.raises(TypeError):
        noise.initiate_host(d, pub, w.table, states[:n_states], msgs.tolist(), status, n_keys)


def test_constants_and_layouts(tmp_path):
    assert (_lib.HS_INITIATED, _lib.HS_FINISHED, _lib.ERR_NO_HANDSHAKE) == (HS_INITIATED, HS_FINISHED, ERR_NO_HANDSHAKE)
    assert (noise.HS_INITIATED, noise.HS_FINISHED, noise.ERR_NO_HANDSHAKE, noise.HS_START_COOKIE) == (5, 6, -24, 1)
    assert (noise.HS_STATE_ZEROED, noise.HS_STATE_INITIATED) == (0, 1)
    L = _lib.load()
    assert L.wgcs_strerror(-24) not in (None, b"", b"unknown status")
    for name in ("wgcs_handshake_initiate_batch", "wgcs_handshake_finish_batch", "wgcs_handshake_initiate_host",
                 "wgcs_handshake_finish_host"):
        assert name in _lib.declared_symbols() and hasattr(L, name)
    state = {"state": 0, "local_index": 4, "peer_row": 8, "remote_index": 12, "send_key": 16, "recv_key": 20, "claim": 24,
             "pad": 28, "hash": 32, "chain_key": 64, "ephemeral_private": 96}
    start = {"state_row": 0, "peer_row": 4, "local_index": 8, "send_key": 12, "recv_key": 16, "flags": 20, "timestamp": 24,
             "pad0": 36, "ephemeral_private": 40, "cookie": 72, "pad1": 88}
    assert {k: noise.HS_STATE_DTYPE.fields[k][1] for k in state} == state and noise.HS_STATE_DTYPE.itemsize == 128
    assert {k: noise.HS_START_DTYPE.fields[k][1] for k in start} == start and noise.HS_START_DTYPE.itemsize == 96
    checks = " && ".join([f"offsetof(wgcs_hs_state, {k}) == {v}" for k, v in state.items()] +
                         [f"offsetof(wgcs_hs_start, {k}) == {v}" for k, v in start.items()])
    src = tmp_path / "t.c"
    src.write_text('#include "wgcsum.h"\n#include <stddef.h>\n'
                   f'_Static_assert({checks}, "offsets");\n'
                   '_Static_assert(sizeof(wgcs_hs_state) == 128 && _Alignof(wgcs_hs_state) == 4 && '
                   'sizeof(wgcs_hs_start) == 96 && _Alignof(wgcs_hs_start) == 4, "sizes");\n'
                   '_Static_assert(WGCS_HS_INITIATED == 5 && WGCS_HS_FINISHED == 6 && WGCS_ERR_NO_HANDSHAKE == -24 && '
                   'WGCS_HS_STATE_ZEROED == 0 && WGCS_HS_STATE_INITIATED == 1 && WGCS_HS_START_COOKIE == 1, "codes");\n'
                   '_Static_assert(sizeof(wgcs_hs_init) == 128 && sizeof(wgcs_hs_resp) == 80 && sizeof(wgcs_aead_key) == 48, '
                   '"neighbours keep their layout");\n'
                   "int main(void) { return 0; }\n")
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)
