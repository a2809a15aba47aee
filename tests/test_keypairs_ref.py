"""wgcs_keypairs_begin_responder_host, wgcs_keypairs_begin_initiator_host and
wgcs_keypairs_received_host (wireguard_amd/csrc/keypairs.cpp) against the
literal restatement of device/noise.go:664-754 and device/sessions.go in
tests/keypairs_ref.py (CPU only).

After every step -- one call -- the library's tables are compared, in all
their bytes, with what the restatement renders: the wgcs_keypairs rows, both
slot arrays, the AEAD key table and its key -> peer id column, and the step's
own output (the statuses, or d_rotated).  The named cases are those of
tests/keypairs_cases.py; the random sequences are drawn from the seeds fixed
below."""
import numpy as np
import pytest

import keypairs_cases as cases
from keypairs_cases import I, NOW, TABLES
from keypairs_ref import (CLAIM_NONE, ERR_INVALID_ARG, ERR_NO_HANDSHAKE, HS_BEGUN, HS_NONE, INITIATOR, NO_KEYPAIR,
                          PEER_NONE, SET)
from wireguard_amd import _lib, keypairs

SEEDS = range(200)


def check(c):
    w = c.world
    t, d = cases.tables_of(w), cases.device_of(w)
    outs = []
    for k, s in enumerate(c.steps):
        got = cases.run_host(w, t, s)
        want = cases.run_ref(w, d, s)
        assert got.tolist() == want.tolist(), (c.name, k, s.kind)
        for name, r in zip(TABLES, d.render(w.slots, w.peer_keys)):
            assert t[name].tobytes() == r.tobytes(), (c.name, k, s.kind, name)
        outs.append(got)
    return t, outs


@pytest.mark.parametrize("c", cases.named(), ids=lambda c: c.name)
def test_named_case(c):
    check(c)


def test_random_sequences():
    begun = rotated = refused = 0
    for seed in SEEDS:
        c = cases.random_case(seed)
        _, outs = check(c)
        for s, o in zip(c.steps, outs):
            if s.kind == "recv":
                rotated += int(o.sum())
            else:
                begun += int((o == HS_BEGUN).sum())
                refused += int((o == ERR_NO_HANDSHAKE).sum())
    assert begun > 2000 and rotated > 200 and refused > 50  # the sequences reach what they are for


def named(name):
    return next(c for c in cases.named() if c.name == name)


def test_what_the_named_cases_reach():
    """The cases are what their names say: spot checks of the states, independent of the restatement."""
    t, outs = check(named("responder_twice"))
    k = t["kp"][0]
    assert outs[0].tolist() == [HS_BEGUN] and outs[1].tolist() == [HS_BEGUN]
    assert tuple(k["next"]) == (2, 3, I[1], SET, NOW + 5) and k["current"]["flags"] == 0 and k["previous"]["flags"] == 0
    assert not t["keys"][0:2].view(np.uint8).any() and t["keys"][2:4].view(np.uint8).any()
    peer0 = int(named("responder_twice").world.table["peer"][0])
    assert t["key_peer"][:4].tolist() == [PEER_NONE, PEER_NONE, peer0, peer0]
    slot = {int(s["index"]): int(s["key"]) for s in t["slots"] if s["key"] != 0xFFFFFFFF}
    assert slot[I[0]] == NO_KEYPAIR and slot[I[1]] == 3

    t, outs = check(named("initiator_rekey_deletes_the_old_previous"))
    k = t["kp"][1]
    assert tuple(k["current"]) == (12, 13, I[8], SET | INITIATOR, NOW + 2) and tuple(k["previous"])[:3] == (10, 11, I[7])
    assert k["next"]["flags"] == 0 and not t["keys"][8:10].view(np.uint8).any() and t["keys"][10:14].view(np.uint8).any()
    peer = int(named("initiator_first").world.table["peer"][1])
    assert {int(s["index"]): int(s["key"]) for s in t["peer_keys"] if s["key"] != 0xFFFFFFFF}[peer] == 12

    t, outs = check(named("initiator_with_a_staged_next"))
    k = t["kp"][1]
    assert tuple(k["previous"])[:3] == (0, 1, I[0]) and tuple(k["current"])[:3] == (10, 11, I[7]) and k["next"]["flags"] == 0
    assert not t["keys"][8:10].view(np.uint8).any()

    t, outs = check(named("two_begins_of_one_peer_in_one_call"))
    assert outs[0].tolist() == [HS_BEGUN] * 3 and outs[1].tolist() == [HS_BEGUN] * 3
    assert tuple(t["kp"][3]["next"])[:3] == (4, 5, I[2]) and not t["keys"][0:2].view(np.uint8).any()
    assert tuple(t["kp"][1]["current"])[:3] == (10, 11, I[7]) and tuple(t["kp"][1]["previous"])[:3] == (8, 9, I[6])

    _, outs = check(named("a_gated_off_row"))
    assert outs[0].tolist() == [HS_NONE, HS_BEGUN, HS_NONE, HS_NONE] and outs[1].tolist() == [HS_NONE, HS_BEGUN, HS_NONE, HS_NONE]
    _, outs = check(named("each_invalid_arg_row"))
    assert outs[0].tolist() == [ERR_INVALID_ARG] * 6 + [HS_BEGUN] and outs[1].tolist() == [ERR_INVALID_ARG] * 3
    _, outs = check(named("an_unregistered_index"))
    assert outs[0].tolist() == [ERR_NO_HANDSHAKE, HS_BEGUN] and outs[1].tolist() == [ERR_NO_HANDSHAKE]
    _, outs = check(named("an_index_that_already_has_a_keypair"))
    assert outs[1].tolist() == [ERR_NO_HANDSHAKE] * 2 and outs[3].tolist() == [ERR_NO_HANDSHAKE] * 2
    _, outs = check(named("initiator_lookups"))
    assert outs[0].tolist() == [ERR_NO_HANDSHAKE] * 3 + [HS_BEGUN]

    t, outs = check(named("received_under_current_or_previous"))
    assert [o.tolist() for o in outs[2:]] == [[0, 0], [1], [0, 0, 0, 0]]
    assert tuple(t["kp"][1]["previous"])[:3] == (8, 9, I[6]) and tuple(t["kp"][1]["current"])[:3] == (0, 1, I[0])
    t, outs = check(named("three_rows_under_next"))
    assert [o.tolist() for o in outs[2:]] == [[0, 0, 1, 0, 0, 0], [0, 0]]
    _, outs = check(named("next_with_a_replay_or_auth_verdict"))
    assert [o.tolist() for o in outs[2:]] == [[0] * 5, [0, 1, 0]]
    _, outs = check(named("a_key_row_whose_peer_has_no_row"))
    assert outs[2].tolist() == [0] * 6
    assert (t["kp"]["claim"] == CLAIM_NONE).all()


def test_host_forms_refuse_bad_arguments():
    w = cases.named()[3].world
    t = cases.tables_of(w)
    before = {k: v.tobytes() for k, v in t.items()}
    L = _lib.load()
    s, r, q = cases.resp_step([(0, I[0], 0, 1)]), cases.recv_step([(1, 100)]), cases.init_step([I[6]])
    status, rot = np.full(1, 77, np.int32), np.full(1, 77, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    tail = lambda n_slots=len(t["slots"]), n_pk=len(t["peer_keys"]), keys=p(t["keys"]): (  # noqa: E731
        p(w.table), 4, p(t["kp"]), p(t["slots"]), n_slots, p(t["peer_keys"]), n_pk, keys, p(t["key_peer"]), 16)
    bad = _lib.ERR_INVALID_ARG
    assert L.wgcs_keypairs_begin_responder_host(None, p(s.gate), 1, NOW, *tail(), p(status)) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), None, 1, NOW, *tail(), p(status)) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), p(s.gate), 1, NOW, *tail(), None) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), p(s.gate), 1, NOW, *tail(), p(s.gate)) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), p(s.gate), 1, NOW, *tail(n_slots=24), p(status)) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), p(s.gate), 1, NOW, *tail(n_pk=3), p(status)) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), p(s.gate), 1, NOW, *tail(keys=None), p(status)) == bad
    assert L.wgcs_keypairs_begin_responder_host(p(s.resp), p(s.gate), (1 << 24) + 1, NOW, *tail(), p(status)) == bad
    hs = (p(w.hs_slots), len(w.hs_slots), p(w.states), len(w.states))
    assert L.wgcs_keypairs_begin_initiator_host(None, p(q.pkts), p(q.gate), 1, NOW, *hs, *tail(), p(status)) == bad
    assert L.wgcs_keypairs_begin_initiator_host(p(q.arena), p(q.pkts), p(q.gate), 1, NOW, p(w.hs_slots), 12, p(w.states),
                                                len(w.states), *tail(), p(status)) == bad
    assert L.wgcs_keypairs_begin_initiator_host(p(q.arena), p(q.pkts), p(q.gate), 1, NOW, None, len(w.hs_slots),
                                                p(w.states), len(w.states), *tail(), p(status)) == bad
    rest = (p(t["key_peer"]), 16, p(w.peer_rows), w.n_ids, p(t["kp"]), 4, p(t["slots"]), len(t["slots"]), p(t["peer_keys"]),
            len(t["peer_keys"]), p(t["keys"]))
    assert L.wgcs_keypairs_received_host(None, p(r.verdict), 1, *rest, p(rot)) == bad
    assert L.wgcs_keypairs_received_host(p(r.pkts), None, 1, *rest, p(rot)) == bad
    assert L.wgcs_keypairs_received_host(p(r.pkts), p(r.verdict), 1, *rest, None) == bad
    assert L.wgcs_keypairs_received_host(p(r.pkts), p(r.verdict), (1 << 28) + 1, *rest, p(rot)) == bad
    # n == 0 is a no-op whatever else is given
    assert L.wgcs_keypairs_begin_responder_host(None, None, 0, NOW, *tail(), None) == 0
    assert L.wgcs_keypairs_begin_initiator_host(None, None, None, 0, NOW, *hs, *tail(), None) == 0
    assert L.wgcs_keypairs_received_host(None, None, 0, *rest, None) == 0
    assert status[0] == 77 and rot[0] == 77 and {k: v.tobytes() for k, v in t.items()} == before


def test_layout_and_constants():
    assert keypairs.KEYPAIR_REF_DTYPE.itemsize == 24 and keypairs.KEYPAIRS_DTYPE.itemsize == 80
    assert keypairs.KEYPAIRS_DTYPE.fields["claim"][1] == 72 and keypairs.KEYPAIR_REF_DTYPE.fields["created_ns"][1] == 16
    assert keypairs.SESSION_NO_KEYPAIR == NO_KEYPAIR == 0xFFFFFFFE and keypairs.HS_BEGUN == HS_BEGUN == 8
    assert (keypairs.KEYPAIR_SET, keypairs.KEYPAIR_INITIATOR) == (SET, INITIATOR) == (1, 2)
