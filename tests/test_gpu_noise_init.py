"""The device-resident handshake initiator on the GPU
(wgcs_handshake_initiate_batch and wgcs_handshake_finish_batch: hs_initiate_kernel,
hs_finish_kernel and hs_finish_commit_kernel of noise_init_kernels.hip).

Message rows, the whole state table, the whole key table, the scratch and the
status arrays are compared byte for byte with the host forms
wgcs_handshake_initiate_host / wgcs_handshake_finish_host, which
tests/test_noise_init_host.py and tests/test_noise_init_ref.py pin to the
restatements; every output is filled with a sentinel first and is longer than
the batch and its table, so the rows that must stay untouched are compared too.
The last test runs a whole handshake between two devices' worth of tables on
one stream and passes transport packets both ways under the keys it left."""
import numpy as np
import pytest
import torch

import cookie_ref
import noise_init_cases as cases
import noise_ref
import noise_resp_ref
from noise_init_cases import ERR_NO_HANDSHAKE, HS_FINISHED, HS_INITIATED, N_PEERS, PITCH, SENTINEL, STATUS_FILL, WORK, world
from noise_ref import ERR_AUTH, ERR_INVALID_ARG, ERR_LOW_ORDER, HS_CONSUMED, HS_NONE, HS_PASS
from test_gpu_cookie import up
from wireguard_amd import _lib, cookie, noise, router, transport
from wireguard_amd.noise import HS_RESP_DTYPE, HS_START_DTYPE, HS_STATE_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [1, 67, 300]  # one lane; a partial wave past a full one; a batch that crosses the 256-lane workgroup


def differ(got, want, row_bytes, what):
    bad = np.flatnonzero(np.asarray(got).view(np.uint8).reshape(-1) != np.asarray(want).view(np.uint8).reshape(-1))
    assert len(bad) == 0, f"{what} differs, first in row {bad[0] // row_bytes} at byte {bad[0] % row_bytes}"


def run_initiate(dev, n, plain=False, stream=None):
    """The launch over start_batch(n, plain): (d_states, states, msgs, status) with the outputs' fill and spare rows."""
    w = world()
    d, n_states, n_keys = cases.start_batch(n, plain)
    states, msgs, status = cases.initiate_outputs(n, n_states)
    d_start, d_pub, d_table = up(d), up(np.frombuffer(w.public, np.uint8)), up(w.table)
    d_states, d_msgs, d_status = up(states), up(msgs), torch.from_numpy(status.copy()).cuda()
    noise.initiate_batch(dev, d_start, d_pub, d_table, d_states, d_msgs, d_status, n_keys, stream=stream, n=n,
                         n_peers=N_PEERS, n_states=n_states)
    torch.cuda.synchronize()
    for t, a, what in ((d_start, d, "d_start"), (d_table, w.table, "d_table")):
        assert t.cpu().numpy().tobytes() == a.tobytes(), f"the initiate step wrote {what}"
    return d_states, d_states.cpu().numpy(), d_msgs.cpu().numpy(), d_status.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_initiate_batch_matches_the_host_form(dev, n):
    d, n_states, n_keys = cases.start_batch(n)
    want_states, want_msgs, want_status = cases.initiate_expect(n)
    _, states, msgs, status = run_initiate(dev, n)
    bad = np.flatnonzero(status != want_status)
    assert len(bad) == 0, f"{len(bad)} statuses differ, first at row {bad[0]}: got {status[bad[0]]}, want {want_status[bad[0]]}"
    differ(msgs, want_msgs, PITCH, "d_msgs")
    differ(states, want_states, 128, "d_states")
    st = states.view(HS_STATE_DTYPE)
    for j in range(n):  # what the table of include/wgcsum.h promises, row by row
        row = msgs[PITCH * j:PITCH * (j + 1)]
        if status[j] == HS_INITIATED:
            s = int(d["state_row"][j])
            assert not row[148:].any() and row[116:132].any() and row[132:148].any() == bool(d["flags"][j] & 1)
            assert (st["state"][s], st["local_index"][s], st["claim"][s]) == (1, d["local_index"][j], 0xFFFFFFFF)
        else:
            assert (row == (0 if status[j] == ERR_LOW_ORDER else SENTINEL)).all()
            if int(d["state_row"][j]) < n_states:
                assert st[int(d["state_row"][j])].tobytes() == bytes([SENTINEL]) * 128, "a failing row wrote its state"
    assert (states[128 * n_states:] == SENTINEL).all() and (status[n:] == STATUS_FILL).all()
    if n == 1:
        assert status[0] == HS_INITIATED
    else:
        assert {HS_INITIATED, ERR_INVALID_ARG, ERR_LOW_ORDER} == set(status[:n].tolist())
        ok = np.flatnonzero(status[:n] == HS_INITIATED)
        assert {int(d["flags"][j]) & 1 for j in ok} == {0, 1} and any(int(d["flags"][j]) > 1 for j in ok)


def run_finish(dev, c, d_states, d_keys, use_gate=True, stream=None):
    w = world()
    d_arena, d_pkts, d_types, d_gate = up(c.arena), up(c.pkts), up(c.types), up(c.gate)
    d_self, d_slots, d_psk = up(w.responder), up(c.slots), up(w.psk)
    _, work, verdict = cases.finish_outputs(c)
    d_work, d_verdict = up(work), torch.from_numpy(verdict.copy()).cuda()
    noise.finish_batch(dev, d_arena, d_pkts, d_types, d_gate if use_gate else None, d_self, d_slots, d_states, d_psk,
                       d_keys, d_work, d_verdict, stream=stream, n=c.n, n_slots=len(c.slots), n_states=c.n_states,
                       n_peers=N_PEERS, n_keys=c.n_keys)
    torch.cuda.synchronize()
    for t, a, what in ((d_arena, c.arena, "d_arena"), (d_pkts, c.pkts, "d_pkts"), (d_slots, c.slots, "d_slots"),
                       (d_self, w.responder, "d_responder")):
        assert t.cpu().numpy().tobytes() == a.tobytes(), f"the finish step wrote {what}"
    return d_states.cpu().numpy(), d_keys.cpu().numpy(), d_work.cpu().numpy(), d_verdict.cpu().numpy()


def check_finish(got, want, c, what):
    (states, keys, work, verdict), (want_states, want_keys, want_work, want_verdict) = got, want
    bad = np.flatnonzero(verdict != want_verdict)
    assert len(bad) == 0, (f"{what}: {len(bad)} verdicts differ, first at row {bad[0]} ({c.kinds[bad[0]]}): "
                           f"got {verdict[bad[0]]}, want {want_verdict[bad[0]]}")
    differ(keys, want_keys, 48, f"{what}: d_keys")
    differ(states, want_states, 128, f"{what}: d_states")
    differ(work, want_work, WORK, f"{what}: d_work")


@pytest.mark.parametrize("n", SIZES)
def test_finish_batch_matches_the_host_form_twice_and_again(dev, n):
    c = cases.finish_case(n)
    # the states are made by an initiate launch on the device, then edited as the case says
    d_made, made, msgs, status = run_initiate(dev, c.n_hs, plain=True)
    assert (status[:c.n_hs] == HS_INITIATED).all()
    differ(msgs, c.msgs, PITCH, "d_msgs of the initiate launch")
    words = d_made.view(torch.int32)
    for row, field, value in c.edits:
        words[32 * row + HS_STATE_DTYPE.fields[field][1] // 4] = value - (1 << 32 if value >= 1 << 31 else 0)
    differ(d_made.cpu().numpy(), c.states, 128, "the states that go into the finish step")
    want = cases.finish_expect(c)
    assert want[3][:n].tolist() == c.want.tolist()
    assert not want[2][:WORK * n].any() and (want[2][WORK * n:] == SENTINEL).all()
    keys0 = cases.finish_outputs(c)[0]
    runs = []
    for _ in range(2):  # two fresh copies of the inputs: the duplicate rule does not depend on timing
        d_states, d_keys = d_made.clone(), up(keys0)
        runs.append((run_finish(dev, c, d_states, d_keys), d_states, d_keys))
        check_finish(runs[-1][0], want, c, f"run {len(runs)}")
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a.tobytes() == b.tobytes()
    if n > 1:
        q = c.kinds.index("forged")
        assert runs[0][0][3][q:q + 3].tolist() == [ERR_AUTH, HS_FINISHED, ERR_NO_HANDSHAKE]
    if n >= 290:  # an authentic copy in the second workgroup of a response in the first
        assert c.kinds[n - 1] == "late_copy" and runs[0][0][3][[0, n - 1]].tolist() == [HS_FINISHED, ERR_NO_HANDSHAKE]
    # again on the finished states: every formerly finished row finds no handshake, keys and states stay
    (states, keys, _, verdict), d_states, d_keys = runs[0]
    again = run_finish(dev, c, d_states, d_keys)
    check_finish(again, cases.finish_expect(c, states=states.view(HS_STATE_DTYPE), keys=keys.view(AEAD_KEY_DTYPE)), c, "again")
    was = verdict[:n] == HS_FINISHED
    assert was.any() and (again[3][:n][was] == ERR_NO_HANDSHAKE).all()
    assert again[0].tobytes() == states.tobytes() and again[1].tobytes() == keys.tobytes()


def test_null_gate_and_null_psk(dev):
    w = world()
    c = cases.finish_case(67)
    d_states, d_keys = up(c.states), up(cases.finish_outputs(c)[0])
    check_finish(run_finish(dev, c, d_states, d_keys, use_gate=False), cases.finish_expect(c, use_gate=False), c, "no gate")
    # d_psk NULL is the zero key for every peer
    d_states, d_keys = up(c.states), up(cases.finish_outputs(c)[0])
    _, work, verdict = cases.finish_outputs(c)
    d_work, d_verdict = up(work), torch.from_numpy(verdict.copy()).cuda()
    noise.finish_batch(dev, up(c.arena), up(c.pkts), up(c.types), up(c.gate), up(w.responder), up(c.slots), d_states, None,
                       d_keys, d_work, d_verdict, n=c.n, n_slots=len(c.slots), n_states=c.n_states, n_peers=N_PEERS,
                       n_keys=c.n_keys)
    torch.cuda.synchronize()
    got = (d_states.cpu().numpy(), d_keys.cpu().numpy(), d_work.cpu().numpy(), d_verdict.cpu().numpy())
    check_finish(got, cases.finish_expect(c, psk=None), c, "no psk")
    assert {ERR_AUTH, HS_FINISHED} <= set(got[3][:c.n].tolist())


def test_arguments_of_both_batches(dev):
    w = world()
    n = 67
    d, n_states, n_keys = cases.start_batch(n)
    states, msgs, status = cases.initiate_outputs(n, n_states)
    d_start, d_pub, d_table = up(d), up(np.frombuffer(w.public, np.uint8)), up(w.table)
    d_states, d_msgs, d_status = up(states), up(msgs), torch.from_numpy(status.copy()).cuda()

    def initiate(**kw):
        a = dict(start=d_start, static_public=d_pub, table=d_table, states=d_states, msgs=d_msgs, status=d_status,
                 n_keys=n_keys, n=n, n_peers=N_PEERS, n_states=n_states)
        a.update(kw)
        noise.initiate_batch(dev, **a)

    initiate(n=0)  # a no-op
    initiate(n=0, start=None, msgs=None, status=None)
    for kw in (dict(start=None), dict(static_public=None), dict(msgs=None), dict(status=None), dict(n=(1 << 28) + 1),
               dict(start=d_start.data_ptr() + 2), dict(static_public=d_pub.data_ptr() + 1),
               dict(table=d_table.data_ptr() + 2), dict(states=d_states.data_ptr() + 2), dict(msgs=d_msgs.data_ptr() + 1),
               dict(status=d_status.data_ptr() + 2)):
        with pytest.raises(_lib.WgcsError) as ei:
            initiate(**kw)
        assert ei.value.code == ERR_INVALID_ARG, kw
    good = [dev.h, d_start.data_ptr(), n, d_pub.data_ptr(), d_table.data_ptr(), N_PEERS, n_keys, d_states.data_ptr(),
            n_states, d_msgs.data_ptr(), d_status.data_ptr(), None]
    for k in (0, 4, 7):  # no context; a table is required where its count says there is one
        args = list(good)
        args[k] = None
        assert dev.lib.wgcs_handshake_initiate_batch(*args) == ERR_INVALID_ARG, k
    torch.cuda.synchronize()
    assert (d_status.cpu().numpy() == STATUS_FILL).all() and (d_msgs.cpu().numpy() == SENTINEL).all()
    assert (d_states.cpu().numpy() == SENTINEL).all()
    initiate(n_states=0, states=None)  # with an empty table every descriptor is out of range, and nothing is read
    torch.cuda.synchronize()
    assert (d_status.cpu().numpy()[:n] == ERR_INVALID_ARG).all() and (d_msgs.cpu().numpy() == SENTINEL).all()

    c = cases.finish_case(67)
    keys, work, verdict = cases.finish_outputs(c)
    t = dict(arena=up(c.arena), pkts=up(c.pkts), types=up(c.types), gate=up(c.gate), responder=up(w.responder),
             slots=up(c.slots), states=up(c.states), psk=up(w.psk), keys=up(keys), work=up(work),
             verdict=torch.from_numpy(verdict.copy()).cuda())

    def finish(**kw):
        a = dict(t, n=c.n, n_slots=len(c.slots), n_states=c.n_states, n_peers=N_PEERS, n_keys=c.n_keys)
        a.update(kw)
        noise.finish_batch(dev, **a)

    finish(n=0)
    cases_bad = [dict(arena=None), dict(pkts=None), dict(types=None), dict(responder=None), dict(work=None),
                 dict(verdict=None), dict(gate=t["verdict"]), dict(n=(1 << 28) + 1), dict(n_slots=len(c.slots) - 1),
                 dict(pkts=t["pkts"].data_ptr() + 4)]
    cases_bad += [{k: t[k].data_ptr() + 2} for k in ("types", "gate", "responder", "slots", "states", "psk", "keys", "work",
                                                     "verdict")]
    for kw in cases_bad:
        with pytest.raises(_lib.WgcsError) as ei:
            finish(**kw)
        assert ei.value.code == ERR_INVALID_ARG, kw
    order = ["arena", "pkts", "types", "gate", None, "responder", "slots", None, "states", None, "psk", None, "keys", None,
             "work", "verdict"]
    counts = {4: c.n, 7: len(c.slots), 9: c.n_states, 11: N_PEERS, 13: c.n_keys}
    good = [dev.h] + [counts[i] if k is None else t[k].data_ptr() for i, k in enumerate(order)] + [None]
    for k in (0, 7, 9, 13):  # no context, and d_slots, d_states, d_keys with a count
        args = list(good)
        args[k] = None
        assert dev.lib.wgcs_handshake_finish_batch(*args) == ERR_INVALID_ARG, k
    torch.cuda.synchronize()
    assert (t["verdict"].cpu().numpy() == STATUS_FILL).all() and (t["keys"].cpu().numpy() == SENTINEL).all()
    assert t["states"].cpu().numpy().tobytes() == c.states.tobytes() and (t["work"].cpu().numpy() == SENTINEL).all()
    finish(n_slots=0, slots=None)  # no handshake is in flight: the table is not read
    torch.cuda.synchronize()
    v = t["verdict"].cpu().numpy()[:c.n]
    assert set(v.tolist()) == {HS_NONE, ERR_INVALID_ARG, ERR_NO_HANDSHAKE} and not t["work"].cpu().numpy()[:WORK * c.n].any()


# ----------------------------------------------------------------------- chain
def test_whole_handshake_on_one_stream_and_transport_both_ways(dev):
    """wgcs_handshake_initiate_batch (device A) -> its d_msgs as B's arena -> wgcs_recv_classify_batch ->
    wgcs_handshake_screen_batch -> wgcs_handshake_consume_batch -> wgcs_handshake_respond_batch (device B) ->
    B's d_msgs as A's arena -> classify -> screen -> wgcs_handshake_finish_batch -> wgcs_aead_seal_batch under A's
    send rows -> wgcs_aead_open_batch under B's recv rows, and the reverse direction, all enqueued on one stream.
    The host builds descriptors only: B's are written before anything runs, since its peer rows, indices and
    ephemeral keys do not depend on what A sends.  Five peers in either table, five handshakes in flight."""
    rng = np.random.default_rng(20261021)
    n = 5
    a_private, b_private = rng.bytes(32), rng.bytes(32)
    a_resp, a_public = noise.responder_init(a_private)
    b_resp, b_public = noise.responder_init(b_private)
    others = [noise_ref.public_key(rng.bytes(32)) for _ in range(4)]  # both tables hold 5 peers
    a_table = noise.peer_keys_build(a_resp, [b_public] + others, [10, 11, 12, 13, 14])  # A's peers: B among them
    b_table = noise.peer_keys_build(b_resp, [a_public] + others, [20, 21, 22, 23, 24])  # B's peers: A among them
    a_row_b, b_row_a = noise.peer_keys_find(a_table, b_public), noise.peer_keys_find(b_table, a_public)
    psk = rng.bytes(32)
    a_psk, b_psk = np.zeros((5, 32), np.uint8), np.zeros((5, 32), np.uint8)
    a_psk[a_row_b] = b_psk[b_row_a] = np.frombuffer(psk, np.uint8)
    a_index = [int(x) for x in rng.choice(2**31, n, replace=False) + 1]
    b_index = [int(x) for x in rng.choice(2**31, n, replace=False) + 2**31]
    n_keys = 2 * n + 1
    start, resp = np.zeros(n, HS_START_DTYPE), np.zeros(n, HS_RESP_DTYPE)
    for j in range(n):
        cookie_ = rng.bytes(16)
        start[j] = (j, a_row_b, a_index[j], 2 * j, 2 * j + 1, j & 1, np.frombuffer(rng.bytes(12), np.uint8), 0,
                    np.frombuffer(rng.bytes(32), np.uint8), np.frombuffer(cookie_, np.uint8), 0)
        resp[j] = (j, b_row_a, b_index[j], 2 * j, 2 * j + 1, 0, 0, np.frombuffer(rng.bytes(32), np.uint8), 0)
    a_slots = router.session_table(np.array(a_index, np.uint32), np.arange(n, dtype=np.uint32))
    none = router.session_table(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    a_checker = np.frombuffer(cookie_ref.Checker(a_public).tobytes(), cookie.COOKIE_CHECKER_DTYPE)
    b_checker = np.frombuffer(cookie_ref.Checker(b_public).tobytes(), cookie.COOKIE_CHECKER_DTYPE)
    mtu, slot = 1420, 256
    plain = [bytes([0x45, 0, 0, 40 + 4 * j]) + rng.bytes(36 + 4 * j) for j in range(2 * n)]  # A's packets, then B's
    seal_arena = np.full(2 * n * slot + 64, SENTINEL, np.uint8)
    seal_pkts, open_pkts = np.zeros(2 * n, AEAD_PKT_DTYPE), np.zeros(2 * n, AEAD_PKT_DTYPE)
    for i, p in enumerate(plain):
        j, off = i % n, i * slot + 1 + i  # any byte offset
        seal_arena[off + 16:off + 16 + len(p)] = np.frombuffer(p, np.uint8)
        seal_pkts[i] = (off, 7 + i, len(p), 2 * j)  # both sides send under key row 2j of their own table
        size = 32 + len(p) + (-len(p)) % 16
        open_pkts[i] = (off, 0, size, 2 * j + 1)    # and receive under row 2j + 1

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        i32 = lambda m, fill=STATUS_FILL: torch.full((m,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
        u8 = lambda m, fill=SENTINEL: torch.full((m,), fill, dtype=torch.uint8, device="cuda")  # noqa: E731
        d_start, d_resp = up(start), up(resp)
        d_a_pub, d_a_table, d_a_self, d_a_psk = up(np.frombuffer(a_public, np.uint8)), up(a_table), up(a_resp), up(a_psk)
        d_b_table, d_b_self, d_b_psk = up(b_table), up(b_resp), up(b_psk)
        d_a_slots, d_none, d_a_checker, d_b_checker = up(a_slots), up(none), up(a_checker), up(b_checker)
        d_states, d_a_keys, d_b_keys = u8(128 * n), u8(48 * n_keys), u8(48 * n_keys)
        d_init_msgs, d_resp_msgs = u8(PITCH * n), u8(96 * n)
        d_status_a, d_status_b = i32(n), i32(n)
        d_size_b, d_size_a = i32(n, 148), i32(n, 92)
        d_pkts_b, d_pkts_a = u8(24 * n), u8(24 * n)
        d_type_b, d_type_a, d_screen_b, d_screen_a, d_consumed, d_finished = (i32(n) for _ in range(6))
        d_init, d_work = u8(128 * n), u8(WORK * n)
        d_seal_arena, d_seal_pkts, d_open_pkts = up(seal_arena), up(seal_pkts), up(open_pkts)
        d_out_len, d_pkt_len = i32(2 * n), i32(2 * n)
        d_counter = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        stream.synchronize()
        noise.initiate_batch(dev, d_start, d_a_pub, d_a_table, d_states, d_init_msgs, d_status_a, n_keys, stream=stream,
                             n=n, n_peers=5, n_states=n)
        router.classify_batch(dev, d_init_msgs, d_size_b, d_none, d_pkts_b, d_type_b, stride=PITCH, stream=stream, n=n,
                              n_slots=len(none))
        cookie.screen_batch(dev, d_init_msgs, d_pkts_b, d_type_b, d_b_checker, None, d_screen_b, under_load=False,
                            stream=stream, n=n)
        noise.consume_batch(dev, d_init_msgs, d_pkts_b, d_type_b, d_screen_b, d_b_self, d_b_table, d_consumed, d_init,
                            stream=stream, n=n, n_peers=5)
        noise.respond_batch(dev, d_resp, d_init, d_consumed, d_b_table, d_b_psk, d_b_keys, d_resp_msgs, d_status_b,
                            stream=stream, n=n, n_init=n, n_peers=5, n_keys=n_keys)
        router.classify_batch(dev, d_resp_msgs, d_size_a, d_none, d_pkts_a, d_type_a, stride=96, stream=stream, n=n,
                              n_slots=len(none))
        cookie.screen_batch(dev, d_resp_msgs, d_pkts_a, d_type_a, d_a_checker, None, d_screen_a, under_load=False,
                            stream=stream, n=n)
        noise.finish_batch(dev, d_resp_msgs, d_pkts_a, d_type_a, d_screen_a, d_a_self, d_a_slots, d_states, d_a_psk,
                           d_a_keys, d_work, d_finished, stream=stream, n=n, n_slots=len(a_slots), n_states=n, n_peers=5,
                           n_keys=n_keys)
        # A seals its packets (the first n) under its table, B its own (the last n) under its table ...
        transport.seal_batch(dev, d_seal_arena, d_seal_pkts[:24 * n], d_a_keys, mtu, d_out_len[:n], stream=stream, n=n,
                             n_keys=n_keys)
        transport.seal_batch(dev, d_seal_arena, d_seal_pkts[24 * n:], d_b_keys, mtu, d_out_len[n:], stream=stream, n=n,
                             n_keys=n_keys)
        # ... and each opens what the other sealed
        transport.open_batch(dev, d_seal_arena, d_open_pkts[:24 * n], d_b_keys, d_pkt_len[:n], d_counter[:n], stream=stream,
                             n=n, n_keys=n_keys)
        transport.open_batch(dev, d_seal_arena, d_open_pkts[24 * n:], d_a_keys, d_pkt_len[n:], d_counter[n:], stream=stream,
                             n=n, n_keys=n_keys)
        stream.synchronize()
    assert d_status_a.cpu().tolist() == [HS_INITIATED] * n and d_type_b.cpu().tolist() == [1] * n
    assert d_screen_b.cpu().tolist() == [HS_PASS] * n and d_consumed.cpu().tolist() == [HS_CONSUMED] * n
    assert d_status_b.cpu().tolist() == [4] * n and d_type_a.cpu().tolist() == [2] * n
    assert d_screen_a.cpu().tolist() == [HS_PASS] * n and d_finished.cpu().tolist() == [HS_FINISHED] * n
    assert not d_work.cpu().numpy().any()
    a_keys, b_keys = d_a_keys.cpu().numpy().view(AEAD_KEY_DTYPE), d_b_keys.cpu().numpy().view(AEAD_KEY_DTYPE)
    states, init_msgs, resp_msgs = d_states.cpu().numpy().view(HS_STATE_DTYPE), d_init_msgs.cpu().numpy(), d_resp_msgs.cpu().numpy()
    assert (a_keys.view(np.uint8)[-48:] == SENTINEL).all() and (b_keys.view(np.uint8)[-48:] == SENTINEL).all()
    for j in range(n):
        # the restatement's initiator, from the descriptor alone, ends with the keys of A's rows
        eph, ts = start["ephemeral_private"][j].tobytes(), start["timestamp"][j].tobytes()
        msg, h, chain = noise_ref.create_initiation(a_private, b_public, eph, ts, a_index[j])
        msg = cookie_ref.add_macs(noise_resp_ref.mac1_key(b_public), msg, start["cookie"][j].tobytes() if j & 1 else None)[0]
        assert init_msgs[PITCH * j:PITCH * j + 148].tobytes() == msg
        rc, sender, _, _, _, chain = noise_resp_ref.consume_response(a_private, h, chain, eph, a_index[j],
                                                                    resp_msgs[96 * j:96 * j + 92].tobytes(), psk)
        assert (rc, sender) == (0, b_index[j])
        send, recv = noise_resp_ref.initiator_keys(chain)
        assert a_keys[2 * j].tobytes() == noise_resp_ref.aead_key_bytes(send, b_index[j])
        assert a_keys[2 * j + 1].tobytes() == noise_resp_ref.aead_key_bytes(recv, 0)
        assert b_keys[2 * j].tobytes() == noise_resp_ref.aead_key_bytes(recv, a_index[j])
        assert b_keys[2 * j + 1].tobytes() == noise_resp_ref.aead_key_bytes(send, 0)
        assert states[j].tobytes() == np.array([(0, a_index[j], a_row_b, b_index[j], 2 * j, 2 * j + 1, 0xFFFFFFFF, 0, 0, 0, 0)],
                                               HS_STATE_DTYPE).tobytes()
    arena, pkt_len, counter = d_seal_arena.cpu().numpy(), d_pkt_len.cpu().numpy(), d_counter.cpu().numpy()
    for i, p in enumerate(plain):
        off = int(seal_pkts["off"][i])
        assert d_out_len[i].item() == open_pkts["len"][i] and counter[i] == 7 + i
        assert pkt_len[i] == len(p) and arena[off + 16:off + 16 + len(p)].tobytes() == p, f"packet {i} did not come back"
