"""GPU parity: wgcs_write_build_batch (one wave per receive batch,
write_kernels.hip) against tests/write_ref.py, exact and whole-array, every
output behind marker-filled guard rows; then the builder feeding
wgcs_handle_gro_batch with the rows of three peers interleaved, on one stream
with no synchronisation between the two launches, against write_ref +
oracle.handle_gro per group."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import write_ref
from test_gpu_gro import flow
from write_ref import ERR_BATCH_FULL, ERR_OUT_OF_RANGE, ERR_SOURCE, MARK_TW, NO_KEY, PEER_NONE
from wireguard_amd import _lib, writeplan
from wireguard_amd.transport import AEAD_PKT_DTYPE
from wireguard_amd.tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE, GRO_CAN_UDP
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

pytestmark = pytest.mark.gpu

OFFSET, CAP = 16, 1536
MARK8, GUARD = 0xC7, 3
I32 = np.dtype("<i4")
OUTPUTS = (("bufs", GRO_BUF_DTYPE), ("calls", GRO_CALL_DTYPE), ("groups", WRITE_GROUP_DTYPE), ("n_groups", I32),
           ("status", I32))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def outputs(n_rows, n_calls, nb):
    """Every output as marker bytes, GUARD rows longer than the builder may write."""
    rows = dict(bufs=n_rows, calls=n_calls, groups=n_calls, n_groups=nb, status=nb)
    return SimpleNamespace(**{k: torch.full(((rows[k] + GUARD) * dt.itemsize,), MARK8, dtype=torch.uint8, device="cuda")
                              for k, dt in OUTPUTS}), rows


def download(o, rows):
    """The written part of every output; the guard rows must still be markers."""
    got = SimpleNamespace()
    for k, dt in OUTPUTS:
        a = getattr(o, k).cpu().numpy()
        assert (a[rows[k] * dt.itemsize:] == MARK8).all(), f"{k}: guard rows written"
        setattr(got, k, a[:rows[k] * dt.itemsize].view(dt))
    return got


def build(dev, pkts, verdict, n_msgs, key_peer, offset, cap, cpb, flags=GRO_CAN_UDP):
    nb = len(pkts) // n_msgs
    d_pkts, d_verdict, d_kp = up(pkts), up(verdict), up(key_peer)
    o, rows = outputs(len(pkts), nb * cpb, nb)
    writeplan.write_build_batch(dev, d_pkts, d_verdict, n_msgs, d_kp, offset, cap, cpb, o.bufs, o.calls, o.groups,
                                o.n_groups, o.status, gro_flags=flags, n_batches=nb, n_keys=len(key_peer))
    torch.cuda.synchronize()
    assert d_pkts.cpu().numpy().tobytes() == pkts.tobytes(), "d_pkts is only read"
    assert d_verdict.cpu().numpy().tobytes() == verdict.tobytes(), "d_verdict is only read"
    assert d_kp.cpu().numpy().tobytes() == key_peer.tobytes(), "d_key_peer is only read"
    return download(o, rows)


def same_plan(got, want, what):
    for name, _ in OUTPUTS:
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: got {g[bad[0]]}, "
                                 f"want {w[bad[0]]}")


@pytest.mark.parametrize("n_batches", [1, 4, 5])  # a single wave, a whole workgroup, a workgroup and a spare wave
def test_builder_matches_the_restatement(dev, n_batches):
    rng = np.random.default_rng(20261021 + n_batches)
    refused = good = 0
    for n_msgs, cpb in write_ref.shapes():
        key_peer = write_ref.key_table(rng, int(rng.choice([2, 5, 40])))
        pkts, verdict = write_ref.random_table(rng, n_msgs, n_batches, key_peer, OFFSET, CAP, p_long=0.004)
        want = write_ref.write_ref(pkts, verdict, n_msgs, key_peer, OFFSET, CAP, cpb)
        same_plan(build(dev, pkts, verdict, n_msgs, key_peer, OFFSET, CAP, cpb), want, (n_msgs, cpb, n_batches))
        refused += int((want.status != 0).sum())
        good += int(((want.status == 0) & (want.n_groups > 0)).sum())
    assert refused and good


def table(n, keys, verdicts, lens=132):
    pk = np.zeros(n, AEAD_PKT_DTYPE)
    pk["off"] = np.arange(n, dtype=np.uint64) * np.uint64(2048) + np.uint64(1 << 40)
    pk["key"], pk["len"] = keys, lens
    return pk, np.array(verdicts, np.int32)


def test_refused_batches_beside_good_ones(dev):
    """Five batches of 128 in one launch: good, full, out of range, 128 peers, good."""
    wide = np.concatenate([np.arange(1, 129, dtype=np.uint32), [7, PEER_NONE]]).astype(np.uint32)  # key 128: peer 7 again
    parts = [
        table(128, [0, 1] * 64, [1000] * 128),                                         # two groups, every row kept
        table(128, [0, 1, 2] * 42 + [0, 1], [40] * 128),                               # three peers, two call rows
        table(128, [0] * 127 + [1], [40] * 127 + [CAP - OFFSET + 1]),                  # its last row does not fit
        table(128, np.arange(128)[::-1].copy(), [60] * 128),                           # as many peers as rows
        table(128, [6, 128, NO_KEY, 129] * 32, [0, ERR_SOURCE, 500, 500] * 32, 32),    # one peer, two keys, nothing kept
    ]
    pkts, verdict = np.concatenate([p for p, _ in parts]), np.concatenate([v for _, v in parts])
    want = write_ref.write_ref(pkts, verdict, 128, wide, OFFSET, CAP, 2)
    assert want.status.tolist() == [0, ERR_BATCH_FULL, ERR_OUT_OF_RANGE, ERR_BATCH_FULL, 0]
    assert want.n_groups.tolist() == [2, 3, 2, 128, 1] and want.calls["n"].tolist() == [64, 64, 0, 0, 0, 0, 0, 0, 0, 0]
    assert want.groups[8].tolist() == (7, 4 * 128 + 125, 0, 64, 64 * 32) and want.keys_of[8] == {6, 128}
    same_plan(build(dev, pkts, verdict, 128, wide, OFFSET, CAP, 2), want, "cpb 2")
    want = write_ref.write_ref(pkts, verdict, 128, wide, OFFSET, CAP, 128)
    assert want.status.tolist() == [0, 0, ERR_OUT_OF_RANGE, 0, 0] and (want.calls["n"][3 * 128:4 * 128] == 1).all()
    same_plan(build(dev, pkts, verdict, 128, wide, OFFSET, CAP, 128), want, "cpb 128")


def test_entry_point_refusals_write_nothing(dev):
    key_peer = np.array([1, 2], np.uint32)
    d_pkts, d_verdict, d_kp = up(np.zeros(256, AEAD_PKT_DTYPE)), up(np.zeros(256, np.int32)), up(key_peer)
    o, rows = outputs(256, 256, 2)
    ptr = lambda t: t.data_ptr()
    good = dict(pkts=ptr(d_pkts), verdict=ptr(d_verdict), n_msgs=128, n_batches=2, key_peer=ptr(d_kp), n_keys=2,
                offset=16, cap=1536, gro_flags=1, cpb=2, bufs=ptr(o.bufs), calls=ptr(o.calls), groups=ptr(o.groups),
                n_groups=ptr(o.n_groups), status=ptr(o.status))
    bad = [dict(n_msgs=0), dict(n_msgs=129), dict(cpb=0), dict(cpb=129), dict(n_msgs=64, cpb=65),
           dict(n_msgs=1, cpb=1, n_batches=(1 << 28) + 1), dict(offset=-1), dict(offset=1537), dict(offset=17, cap=16)]
    bad += [{k: None} for k in ("pkts", "verdict", "key_peer", "bufs", "calls", "groups", "n_groups", "status")]
    bad += [{k: good[k] + 8} for k in ("pkts", "bufs", "calls")] + [dict(groups=good["groups"] + 4)]
    bad += [{k: good[k] + 2} for k in ("verdict", "key_peer", "n_groups", "status")]
    for change in bad:
        rc = dev.lib.wgcs_write_build_batch(dev.h, *{**good, **change}.values(), None)
        assert rc == _lib.ERR_INVALID_ARG, change
    assert dev.lib.wgcs_write_build_batch(None, *good.values(), None) == _lib.ERR_INVALID_ARG
    assert dev.lib.wgcs_write_build_batch(dev.h, *{**good, "n_batches": 0}.values(), None) == 0
    torch.cuda.synchronize()
    for k, dt in OUTPUTS:
        assert (getattr(o, k).cpu().numpy() == MARK8).all(), k
    assert dev.lib.wgcs_write_build_batch(dev.h, *good.values(), None) == 0
    dev.sync()
    got = download(o, rows)
    assert (got.status == 0).all() and (got.n_groups == 1).all() and (got.groups["n_valid"][[0, 2]] == 128).all()


# ------------------------------------------------------------- builder -> GRO
STRIDE, N_MSGS, CPB = 2048, 32, 4
P1, P2, P3, P4 = 101, 202, 303, 404
KEY_PEER = np.array([P1, P2, P3, P4, P1], np.uint32)  # key 4: P1's previous keypair


def mixed_scene():
    """Three batches of 32 slots: plaintext packets at offset 16 of their slot,
    every flow owned by one peer, the peers' rows interleaved."""
    tcp4, tcp6, udp4 = flow(6, 200, seed=11), flow(5, 300, v6=True, seed=12), flow(6, 250, udp=True, seed=13)
    tcp4b, udp6 = flow(4, 100, seed=14), flow(3, 400, v6=True, udp=True, seed=15)
    batches = [[], [], []]
    for i in range(6):  # batch 0: P1 (both its keypairs), P2 and P3 take turns; P4 sends a keepalive only
        batches[0] += [(0 if i < 3 else 4, tcp4[i])]
        if i < 5:
            batches[0] += [(1, tcp6[i])]
        batches[0] += [(2, udp4[i])]
        if i == 2:
            batches[0] += [(3, None)]
    batches[1] = [(NO_KEY, "auth"), (0, "auth"), (1, "replay"), (5, tcp4[0])]  # nobody validated anything
    for i in range(4):  # batch 2: P2 first, P3's source is rejected, P1 has two flows
        batches[2] += [(1, udp6[i])] if i < 3 else []
        batches[2] += [(0, tcp4b[i]), (2, "source"), (4, tcp4[i])]
    n = 3 * N_MSGS
    arena = np.full(n * STRIDE + 64, 0x5A, np.uint8)
    pkts, verdict = np.zeros(n, AEAD_PKT_DTYPE), np.full(n, write_ref.ERR_INVALID_ARG, np.int32)
    pkts["off"], pkts["key"] = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE), NO_KEY
    for b, rows in enumerate(batches):
        for i, (key, what) in enumerate(rows):
            q = b * N_MSGS + i + i // 5 + (b & 1)  # an unused slot now and then
            assert q < (b + 1) * N_MSGS
            pkts["key"][q] = key
            if isinstance(what, bytes):
                arena[q * STRIDE + OFFSET:q * STRIDE + OFFSET + len(what)] = np.frombuffer(what, np.uint8)
                pkts["len"][q], verdict[q] = 32 + len(what), len(what)
            else:
                pkts["len"][q] = 32 if what is None else 132
                verdict[q] = {None: 0, "auth": write_ref.ERR_AUTH, "replay": write_ref.ERR_REPLAY,
                              "source": ERR_SOURCE}[what]
    return arena, pkts, verdict


def test_builder_feeds_gro_with_mixed_peers(dev):
    arena, pkts, verdict = mixed_scene()
    nb, n = 3, 3 * N_MSGS
    plan = write_ref.write_ref(pkts, verdict, N_MSGS, KEY_PEER, OFFSET, STRIDE, CPB)
    want = write_ref.gro_ref(arena, plan)
    # the scene is what it claims to be
    assert plan.status.tolist() == [0, 0, 0] and plan.n_groups.tolist() == [4, 0, 3]
    assert plan.groups["peer"].tolist() == [P1, P2, P3, P4, *[PEER_NONE] * 4, P2, P1, P3, PEER_NONE]
    assert plan.calls["n"].tolist() == [6, 5, 6, 0, 0, 0, 0, 0, 3, 8, 0, 0] and plan.keys_of[0] == {0, 4}
    assert (want.status == 0).all()
    merged = [[c for c in range(b * CPB, (b + 1) * CPB) if 0 < want.n_write[c] < plan.calls["n"][c]] for b in range(nb)]
    assert len(merged[0]) == 3 and len(merged[2]) == 2, "batches with coalescing in two or more groups"

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_arena, d_pkts, d_verdict, d_kp = up(arena), up(pkts), up(verdict), up(KEY_PEER)
        o, rows = outputs(n, nb * CPB, nb)
        st, nw = (torch.full((nb * CPB,), 12345, dtype=torch.int32, device="cuda") for _ in range(2))
        tw = torch.full((n,), MARK_TW, dtype=torch.int32, device="cuda")
        stream.synchronize()  # the uploads
        writeplan.write_build_batch(dev, d_pkts, d_verdict, N_MSGS, d_kp, OFFSET, STRIDE, CPB, o.bufs, o.calls, o.groups,
                                    o.n_groups, o.status, stream=stream, n_batches=nb, n_keys=len(KEY_PEER))
        dev.handle_gro_batch(d_arena, o.bufs, o.calls, nb * CPB, st, nw, tw, stream=stream)
        stream.synchronize()
    got = download(o, rows)
    for name in ("status", "n_groups", "calls", "groups"):
        assert getattr(got, name).tobytes() == getattr(plan, name).tobytes(), name
    st, nw, tw = st.cpu().numpy(), nw.cpu().numpy(), tw.cpu().numpy()
    assert np.array_equal(st, want.status) and np.array_equal(nw, want.n_write)
    assert np.array_equal(tw, want.to_write), "toWrite, and the marker everywhere else"
    assert got.bufs.tobytes() == want.bufs.tobytes(), "slice headers after GRO"
    got_arena = d_arena.cpu().numpy()
    if not np.array_equal(got_arena, want.arena):
        bad = np.flatnonzero(got_arena != want.arena)
        raise AssertionError(f"arena: {len(bad)} bytes differ, first in slot {bad[0] // STRIDE}")
    empty = np.flatnonzero(plan.calls["n"] == 0)
    assert len(empty) == 7 and (st[empty] == 0).all() and (nw[empty] == 0).all()
    assert (tw[N_MSGS:2 * N_MSGS] == MARK_TW).all() and not np.array_equal(want.arena, arena)
