"""wgcs_write_build_host (the scalar rule of wireguard_amd/csrc/wgcs_write_plan.h
through the library, CPU only) against tests/write_ref.py, the plain-Python
restatement of device/receive.go:178-228 and :398-504 -- exact and whole-array
over outputs pre-filled with markers -- and write_ref itself against the
one-call-per-batch host step of tests/path_ref.py on its scenario, where every
batch holds packets of at most one peer."""
from types import SimpleNamespace

import numpy as np
import pytest

import path_ref
import write_ref
from write_ref import (ERR_BATCH_FULL, ERR_OUT_OF_RANGE, ERR_SOURCE, MIN_MESSAGE, NO_KEY, PEER_NONE)
from wireguard_amd import _lib, writeplan
from wireguard_amd.transport import AEAD_PKT_DTYPE
from wireguard_amd.tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE, GRO_CAN_UDP
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

OFFSET, CAP = 16, 1536
BATCHES_PER_SHAPE = 120  # 18 shapes: 2,160 random batches, and the hand-made ones below
MARK8 = 0xC7


def marked(n, dtype):
    return np.frombuffer(bytes([MARK8]) * (n * dtype.itemsize), dtype).copy()


def host_build(pkts, verdict, n_msgs, key_peer, offset, cap, cpb, gro_flags=GRO_CAN_UDP):
    nb = len(pkts) // n_msgs
    o = SimpleNamespace(bufs=marked(len(pkts), GRO_BUF_DTYPE), calls=marked(nb * cpb, GRO_CALL_DTYPE),
                        groups=marked(nb * cpb, WRITE_GROUP_DTYPE), n_groups=marked(nb, np.dtype("<i4")),
                        status=marked(nb, np.dtype("<i4")))
    p0, v0 = pkts.copy(), verdict.copy()
    writeplan.write_build_host(pkts, verdict, n_msgs, key_peer, offset, cap, cpb, o.bufs, o.calls, o.groups,
                               o.n_groups, o.status, gro_flags=gro_flags)
    assert pkts.tobytes() == p0.tobytes() and np.array_equal(verdict, v0), "the inputs are only read"
    return o


def same_plan(got, want, what):
    for name in ("status", "n_groups", "calls", "groups", "bufs"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError(f"{what}: {name} differs in {len(bad)} rows, first {bad[0]}: got {g[bad[0]]}, "
                                 f"want {w[bad[0]]}")


def hand_made():
    """(name, n_msgs, cpb, key_peer, pkts, verdict): the batches the corpus must not lack."""
    out = []
    kp = np.array([5, 9, 5, PEER_NONE], np.uint32)  # keys 0 and 2 are one peer's two keypairs
    def table(n, keys, verdicts, lens=None):
        pk = np.zeros(n, AEAD_PKT_DTYPE)
        pk["off"] = np.arange(n, dtype=np.uint64) * np.uint64(2048)
        pk["key"], pk["len"] = keys, MIN_MESSAGE + 100 if lens is None else lens
        return pk, np.array(verdicts, np.int32)
    out.append(("all 128 kept", 128, 2, kp, *table(128, [0, 1] * 64, [1000] * 128)))
    out.append(("all 128 kept, one group", 128, 1, kp, *table(128, 0, [CAP - OFFSET] * 128)))
    out.append(("no validated row", 64, 2, kp, *table(64, [0, 1, 3, NO_KEY] * 16, [-18, -20, 700, 700] * 16)))
    out.append(("keepalives only", 65, 2, kp, *table(65, 1, [0] * 65, MIN_MESSAGE)))
    out.append(("two keys in one group", 63, 1, kp, *table(63, [0, 2, 2] * 21, [500, 0, ERR_SOURCE] * 21)))
    out.append(("batch full", 127, 1, kp, *table(127, [1] + [0] * 126, [40] * 127)))
    out.append(("out of range and full", 2, 1, kp, *table(2, [0, 1], [CAP - OFFSET + 1, 40])))
    out.append(("out of range in a counted group", 128, 2, kp, *table(128, [0] * 127 + [1], [40] * 127 + [CAP])))
    wide = np.arange(1, 141, dtype=np.uint32)  # 128 peers in one batch
    out.append(("128 groups", 128, 128, wide, *table(128, np.arange(128)[::-1].copy(), [60] * 128)))
    out.append(("128 groups refused", 128, 2, wide, *table(128, np.arange(128), [60] * 128)))
    return out


@pytest.fixture(scope="module")
def corpus():
    """[(name, n_msgs, cpb, key_peer, pkts, verdict, reference plan)]"""
    rng = np.random.default_rng(20261020)
    tables = []
    for n_msgs, cpb in write_ref.shapes():
        key_peer = write_ref.key_table(rng, int(rng.choice([2, 5, 40])))
        pkts, verdict = write_ref.random_table(rng, n_msgs, BATCHES_PER_SHAPE, key_peer, OFFSET, CAP)
        tables.append((f"random {n_msgs}/{cpb}", n_msgs, cpb, key_peer, pkts, verdict))
    tables += hand_made()
    return [t + (write_ref.write_ref(t[4], t[5], t[1], t[3], OFFSET, CAP, t[2]),) for t in tables]


def test_corpus_is_not_vacuous(corpus):
    """Asserted on the reference's own outputs."""
    seen = dict.fromkeys(("batches", "groups>1", "n==0", "two keys", "128 kept", "none", "full", "range", "good",
                          "no key", "past table", "peerless key", "data", "no data", "wide sum"), 0)
    codes = set()
    for name, n_msgs, cpb, key_peer, pkts, verdict, want in corpus:
        nb = len(pkts) // n_msgs
        seen["batches"] += nb
        codes |= {int(v) for v in verdict if v <= 0}
        seen["no key"] += int((pkts["key"] == NO_KEY).sum())
        seen["past table"] += int((pkts["key"] == len(key_peer)).sum())
        listed = pkts["key"] < len(key_peer)
        seen["peerless key"] += int((key_peer[pkts["key"][listed]] == PEER_NONE).sum())
        for b in range(nb):
            st, ng = int(want.status[b]), int(want.n_groups[b])
            rows = slice(b * cpb, (b + 1) * cpb)
            seen["full"] += st == ERR_BATCH_FULL
            seen["range"] += st == ERR_OUT_OF_RANGE
            seen["none"] += ng == 0
            if st:
                assert (want.calls["n"][rows] == 0).all() and (want.groups["peer"][rows] == PEER_NONE).all()
                continue
            seen["good"] += 1
            seen["groups>1"] += ng > 1
            seen["n==0"] += int((want.calls["n"][rows][:ng] == 0).any())
            seen["two keys"] += any(len(k) > 1 for k in want.keys_of[rows])
            seen["128 kept"] += int(want.calls["n"][rows].sum()) == 128
            seen["data"] += int((want.groups["flags"][rows][:ng] == 1).sum())
            seen["no data"] += int((want.groups["flags"][rows][:ng] == 0).sum())
            seen["wide sum"] += int((want.groups["rx_bytes"][rows] > 0xFFFFFFFF).sum())
    assert seen["batches"] >= 2000
    assert all(seen.values()), seen
    assert codes >= set(write_ref.VERDICT_CODES), codes


def test_host_form_matches_the_restatement(corpus):
    for name, n_msgs, cpb, key_peer, pkts, verdict, want in corpus:
        same_plan(host_build(pkts, verdict, n_msgs, key_peer, OFFSET, CAP, cpb), want, name)


def test_host_form_other_scalars():
    """offset 0 and cap == offset + the longest verdict; other flags; a table of one batch."""
    rng = np.random.default_rng(7)
    key_peer = write_ref.key_table(rng, 4)
    pkts, verdict = write_ref.random_table(rng, 65, 6, key_peer, 0, 899, p_long=0)
    pkts["key"][0], verdict[0] = int(np.flatnonzero(key_peer != PEER_NONE)[0]), 900  # a kept row at the limit
    for offset, cap, flags in ((0, 900, 0), (900, 1800, 0xFFFFFFFF), (0, 899, GRO_CAN_UDP)):
        want = write_ref.write_ref(pkts, verdict, 65, key_peer, offset, cap, 2, flags)
        same_plan(host_build(pkts, verdict, 65, key_peer, offset, cap, 2, flags), want, (offset, cap))
        assert ((want.status == ERR_OUT_OF_RANGE).tolist() == [cap == 899] + [False] * 5), (offset, cap)
    want = write_ref.write_ref(pkts[:65], verdict[:65], 65, key_peer, 0, 2000, 65)
    same_plan(host_build(pkts[:65].copy(), verdict[:65].copy(), 65, key_peer, 0, 2000, 65), want, "one batch")


def test_host_form_refuses_bad_arguments():
    L = _lib.load()
    key_peer = np.array([1, 2], np.uint32)
    pkts, verdict = np.zeros(256, AEAD_PKT_DTYPE), np.zeros(256, np.int32)
    o = SimpleNamespace(bufs=marked(256, GRO_BUF_DTYPE), calls=marked(256, GRO_CALL_DTYPE),
                        groups=marked(256, WRITE_GROUP_DTYPE), n_groups=marked(2, np.dtype("<i4")),
                        status=marked(2, np.dtype("<i4")))
    before = [getattr(o, k).tobytes() for k in ("bufs", "calls", "groups", "n_groups", "status")]
    ptr = lambda a: a.ctypes.data
    good = dict(pkts=ptr(pkts), verdict=ptr(verdict), n_msgs=128, n_batches=2, key_peer=ptr(key_peer), n_keys=2,
                offset=16, cap=1536, gro_flags=1, cpb=2, bufs=ptr(o.bufs), calls=ptr(o.calls), groups=ptr(o.groups),
                n_groups=ptr(o.n_groups), status=ptr(o.status))
    bad = [dict(n_msgs=0), dict(n_msgs=129), dict(cpb=0), dict(cpb=129), dict(n_msgs=64, cpb=65),
           dict(n_msgs=1, cpb=1, n_batches=(1 << 28) + 1), dict(offset=-1), dict(offset=1537), dict(offset=17, cap=16)]
    bad += [{k: None} for k in ("pkts", "verdict", "key_peer", "bufs", "calls", "groups", "n_groups", "status")]
    bad += [{k: good[k] + 8} for k in ("pkts", "bufs", "calls")] + [dict(groups=good["groups"] + 4)]
    bad += [{k: good[k] + 2} for k in ("verdict", "key_peer", "n_groups", "status")]
    for change in bad:
        rc = L.wgcs_write_build_host(*{**good, **change}.values())
        assert rc == _lib.ERR_INVALID_ARG, change
        assert [getattr(o, k).tobytes() for k in ("bufs", "calls", "groups", "n_groups", "status")] == before, change
    assert L.wgcs_write_build_host(*{**good, "n_batches": 0}.values()) == 0
    assert [getattr(o, k).tobytes() for k in ("bufs", "calls", "groups", "n_groups", "status")] == before
    assert L.wgcs_write_build_host(*good.values()) == 0
    assert (o.status == 0).all() and (o.n_groups == 1).all()  # 256 keepalives of key 0


@pytest.fixture(scope="module", params=[(4096, 4096), (4112, 4099)], ids=lambda p: f"{p[0]}-{p[1]}")
def path(request):
    return path_ref.run_reference(20261019, *request.param)


def test_path_scenario_one_peer_per_batch(path):
    """On path_ref's scenario the per-peer calls are the host step's calls: the
    non-empty call rows at calls_per_batch = 1 map one to one onto
    host_write_step's rows, and their buffers are identical."""
    s, rcv = path.s, path.rcv
    key_peer = np.array(s.key_peer, np.uint32)
    want = write_ref.write_ref(rcv.pkts, rcv.verdict, path_ref.N_MSGS, key_peer, path_ref.HDR, s.stride, 1)
    assert (want.status == 0).all(), "no batch of the scenario holds two peers"
    rows = np.flatnonzero(want.calls["n"] > 0)
    assert len(rows) == len(rcv.gro_calls) >= 4
    for c, row in enumerate(rows):
        call, ref_call = want.calls[row], rcv.gro_calls[c]
        assert (call["n"], call["offset"], call["flags"]) == (ref_call["n"], ref_call["offset"], ref_call["flags"])
        mine = want.bufs[int(call["first"]):int(call["first"]) + int(call["n"])]
        theirs = rcv.gro_bufs_in[int(ref_call["first"]):int(ref_call["first"]) + int(ref_call["n"])]
        assert mine.tobytes() == theirs.tobytes(), c
    same_plan(host_build(rcv.pkts.copy(), rcv.verdict.copy(), path_ref.N_MSGS, key_peer, path_ref.HDR, s.stride, 1),
              want, "path scenario")
    # job 8: a source the receiver does not allow for peer B -- a group that validates but writes nothing
    snd = path.snd
    rejected = [g for g in want.groups if g["peer"] == path_ref.PEER_B and
                (rcv.verdict[int(g["tail"])] == ERR_SOURCE)]
    assert len(rejected) == 1
    g = rejected[0]
    row = int(np.flatnonzero(want.groups["tail"] == g["tail"])[0])
    assert want.calls["n"][row] == 0 and g["n_valid"] == snd.nbufs[7] > 0
    assert g["flags"] == write_ref.GROUP_DATA and g["rx_bytes"] == int(snd.out_len[7 * path_ref.MAX_SEGS:][:snd.nbufs[7]].sum())
