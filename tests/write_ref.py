"""The Write calls of a receive batch, one per peer, restated in plain Python
from device/receive.go (test infrastructure only; numpy, no GPU, none of the
library's code):

  RoutineReceiveIncoming sorts the items of a recvmmsg batch into one container
  per peer (:115, :178-186, :220-228).  Each peer's RoutineSendToInternet takes
  its container in slot order (:398-504): an item whose packet is nil (Open
  failed) or whose counter the replay filter rejects is dropped (:407-420);
  every other item is `validated` -- it counts for the peer's books: rxBytes
  (:431), validTailPacket (:421), dataPacketReceived for anything longer
  than a keepalive (:436).  Of those, the packets that survive the length and
  source checks (:432-482) are handed to one Tun.Write in slot order (:483-504).

`write_ref` keeps a dict of per-peer lists in first-appearance order (Go leaves
the order of the peers open; this is the library's documented choice) and
flattens it into the documented fixed layout of include/wgcsum.h.
`gro_ref` then runs oracle.handle_gro per call row on an opened arena."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import oracle
from wireguard_amd.tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE, GRO_CAN_UDP
from wireguard_amd.writeplan import WRITE_GROUP_DTYPE

PEER_NONE = 0xFFFFFFFF
NO_KEY = 0xFFFFFFFF
GROUP_DATA = 1
MIN_MESSAGE = 32  # MessageTransportSize: header + tag of an empty packet
ERR_INVALID_ARG, ERR_PACKET_TOO_SHORT, ERR_OUT_OF_RANGE, ERR_BATCH_FULL = -1, -8, -13, -14
ERR_AUTH, ERR_SOURCE, ERR_REPLAY = -18, -19, -20
MARK_TW = -7


def containers(pkts, verdict, q0, n_msgs, key_peer):
    """{peer: [q, ...]} of one batch in first-appearance order: the items each
    peer's RoutineSendToInternet validates."""
    per_peer = {}
    for q in range(q0, q0 + n_msgs):
        key, v = int(pkts["key"][q]), int(verdict[q])
        if key >= len(key_peer):
            continue  # not a transport message of a listed session: it never reached a peer's queue
        peer = int(key_peer[key])
        if peer == PEER_NONE:
            continue
        if v < 0 and v not in (ERR_SOURCE, ERR_PACKET_TOO_SHORT):
            continue  # Open failed (:407-410) or the replay filter said no (:414-420)
        per_peer.setdefault(peer, []).append(q)
    return per_peer


def write_ref(pkts, verdict, n_msgs, key_peer, offset, cap, calls_per_batch, gro_flags=GRO_CAN_UDP):
    """-> SimpleNamespace(bufs, calls, groups, n_groups, status, keys_of): the
    five output arrays of wgcs_write_build_*, and per call row the set of key
    rows its validated items came from (for the tests' own guards)."""
    n = len(pkts)
    nb = n // n_msgs
    assert nb * n_msgs == n == len(verdict)
    r = SimpleNamespace(bufs=np.zeros(n, GRO_BUF_DTYPE), calls=np.zeros(nb * calls_per_batch, GRO_CALL_DTYPE),
                        groups=np.zeros(nb * calls_per_batch, WRITE_GROUP_DTYPE), n_groups=np.zeros(nb, np.int32),
                        status=np.zeros(nb, np.int32), keys_of=[set() for _ in range(nb * calls_per_batch)])
    for b in range(nb):
        q0, c0 = b * n_msgs, b * calls_per_batch
        per_peer = containers(pkts, verdict, q0, n_msgs, key_peer)
        r.n_groups[b] = len(per_peer)
        r.calls[c0:c0 + calls_per_batch] = (q0, 0, offset, gro_flags)
        r.groups[c0:c0 + calls_per_batch] = (PEER_NONE, -1, 0, 0, 0)
        writes = {peer: [q for q in qs if verdict[q] > 0] for peer, qs in per_peer.items()}
        if any(offset + int(verdict[q]) > cap for qs in writes.values() for q in qs):
            r.status[b] = ERR_OUT_OF_RANGE  # elem.buffer[:offset+len(packet)] past the buffer: Go panics
            continue
        if len(per_peer) > calls_per_batch:
            r.status[b] = ERR_BATCH_FULL
            continue
        at = q0
        for g, (peer, qs) in enumerate(per_peer.items()):
            rx = sum(int(pkts["len"][q]) for q in qs)
            data = any(int(pkts["len"][q]) > MIN_MESSAGE for q in qs)
            r.groups[c0 + g] = (peer, qs[-1], GROUP_DATA if data else 0, len(qs), rx)
            r.calls[c0 + g] = (at, len(writes[peer]), offset, gro_flags)
            r.keys_of[c0 + g] = {int(pkts["key"][q]) for q in qs}
            for q in writes[peer]:
                r.bufs[at] = (pkts["off"][q], offset + int(verdict[q]), cap)
                at += 1
    return r


N_MSGS_SET = (1, 2, 63, 64, 65, 127, 128)
VERDICT_CODES = (0, ERR_AUTH, ERR_REPLAY, ERR_SOURCE, ERR_PACKET_TOO_SHORT, ERR_INVALID_ARG, ERR_OUT_OF_RANGE)


def shapes():
    """(n_msgs, calls_per_batch) over the sets the tests draw from."""
    return [(n, c) for n in N_MSGS_SET for c in sorted({1, 2, n}) if c <= n]


def key_table(rng, n_peers):
    """Key rows -> peers: every peer has a current keypair, the first ones a
    previous one too, one key row belongs to no peer; shuffled."""
    peers = [int(p) for p in rng.choice(1 << 20, n_peers, replace=False) + 1]
    rows = peers + peers[:max(1, n_peers // 3)] + [PEER_NONE]
    rng.shuffle(rows)
    return np.array(rows, np.uint32)


def random_table(rng, n_msgs, n_batches, key_peer, offset=16, cap=1536, p_long=0.002):
    """pkts / verdict of n_batches batches: per batch a few active keys (none,
    one, some, all), rows that name no key or one past the table, and verdicts
    from every code the chain produces; a verdict above cap - offset now and
    then."""
    from wireguard_amd.transport import AEAD_PKT_DTYPE

    n, n_keys = n_msgs * n_batches, len(key_peer)
    pkts, verdict = np.zeros(n, AEAD_PKT_DTYPE), np.zeros(n, np.int32)
    pkts["off"] = rng.permutation(n).astype(np.uint64) * np.uint64(2048) + np.uint64(1 << 33)
    pkts["counter"] = rng.integers(0, 1 << 62, n).astype(np.uint64)
    for b in range(n_batches):
        active = rng.choice(n_keys, int(rng.choice([0, 1, 2, 3, 8, n_keys])) % (n_keys + 1), replace=False)
        p_err = float(rng.choice([0.0, 0.3, 0.9]))
        for q in range(b * n_msgs, (b + 1) * n_msgs):
            u = rng.random()
            key = NO_KEY if u < 0.05 else n_keys if u < 0.08 else int(rng.choice(active)) if len(active) else NO_KEY
            v = int(rng.choice(VERDICT_CODES)) if rng.random() < p_err else int(rng.integers(1, cap - offset + 1))
            if rng.random() < p_long:
                v = cap - offset + int(rng.integers(1, 100))
            pkts["key"][q], verdict[q] = key, v
            # any uint32 is a length as far as the books go: mostly plausible ones, some that need a 64-bit sum
            pkts["len"][q] = (MIN_MESSAGE if v == 0 or rng.random() < 0.2 else
                              0xFFFFFFFF - int(rng.integers(0, 9)) if rng.random() < 0.02 else
                              MIN_MESSAGE + int(rng.integers(1, 1500)))
    return pkts, verdict


def gro_ref(arena, plan, handle_gro=None):
    """oracle.handle_gro per call row of `plan` (write_ref's result) on a copy
    of the opened arena: what wgcs_handle_gro_batch leaves over all call rows.
    -> SimpleNamespace(arena, bufs, status, n_write, to_write)"""
    gro = handle_gro or oracle.handle_gro
    arena = arena.copy()
    nc = len(plan.calls)
    r = SimpleNamespace(arena=arena, bufs=plan.bufs.copy(), status=np.zeros(nc, np.int32),
                        n_write=np.zeros(nc, np.int32), to_write=np.full(len(plan.bufs), MARK_TW, np.int32))
    for c, (first, cnt, offset, flags) in enumerate(plan.calls.tolist()):
        if cnt == 0:
            continue  # an empty Write: status 0, nothing written
        hdrs = plan.bufs[first:first + cnt]
        bufs = [arena[int(h["off"]):int(h["off"]) + int(h["cap"])] for h in hdrs]
        rc, tw, order, lens = gro(bufs, [int(h["len"]) for h in hdrs], offset, bool(flags & GRO_CAN_UDP))
        r.status[c], r.n_write[c] = rc, len(tw)
        r.to_write[first:first + len(tw)] = tw
        for i in range(cnt):  # the slice headers after the prepend swaps and appends
            r.bufs[first + i] = (hdrs[order[i]]["off"], lens[i], hdrs[order[i]]["cap"])
    return r
