"""wgcs_send_assign_batch on the GPU against replay_ref.send_assign_ref (the
jobs in order, each key's nonce counted up).  Every output starts as a marker
and every comparison is exact and whole-array: all n_jobs * max_segs
descriptor rows, d_nbufs, d_job_key and the whole of d_send_nonce; the inputs
must come back as they went in."""
import numpy as np
import pytest
import torch

import replay_ref
from replay_ref import NO_KEY, PEER_NONE, REJECT_AFTER_MESSAGES as LIMIT
from wireguard_amd import _lib, keystate, router
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

MARK = 12345
SEED = 20261020
MAX_SEGS, STRIDE = 64, 2048
N_KEYS = 4
PEER_KEY = {100: 0, 200: 1, 300: 2, 400: 7, 0: 3}  # peer 400's key row is past the table; peer id 0 is a peer
UNLISTED = 555
ERR_TOO_MANY_SEGMENTS = -3


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} rows differ, first at {bad[0]} (got {got[bad[0]]}, want "
                             f"{want[bad[0]]}), last at {bad[-1]}")


def tables(jobs, rng):
    """gso_split's and route_dst's outputs for jobs of (count, status, peer):
    sizes and peers of the slots a job fills, markers and PEER_NONE after."""
    nj = len(jobs)
    sizes = np.full(nj * MAX_SEGS, MARK, np.int32)
    peer = np.full(nj * MAX_SEGS, PEER_NONE, np.uint32)
    count, status = np.zeros(nj, np.int32), np.zeros(nj, np.int32)
    for j, (c, st, p) in enumerate(jobs):
        count[j], status[j] = c, st
        w = min(max(c, 1), MAX_SEGS)
        sizes[j * MAX_SEGS:j * MAX_SEGS + w] = rng.integers(1, 1501, w)
        peer[j * MAX_SEGS:j * MAX_SEGS + w] = p
    return sizes, peer, count, status


def check(dev, jobs, nonce, limit=LIMIT, seed=SEED):
    """Launch on a stream of its own and compare with the reference; returns
    (nbufs, job_key, send_nonce after)."""
    rng = np.random.default_rng(seed)
    sizes, peer, count, status = tables(jobs, rng)
    nj = len(jobs)
    nonce = np.array([np.uint64(x) for x in nonce], np.uint64)
    slots = router.session_table(list(PEER_KEY), list(PEER_KEY.values()), 16)
    want_pk, want_nbufs, want_key, want_nonce = replay_ref.send_assign_ref(sizes, peer, count, status, MAX_SEGS, STRIDE,
                                                                            PEER_KEY, nonce, limit)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_sizes, d_peer, d_count, d_status = (torch.from_numpy(x.view(np.int32).copy()).cuda()
                                              for x in (sizes, peer, count, status))
        d_slots, d_nonce = up(slots), up(nonce)
        d_pk = torch.full((nj * MAX_SEGS * AEAD_PKT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        d_nbufs = torch.full((nj,), MARK, dtype=torch.int32, device="cuda")
        d_key = torch.full((nj,), MARK, dtype=torch.int32, device="cuda")
        work = torch.empty(keystate.work_bytes(nj), dtype=torch.uint8, device="cuda")
        keystate.send_assign_batch(dev, d_sizes, d_peer, d_count, d_status, MAX_SEGS, STRIDE, d_slots, d_nonce, d_pk,
                                   d_nbufs, d_key, work, limit=limit, stream=stream, n_jobs=nj, n_slots=len(slots),
                                   n_keys=len(nonce))
        stream.synchronize()
    for d, h, what in ((d_sizes, sizes, "d_sizes"), (d_peer, peer, "d_peer"), (d_count, count, "d_count"),
                       (d_status, status, "d_status")):
        same(d.cpu().numpy(), h.view(np.int32), what + " is only read")
    same(d_slots.cpu().numpy().view(router.SESSION_SLOT_DTYPE), slots, "d_peer_keys is only read")
    got_pk = d_pk.cpu().numpy().view(AEAD_PKT_DTYPE)
    for field in ("off", "counter", "len", "key"):
        same(got_pk[field], want_pk[field], "d_pkts." + field)
    assert got_pk.tobytes() == want_pk.tobytes()
    nbufs, key, after = d_nbufs.cpu().numpy(), d_key.cpu().numpy().view(np.uint32), d_nonce.cpu().numpy().view(np.uint64)
    same(nbufs, want_nbufs, "d_nbufs")
    same(key, want_key, "d_job_key")
    same(after, want_nonce, "d_send_nonce")
    return nbufs, key, after


def test_segment_counts_keys_interleaved_and_every_drop_reason(dev):
    jobs = [(1, 0, 100), (63, 0, 200), (64, 0, 100), (5, 0, 300), (64, 0, 200), (1, 0, 300),
            (13, ERR_TOO_MANY_SEGMENTS, 100),  # a status
            (63, ERR_TOO_MANY_SEGMENTS, 100),  # the split's own count for that status
            (0, 0, 100), (-1, 0, 100), (65, 0, 100),  # counts out of range
            (7, 0, PEER_NONE),                 # unrouted
            (7, 0, UNLISTED),                  # a peer that the table does not hold
            (7, 0, 400),                       # a peer whose key row is past the table
            (2, 0, 0),                         # peer id 0, key row 3
            (63, 0, 100), (1, 0, 200), (64, 0, 300), (3, 0, 100)]
    first = [7, (1 << 32) + 5, (1 << 40) - 2, 99]
    nbufs, key, after = check(dev, jobs, first)
    assert nbufs.tolist() == [1, 63, 64, 5, 64, 1, 0, 0, 0, 0, 0, 0, 0, 0, 2, 63, 1, 64, 3]
    assert key.tolist() == [0, 1, 0, 2, 1, 2] + [NO_KEY] * 8 + [3, 0, 1, 2, 0]
    assert after.tolist() == [7 + 131, (1 << 32) + 5 + 128, (1 << 40) - 2 + 70, 101]


def test_limit_reached_exactly_and_overrun_by_one(dev):
    limit = 1000
    jobs = [(64, 0, 100), (64, 0, 200), (36, 0, 100),  # key 0 reaches the limit exactly
            (37, 0, 200),                              # key 1 would pass it by one
            (1, 0, 200),                               # ... so this one, which would fit, is dropped too
            (1, 0, 100),                               # key 0 has no nonce left
            (1, 0, 300), (5, 0, 0)]                    # key 2 starts above the limit; key 3 is untouched by all this
    nbufs, key, after = check(dev, jobs, [900, 900, 1001, 0], limit=limit)
    assert nbufs.tolist() == [64, 64, 36, 0, 0, 0, 0, 5]
    assert key.tolist() == [0, 1, 0, NO_KEY, NO_KEY, NO_KEY, NO_KEY, 3]
    assert after.tolist() == [1000, 1000, 1000, 5]


def test_start_next_to_reject_after_messages(dev):
    """Nonces within 3 of the limit: the sums that decide would wrap in 64 bits."""
    assert LIMIT == _lib.REJECT_AFTER_MESSAGES and LIMIT + (1 << 13) + 1 == 1 << 64
    jobs = [(3, 0, 100), (3, 0, 200), (2, 0, 300), (64, 0, 0), (1, 0, 300), (1, 0, 300), (1, 0, 100)]
    nbufs, key, after = check(dev, jobs, [LIMIT - 3, LIMIT - 2, LIMIT - 3, (1 << 64) - 1])
    assert nbufs.tolist() == [3, 0, 2, 0, 1, 0, 0]
    assert after.tolist() == [LIMIT] * 4


def test_many_jobs_of_one_key(dev):
    """Segments of more than one trip: the carry from trip to trip, and a
    limit that a later trip reaches."""
    rng = np.random.default_rng(SEED + 1)
    jobs = [(int(rng.integers(1, 65)), 0, 100 if rng.random() < 0.7 else 200) for _ in range(230)]
    jobs[17] = (5, -5, 100)
    total = [sum(c for c, st, p in jobs if p == peer and st == 0) for peer in (100, 200)]
    nbufs, _, after = check(dev, jobs, [1 << 33, 50, 0, 0])
    assert (nbufs > 0).sum() == 229 and after.tolist() == [(1 << 33) + total[0], 50 + total[1], 0, 0]
    # the same jobs against a limit that key 0 meets in its second trip of 64 jobs and key 1 never
    counts0 = [c for c, st, p in jobs if p == 100 and st == 0]
    limit = (1 << 33) + sum(counts0[:90])
    nbufs, _, after = check(dev, jobs, [1 << 33, 50, 0, 0], limit=limit)
    kept0 = [n for n, (c, st, p) in zip(nbufs, jobs) if p == 100 and st == 0]
    assert all(kept0[:90]) and not any(kept0[90:]) and after.tolist() == [limit, 50 + total[1], 0, 0]


@pytest.mark.parametrize("place", ["highest_key_ends_at_n_jobs", "lowest_key_ends_at_a_key_change"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129])
def test_segment_lengths_around_the_trip(dev, k, place):
    """One key with k jobs of one packet each, k around the 64 rows of a trip:
    its segment ends at the end of the key order (the highest key row, every
    job taking part) or at a short segment of another key behind it."""
    first = [1000, 2000, 3000, 4000]
    if place == "highest_key_ends_at_n_jobs":
        walked, jobs = 3, [(1, 0, 100), (1, 0, 200)] + [(1, 0, 0)] * k  # peer id 0 has key row 3
    else:
        walked, jobs = 0, [(1, 0, 200)] + [(1, 0, 100)] * k + [(1, 0, 200), (1, 0, 200)]
    nbufs, key, after = check(dev, jobs, first)
    assert nbufs.tolist() == [1] * len(jobs)
    assert (key == walked).sum() == k
    assert int(after[walked]) == first[walked] + k


def test_empty_batch_and_small_workspace(dev):
    L = dev.lib
    assert L.wgcs_send_assign_batch(dev.h, None, None, None, None, 0, MAX_SEGS, STRIDE, None, 1, None, 0, LIMIT, None,
                                    None, None, None, 0, None) == 0
    rng = np.random.default_rng(SEED)
    sizes, peer, count, status = tables([(3, 0, 100)] * 10, rng)
    slots = router.session_table(list(PEER_KEY), list(PEER_KEY.values()), 16)
    d = [torch.from_numpy(x.view(np.int32).copy()).cuda() for x in (sizes, peer, count, status)]
    d_slots, d_nonce = up(slots), up(np.full(N_KEYS, 77, np.uint64))
    d_pk = torch.full((10 * MAX_SEGS * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    d_nbufs, d_key = (torch.full((10,), MARK, dtype=torch.int32, device="cuda") for _ in range(2))
    work = torch.empty(keystate.work_bytes(10), dtype=torch.uint8, device="cuda")
    for kw in (dict(work_bytes=64), dict(n_slots=12), dict(max_segs=0)):
        args = dict(max_segs=MAX_SEGS, n_jobs=10, n_slots=16, n_keys=N_KEYS)
        args.update(kw)
        max_segs = args.pop("max_segs")
        with pytest.raises(_lib.WgcsError) as ei:
            keystate.send_assign_batch(dev, *d, max_segs, STRIDE, d_slots, d_nonce, d_pk, d_nbufs, d_key, work, **args)
        assert ei.value.code == _lib.ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert (d_pk.cpu().numpy() == 0xEE).all() and (d_nbufs.cpu().numpy() == MARK).all()
    assert (d_key.cpu().numpy() == MARK).all() and (d_nonce.cpu().numpy().view(np.uint64) == 77).all()
