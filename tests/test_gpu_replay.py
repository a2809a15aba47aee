"""wgcs_replay_batch on the GPU against replay_ref.replay_batch_ref (sequential
Validate calls in slot order).  Every comparison is exact and whole-array: the
verdicts, which start as a marker, and all n_keys x 1,032 filter bytes; the
inputs must come back as they went in.  Filters of keys without a row start as
marker bytes and must keep them."""
import numpy as np
import pytest
import torch

import replay_ref
from replay_ref import EDGES, ERR_REPLAY, REJECT_AFTER_MESSAGES as LIMIT
from wireguard_amd import _lib, keystate
from wireguard_amd.keystate import REPLAY_FILTER_DTYPE
from wireguard_amd.transport import AEAD_PKT_DTYPE

pytestmark = pytest.mark.gpu

MARK = 12345
SEED = 20261020
ERR_AUTH, ERR_OUT_OF_RANGE, ERR_INVALID_ARG, ERR_PACKET_TOO_SHORT = -18, -13, -1, -8


def up(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} rows differ, first at {bad[0]} (got {got[bad[0]]}, want "
                             f"{want[bad[0]]}), last at {bad[-1]}")


def untouched_filters(n_keys):
    """Marker bytes: a filter that no row names must come back like this."""
    return np.frombuffer(bytes([0xC3]) * (n_keys * REPLAY_FILTER_DTYPE.itemsize), REPLAY_FILTER_DTYPE).copy()


def launch(dev, keys, pkt_len, counter, filters, limit=LIMIT, alias=False, work_bytes=None):
    """One launch on a stream of its own.  Returns (verdict, filters after);
    checks that the inputs were only read."""
    n = len(keys)
    pk = np.zeros(n, AEAD_PKT_DTYPE)
    pk["key"], pk["off"], pk["len"] = keys, np.arange(n, dtype=np.uint64) * 2048, 100
    pkt_len = np.asarray(pkt_len, np.int32)
    counter = np.asarray(counter, np.uint64)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_pk, d_len, d_ctr, d_f = up(pk), torch.from_numpy(pkt_len.copy()).cuda(), up(counter), up(filters)
        d_verdict = d_len if alias else torch.full((n,), MARK, dtype=torch.int32, device="cuda")
        wb = keystate.work_bytes(n)
        work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
        keystate.replay_batch(dev, d_pk, d_len, d_ctr, d_f, d_verdict, work, limit=limit, stream=stream, n=n,
                              n_keys=len(filters), work_bytes=wb if work_bytes is None else work_bytes)
        stream.synchronize()
    same(d_pk.cpu().numpy().view(AEAD_PKT_DTYPE), pk, "d_pkts is only read")
    same(d_ctr.cpu().numpy().view(np.uint64), counter, "d_counter is only read")
    if not alias:
        same(d_len.cpu().numpy(), pkt_len, "d_pkt_len is only read")
    return d_verdict.cpu().numpy(), d_f.cpu().numpy().view(REPLAY_FILTER_DTYPE)


def check(dev, keys, pkt_len, counter, filters, limit=LIMIT, alias=False):
    """Launch and compare with the reference; returns (verdict, filters after)."""
    keys = np.asarray(keys, np.uint32)
    pk = np.zeros(len(keys), AEAD_PKT_DTYPE)
    pk["key"] = keys
    want_v, want_f = replay_ref.replay_batch_ref(pk, pkt_len, np.asarray(counter, np.uint64), filters, limit)
    got_v, got_f = launch(dev, keys, pkt_len, counter, filters, limit, alias)
    same(got_v, want_v, "d_verdict")
    same(got_f["last"], want_f["last"], "filters.last")
    same(got_f["ring"], want_f["ring"], "filters.ring")
    assert got_f.tobytes() == want_f.tobytes()
    return got_v, got_f


def interleave(rng, per_key):
    """Slot order for per-key sequences: the keys dealt at random, each key's
    own rows in their order.  Returns (keys, counters)."""
    order = np.concatenate([np.full(len(v), k) for k, v in enumerate(per_key)])
    rng.shuffle(order)
    at = [0] * len(per_key)
    counters = []
    for k in order:
        counters.append(per_key[k][at[k]])
        at[k] += 1
    return order.astype(np.uint32), np.array([np.uint64(c) for c in counters], np.uint64)


def test_segment_lengths_around_the_trip(dev):
    rng = np.random.default_rng(SEED)
    lengths = [1, 63, 64, 65, 129, 257]
    per_key = [replay_ref.sequence(rng, n, LIMIT)[0] for n in lengths]
    keys, counters = interleave(rng, per_key)
    filters = np.zeros(len(lengths) + 1, REPLAY_FILTER_DTYPE)
    filters[-1:] = untouched_filters(1)  # a key without a row
    v, _ = check(dev, keys, np.full(len(keys), 40, np.int32), counters, filters)
    assert (v == ERR_REPLAY).any() and (v == 40).sum() * 3 >= len(v)


@pytest.mark.parametrize("shape", ["300_small_keys", "one_key"])
def test_many_keys_and_one_key(dev, shape):
    rng = np.random.default_rng(SEED + 1)
    if shape == "300_small_keys":
        per_key = [replay_ref.sequence(rng, int(rng.integers(1, 4)), LIMIT)[0] for _ in range(300)]
    else:
        per_key = [replay_ref.sequence(rng, 700, LIMIT)[0]]
    keys, counters = interleave(rng, per_key)
    v, _ = check(dev, keys, np.full(len(keys), 1, np.int32), counters, np.zeros(len(per_key), REPLAY_FILTER_DTYPE))
    assert (v == 1).any()


def test_duplicates_in_a_trip_across_trips_and_across_launches(dev):
    base = 5000 + np.arange(200, dtype=np.uint64) * 3
    c = base.copy()
    c[11], c[41], c[63], c[65] = c[7], c[39], c[2], c[62]  # inside the first trip, and over its edge
    c[151], c[199] = c[20], c[70]                           # from other trips
    filters = np.zeros(1, REPLAY_FILTER_DTYPE)
    v, f1 = check(dev, np.zeros(200, np.uint32), np.full(200, 9, np.int32), c, filters)
    assert np.flatnonzero(v == ERR_REPLAY).tolist() == [11, 41, 63, 65, 151, 199]
    # the same filters see the even rows' values again, and new ones
    c2 = np.concatenate([base[::2], base[-1] + 1 + np.arange(50, dtype=np.uint64)])
    v2, _ = check(dev, np.zeros(len(c2), np.uint32), np.full(len(c2), 9, np.int32), c2, f1)
    assert (v2[:100] == ERR_REPLAY).all() and (v2[100:] == 9).all()


@pytest.mark.parametrize("place", ["in_trip", "trip_edge", "launch_edge"])
def test_edge_vectors(dev, place):
    """One key per edge vector and cut.  Rows at or above the limit fill a
    segment up to a trip's edge: they take part and leave the filter alone."""
    names = sorted(EDGES)
    per_key, wants, second = [], [], []
    for name in names:
        values, want = EDGES[name]
        for cut in ([0] if place == "in_trip" else range(1, len(values))):
            if place == "launch_edge":
                per_key.append(values[:cut])
                second.append(values[cut:])
            else:
                pad = (64 - cut) % 64 if place == "trip_edge" else 3
                per_key.append([LIMIT + 7] * pad + values)
            wants.append(want)
    rng = np.random.default_rng(SEED + 2)
    filters = np.zeros(len(per_key), REPLAY_FILTER_DTYPE)
    keys, counters = interleave(rng, per_key)
    v, f1 = check(dev, keys, np.full(len(keys), 40, np.int32), counters, filters)
    got = [[int(x) == 40 for x in v[keys == k]] for k in range(len(per_key))]
    if place == "launch_edge":
        keys2, counters2 = interleave(rng, second)
        v2, _ = check(dev, keys2, np.full(len(keys2), 40, np.int32), counters2, f1)
        got = [g + [int(x) == 40 for x in v2[keys2 == k]] for k, g in enumerate(got)]
    for k, want in enumerate(wants):
        assert got[k][-len(want):] == want and not any(got[k][:-len(want)]), k


def test_descending_run(dev):
    c = 20000 - np.arange(300, dtype=np.uint64) * 37  # leaves the window after 8,128 / 37 rows
    v, f = check(dev, np.zeros(300, np.uint32), np.full(300, 40, np.int32), c, np.zeros(1, REPLAY_FILTER_DTYPE))
    assert (v[:220] == 40).all() and (v[220:] == ERR_REPLAY).all() and int(f["last"][0]) == 20000


def test_rows_that_do_not_take_part(dev):
    n_keys = 3
    #        key          pkt_len               counter
    rows = [(0,           40,                   100),
            (0,           ERR_AUTH,             101),   # passes through, 101 stays free
            (0,           ERR_OUT_OF_RANGE,     102),
            (0,           ERR_INVALID_ARG,      103),
            (0xFFFFFFFF,  40,                   104),
            (n_keys,      40,                   105),
            (0,           0,                    106),   # a keepalive consumes its counter
            (0,           ERR_PACKET_TOO_SHORT, 107),   # so does a packet the trim rejects
            (0,           40,                   101), (0, 40, 102), (0, 40, 103), (0, 40, 104), (0, 40, 105),
            (0,           40,                   106), (0, 40, 107),
            (1,           ERR_AUTH,             5),     # key 1 and key 2 have no row that takes part
            (2,           -3,                   6)]
    keys, pkt_len, counter = (np.array(x) for x in zip(*rows))
    filters = np.zeros(n_keys, REPLAY_FILTER_DTYPE)
    filters[1:] = untouched_filters(2)
    for alias in (False, True):
        v, f = check(dev, keys, pkt_len, counter, filters, alias=alias)
        assert v.tolist() == [40, ERR_AUTH, ERR_OUT_OF_RANGE, ERR_INVALID_ARG, 40, 40, 0, ERR_PACKET_TOO_SHORT,
                              40, 40, 40, 40, 40, ERR_REPLAY, ERR_REPLAY, ERR_AUTH, -3]
        assert f[1:].tobytes() == filters[1:].tobytes()


def test_verdict_aliases_pkt_len(dev):
    rng = np.random.default_rng(SEED + 3)
    per_key = [replay_ref.sequence(rng, n, LIMIT)[0] for n in (130, 70, 5)]
    keys, counters = interleave(rng, per_key)
    pkt_len = rng.choice(np.array([40, 0, ERR_AUTH, ERR_PACKET_TOO_SHORT, 1400], np.int32), len(keys))
    v, _ = check(dev, keys, pkt_len, counters, np.zeros(3, REPLAY_FILTER_DTYPE), alias=True)
    assert (v == ERR_REPLAY).any() and (v == ERR_AUTH).any()


def test_limit_below_the_counters(dev):
    c = np.arange(100, dtype=np.uint64) + 50
    v, f = check(dev, np.zeros(100, np.uint32), np.full(100, 40, np.int32), c, np.zeros(1, REPLAY_FILTER_DTYPE), limit=100)
    assert (v[:50] == 40).all() and (v[50:] == ERR_REPLAY).all() and int(f["last"][0]) == 99


def test_empty_batch_and_small_workspace(dev):
    filters = untouched_filters(2)
    keys, pkt_len, counter = np.zeros(100, np.uint32), np.full(100, 40, np.int32), np.arange(100, dtype=np.uint64)
    # n == 0 touches nothing, whatever the pointers are
    assert dev.lib.wgcs_replay_batch(dev.h, None, None, None, 0, None, 0, LIMIT, None, None, 0, None) == 0
    d_f, d_v = up(filters), torch.full((100,), MARK, dtype=torch.int32, device="cuda")
    work = torch.empty(keystate.work_bytes(100), dtype=torch.uint8, device="cuda")
    keystate.replay_batch(dev, up(np.zeros(100, AEAD_PKT_DTYPE)), torch.from_numpy(pkt_len).cuda(), up(counter), d_f, d_v,
                          work, n=0)
    torch.cuda.synchronize()
    assert (d_v.cpu().numpy() == MARK).all() and d_f.cpu().numpy().tobytes() == filters.tobytes()
    # a workspace that cannot hold the arrays
    for wb in (0, 16, 28 * 100):
        with pytest.raises(_lib.WgcsError) as ei:
            launch(dev, keys, pkt_len, counter, filters, work_bytes=wb)
        assert ei.value.code == ERR_INVALID_ARG, wb
    d_pk, d_len, d_ctr = up(np.zeros(100, AEAD_PKT_DTYPE)), torch.from_numpy(pkt_len).cuda(), up(counter)
    with pytest.raises(_lib.WgcsError):
        keystate.replay_batch(dev, d_pk, d_len, d_ctr, d_f, d_v, work, n=100, work_bytes=64)
    torch.cuda.synchronize()
    assert (d_v.cpu().numpy() == MARK).all() and d_f.cpu().numpy().tobytes() == filters.tobytes()
    # an unaligned workspace is refused too
    with pytest.raises(_lib.WgcsError):
        keystate.replay_batch(dev, d_pk, d_len, d_ctr, d_f, d_v, work.data_ptr() + 4, n=100, work_bytes=work.numel() - 4)


def test_many_rows_few_keys_narrow_counters(dev):
    """70,000 rows: past the sort's single-block and merge paths' small sizes,
    with counters from a range so narrow that most rows collide."""
    rng = np.random.default_rng(SEED + 4)
    n = 70_000
    keys = rng.integers(0, 3, n).astype(np.uint32)
    counters = (rng.integers(0, 12_000, n) + np.arange(n) // 8).astype(np.uint64)
    v, _ = check(dev, keys, np.full(n, 40, np.int32), counters, np.zeros(3, REPLAY_FILTER_DTYPE))
    rejected = int((v == ERR_REPLAY).sum())
    assert 5000 < rejected < n - 5000, rejected


@pytest.mark.parametrize("n_keys", [1, 1 << 24])
def test_work_bytes_serves_every_size(dev, n_keys):
    """work_bytes(n) is an upper bound for both widths of the key, up to the
    largest batch; no row takes part, so only the key order runs and every
    verdict is its pkt_len."""
    filters = up(untouched_filters(1))
    for n in (1, 1024, 1025, 100_000, 1 << 20, 1 << 24):
        d_pk = torch.zeros(n * AEAD_PKT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_pk.view(torch.int32)[5::6] = -1  # key = 0xFFFFFFFF
        d_len = torch.full((n,), ERR_AUTH, dtype=torch.int32, device="cuda")
        d_ctr = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_v = torch.full((n,), MARK, dtype=torch.int32, device="cuda")
        work = torch.empty(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")
        keystate.replay_batch(dev, d_pk, d_len, d_ctr, filters, d_v, work, n=n, n_keys=n_keys)
        torch.cuda.synchronize()
        assert bool((d_v == ERR_AUTH).all()), n
        del d_pk, d_len, d_ctr, d_v, work
    assert filters.cpu().numpy().tobytes() == untouched_filters(1).tobytes()
