"""CPU tests of the per-keypair references (tests/replay_ref.py): the
sequential filter, the set-plus-maximum model and the trip rule that the GPU
kernel implements agree -- the ring models in `last` and all 128 ring words
after every trip -- on seeded sequences and on hand-derived edge vectors; the
library's host entry points agree with them; and send_assign_ref reproduces
the documented host step of the send chain on the path scenario."""
import ctypes as C

import numpy as np
import pytest

import path_ref
import replay_ref
from replay_ref import EDGES, Filter, REJECT_AFTER_MESSAGES, SetModel, trip_validate, sequence
from wireguard_amd import _lib, keystate

LIMIT = REJECT_AFTER_MESSAGES
SEED = 20261020


def test_three_models_agree_on_seeded_sequences():
    rng = np.random.default_rng(SEED)
    rows = accepted = 0
    for _ in range(400):
        vals, limit = sequence(rng, int(rng.integers(1, 400)))
        seq, trip, model = Filter(), Filter(), SetModel()
        at = 0
        while at < len(vals):
            m = int(rng.integers(1, 65))
            chunk = vals[at:at + m]
            want = [seq.validate(v, limit) for v in chunk]
            assert [model.validate(v, limit) for v in chunk] == want
            assert trip_validate(trip, chunk, limit) == want, (at, chunk)
            assert trip.state() == seq.state(), at
            at += m
            rows += len(chunk)
            accepted += sum(want)
    assert rows > 50_000 and accepted * 3 >= rows, (rows, accepted)  # not a corpus of rejects


def run(values, limit=LIMIT, f=None):
    f = f or Filter()
    return [f.validate(v, limit) for v in values], f


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_vectors(name):
    values, want = EDGES[name]
    got, f = run(values)
    assert got == want
    model = SetModel()
    assert [model.validate(v, LIMIT) for v in values] == want
    # as one trip, and cut at every place
    for cut in range(len(values) + 1):
        t = Filter()
        assert trip_validate(t, values[:cut], LIMIT) + trip_validate(t, values[cut:], LIMIT) == want, cut
        assert t.state() == f.state(), cut


def test_host_entry_points_match_the_restatement():
    L = _lib.load()
    assert L.wgcs_replay_validate(None, 1, 2) == _lib.ERR_INVALID_ARG
    L.wgcs_replay_reset(None)
    assert keystate.REPLAY_FILTER_DTYPE.itemsize == 1032 and _lib.REJECT_AFTER_MESSAGES == LIMIT
    assert _lib.ERR_REPLAY == replay_ref.ERR_REPLAY and b"replay" in L.wgcs_strerror(_lib.ERR_REPLAY)
    rng = np.random.default_rng(SEED + 1)
    for _ in range(40):
        vals, limit = sequence(rng, 300)
        f = np.zeros(1, keystate.REPLAY_FILTER_DTYPE)
        ref = Filter()
        for v in vals:
            assert keystate.replay_validate(f, v, limit) == ref.validate(v, limit)
        assert np.array_equal(f, replay_ref.filters_to_array([ref]))
        keystate.replay_reset(f)
        assert not f.view(np.uint8).any()
    for name, (values, want) in EDGES.items():
        f = np.zeros(1, keystate.REPLAY_FILTER_DTYPE)
        assert [keystate.replay_validate(f, v) for v in values] == want, name


def test_work_bytes_bounds_the_arrays():
    w = [keystate.work_bytes(n) for n in (0, 1, 1000, 65536, 1 << 24)]
    assert all(b >= a for a, b in zip(w, w[1:])) and w[0] > 0
    assert w[3] >= 28 * 65536 and w[-1] < 1 << 30
    with pytest.raises(_lib.WgcsError):
        keystate.work_bytes((1 << 24) + 1)
    L = _lib.load()
    assert L.wgcs_replay_batch(None, None, None, None, 1, None, 0, 0, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.wgcs_send_assign_batch(None, None, None, None, None, 1, 1, 0, None, 1, None, 0, 0, None, None, None, None,
                                    0, None) == _lib.ERR_INVALID_ARG
    assert C.sizeof(C.c_size_t) == 8


def test_replay_batch_ref_takes_the_rows_open_decrypted():
    pk = np.zeros(8, path_ref.AEAD_PKT_DTYPE)
    pk["key"] = [0, 0, 1, 2, 0xFFFFFFFF, 0, 0, 0]
    pkt_len = np.array([40, 40, 40, 40, 40, -18, 0, -8], np.int32)
    counter = np.array([5, 5, 5, 5, 5, 6, 5, 7], np.uint64)
    verdict, fl = replay_ref.replay_batch_ref(pk, pkt_len, counter, np.zeros(2, keystate.REPLAY_FILTER_DTYPE))
    assert verdict.tolist() == [40, -20, 40, 40, 40, -18, -20, -8]
    assert fl["last"].tolist() == [7, 5] and int(fl["ring"][0, 0]) == (1 << 5 | 1 << 7)


@pytest.mark.parametrize("stride", [4096, 4112])
def test_send_assign_ref_reproduces_the_host_step(stride):
    s = path_ref.scenario(20261019, stride)
    snd = path_ref.send_ref(s)
    nj = len(s.jobs)
    pk, nbufs, job_key, nonce = replay_ref.send_assign_ref(snd.sizes, snd.peer, snd.count, snd.status, path_ref.MAX_SEGS,
                                                           stride, s.key_of_peer, s.first_counter)
    n = len(snd.seal_pkts)
    assert 0 < n < nj * path_ref.MAX_SEGS
    assert np.array_equal(pk[:n], snd.seal_pkts) and np.array_equal(nbufs, snd.nbufs)
    rest = pk[n:]
    assert (rest["key"] == replay_ref.NO_KEY).all() and not rest["len"].any() and not rest["counter"].any()
    assert np.array_equal(rest["off"], np.arange(n, nj * path_ref.MAX_SEGS, dtype=np.uint64) * np.uint64(stride))
    for k in (0, 1):
        kept = [j for j in range(nj) if job_key[j] == k]
        assert kept and int(nonce[k]) == s.first_counter[k] + sum(int(snd.count[j]) for j in kept)
    assert ((job_key == replay_ref.NO_KEY) == (nbufs == 0)).all()
