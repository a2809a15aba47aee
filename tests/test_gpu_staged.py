"""The three device calls of the staged queue (wgcs_staged_stage_batch,
_release_batch, _flush_batch) against the library's host forms, which
tests/test_staged_ref.py pins to the restatement of send.go:331-426.

The cases and the random sequences are those of tests/staged_cases.py.  Every
call runs on the host state and on two device states that have seen the same
calls: every state array, d_where, every status, the want bits, the job table
and *d_n_out are compared whole; d_ring and d_out start as a sentinel and are
compared whole too, so live packet bytes are equal and every other byte is
still the sentinel; the inputs are unchanged; and the two device runs agree
byte for byte."""
import numpy as np
import pytest
import torch

import staged_cases as sc
from test_gpu_cookie import up
from wireguard_amd import keystate, staged
from wireguard_amd._lib import ERR_INVALID_ARG, WgcsError

pytestmark = pytest.mark.gpu


def down(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


class DeviceSide:
    """the device calls on a state of their own"""

    def __init__(self, dev, w):
        self.dev, self.w = dev, w
        h = staged.state(w.n_peers, w.cap, w.stride, fill=sc.SENTINEL)
        self.st = staged.State(*[up(a) for a in h.arrays()], w.n_peers, w.cap, w.stride)

    def arrays(self):
        return [down(t) for t in self.st.arrays()]

    def stage(self, jb):
        n, w = len(jb.count), self.w
        ins = [up(a) for a in (jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key, w.peer_rows)]
        d_where = up(np.full(len(jb.sizes), 0x77777777, np.uint32))
        d_work = torch.full((keystate.work_bytes(n),), 0xC3, dtype=torch.uint8, device="cuda")
        staged.stage_batch(self.dev, *ins[:7], jb.max_segs, ins[7], self.st, d_where, d_work, n_jobs=n,
                           n_ids=len(w.peer_rows))
        torch.cuda.synchronize()
        for t, a in zip(ins, (jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key, w.peer_rows)):
            assert down(t).tobytes() == np.ascontiguousarray(a).tobytes(), "an input changed"
        return down(d_where, np.uint32)

    def release(self, now, n_out_max, rk):
        w, m = self.w, n_out_max
        d_table, d_kp, d_nonce, d_rk = up(w.table), up(w.kp), up(w.nonce), up(rk)
        d_status, d_out = up(np.full(w.n_peers, 0x77, np.int32)), up(np.full(m * w.stride, sc.SENTINEL, np.uint8))
        d_peer, d_count, d_sizes, d_ost = (up(np.full(m, 0x77, t)) for t in (np.uint32, np.int32, np.int32, np.int32))
        d_n = up(np.full(1, 0x77, np.uint32))
        d_work = torch.full((keystate.work_bytes(w.n_peers),), 0xC3, dtype=torch.uint8, device="cuda")
        staged.release_batch(self.dev, now, d_table, d_kp, d_nonce, w.limit, d_rk, self.st, m, d_out, d_peer, d_count, d_sizes,
                             d_ost, d_n, d_status, d_work, n_keys=len(w.nonce))
        torch.cuda.synchronize()
        assert down(d_table).tobytes() == w.table.tobytes() and down(d_kp).tobytes() == w.kp.tobytes()
        assert down(d_nonce).tobytes() == w.nonce.tobytes()
        rk[:] = down(d_rk, rk.dtype)
        return sc.Out(down(d_status, np.int32), down(d_out), down(d_peer, np.uint32), down(d_count, np.int32),
                      down(d_sizes, np.int32), down(d_ost, np.int32), int(down(d_n, np.uint32)[0]))

    def flush(self, actions):
        staged.flush_batch(self.dev, None if actions is None else up(actions), self.st)
        torch.cuda.synchronize()


class DeviceDriver:
    """the host forms and two device states, call by call"""

    def __init__(self, dev, w):
        self.w, self.host, self.sides = w, sc.HostSide(w), [DeviceSide(dev, w), DeviceSide(dev, w)]
        self.calls = 0

    @property
    def st(self):
        return self.host.st

    def same_state(self):
        want = [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in self.st.arrays()]
        for side in self.sides:
            got = [a.tobytes() for a in side.arrays()]
            for name, g, x in zip(("len", "head", "lost", "slot_size", "ring"), got, want):
                assert g == x, name
        self.calls += 1

    def stage(self, jb):
        want = self.host.stage(jb)
        for side in self.sides:
            got = side.stage(jb)
            if len(jb.count):  # n_jobs == 0 is a no-op
                assert got.tolist() == want.tolist()
        self.same_state()
        return want

    def release(self, now, n_out_max):
        rk = self.w.rekey.copy()
        want = self.host.release(now, n_out_max, rk)
        for side in self.sides:
            rk2 = self.w.rekey.copy()
            got = side.release(now, n_out_max, rk2)
            assert rk2.tobytes() == rk.tobytes()
            assert got.n_out == want.n_out
            for name in ("status", "out", "peer", "count", "sizes", "out_status"):
                assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), name
        self.w.rekey[:] = rk
        self.same_state()
        return want

    def flush(self, actions):
        self.host.flush(actions)
        for side in self.sides:
            side.flush(actions)
        self.same_state()


@pytest.mark.parametrize("case,n_peers,cap", sc.CASES, ids=[f"{c.__name__}-cap{cap}" for c, _, cap in sc.CASES])
def test_cases(dev, case, n_peers, cap):
    rng = np.random.default_rng(77)
    d = DeviceDriver(dev, sc.world(rng, n_peers, cap))
    case(d, rng)
    assert d.calls


def test_20_random_sequences(dev):
    staged_total = released = 0
    for seed in range(0, 200, 10):
        d = DeviceDriver(dev, sc.random_world(seed))
        a, b = sc.random_sequence(d, seed)
        staged_total, released = staged_total + a, released + b
    assert staged_total > 100 and released > 20


def test_more_than_a_block_and_a_trip(dev):
    """300 single jobs and 70 three-segment jobs of three peers in one call each: more than one block of the keys
    kernel and more than one 64-job trip of a peer's wave; packets of up to 1,424 bytes (89 rows: two trips of the
    copy); rings that overflow within a call; and a release over 267 peer rows, two blocks of the weighted rank,
    whose budget ends inside the second"""
    rng = np.random.default_rng(9)
    w = sc.world(rng, 267, 128, stride=1472)
    d = DeviceDriver(dev, w)
    ids = [int(w.ids[r]) for r in (0, 5, 266)]
    sizes = [1420, 1419, 1424, 17, 0]
    jb = sc.refused(rng, w, [(ids[k % 3], [sizes[k % 5]], 0) for k in range(300)])
    where = d.stage(jb)
    assert (where < sc.STAGED_EVICTED).all() and d.st.len[[0, 5, 266]].tolist() == [100, 100, 100]
    jb = sc.refused(rng, w, [(ids[(k * k) % 3], [sizes[(k + s) % 5] for s in range(3)], 0) for k in range(70)], max_segs=3)
    where = d.stage(jb)
    assert (where == sc.STAGED_NONE).sum() == 0 and d.st.len[0] == 128 and d.st.lost[0] > 0
    for r in list(range(258)) + [266]:
        w.set_current(r, sc.NOW)
    d.stage(sc.refused(rng, w, [(int(w.ids[r]), [64], 0) for r in range(1, 258)]))  # one packet each for most rows
    total = int(d.st.len.sum())
    o = d.release(sc.NOW, total - 1)
    assert o.status[0] == sc.STAGED_RELEASED and o.status[257] == sc.STAGED_RELEASED
    assert o.status[266] == sc.ERR_BATCH_FULL and o.n_out == total - int(d.st.len[266])
    o = d.release(sc.NOW, total)
    assert o.status[266] == sc.STAGED_RELEASED and not d.st.len.any()


@pytest.mark.parametrize("place", ["highest_row_ends_at_n_jobs", "lowest_row_ends_at_a_key_change"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129])
def test_segment_lengths_around_the_trip(dev, k, place):
    """k jobs of one packet each for one peer, k around the 64 jobs of a trip, into a ring of 128: the peer's segment
    ends at the end of the key order (the highest row, every job staged) or at a short segment of another peer behind
    it; 129 jobs also cross the eviction edge inside the third trip's first row"""
    rng = np.random.default_rng(1000 + k)
    w = sc.world(rng, 3, 128, stride=64)
    d = DeviceDriver(dev, w)
    ids = [int(x) for x in w.ids]
    one = lambda r, i: (ids[r], [i % 17], 0)  # a slot of 64 bytes holds 16 of a packet
    if place == "highest_row_ends_at_n_jobs":
        row, spec = 2, [one(0, 3), one(1, 5)] + [one(2, i) for i in range(k)]
    else:
        row, spec = 0, [one(1, 3)] + [one(0, i) for i in range(k)] + [one(1, 5), one(1, 7)]
    where = d.stage(sc.refused(rng, w, spec))
    assert (where == sc.STAGED_NONE).sum() == 0 and (where == sc.STAGED_EVICTED).sum() == max(k - 128, 0)
    assert d.st.len[row] == min(k, 128) and d.st.lost[row] == max(k - 128, 0)


def test_what_is_refused_writes_nothing(dev):
    rng = np.random.default_rng(2)
    w = sc.world(rng, 3, 4)
    side = DeviceSide(dev, w)
    jb = sc.refused(rng, w, [(int(w.ids[0]), [20], 0)])
    before = [a.copy() for a in side.arrays()]
    good = side.st
    for bad in (staged.State(*good.arrays(), 3, 3, w.stride), staged.State(*good.arrays(), 3, 2048, w.stride),
                staged.State(*good.arrays(), 3, 4, w.stride + 8)):
        side.st = bad
        with pytest.raises(WgcsError) as e:
            side.stage(jb)
        assert e.value.code == ERR_INVALID_ARG
        with pytest.raises(WgcsError):
            side.release(sc.NOW, 2, w.rekey.copy())
    side.st = good
    ins = [up(a) for a in (jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key, w.peer_rows)]
    d_where = up(np.full(1, 0x77777777, np.uint32))
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(WgcsError):  # scratch that is too small
        staged.stage_batch(dev, *ins[:7], 1, ins[7], good, d_where, small, n_jobs=1, n_ids=len(w.peer_rows))
    with pytest.raises(WgcsError):  # the ring as the arena
        staged.stage_batch(dev, good.ring, *ins[1:7], 1, ins[7], good, d_where,
                           torch.zeros(keystate.work_bytes(1), dtype=torch.uint8, device="cuda"), n_jobs=1,
                           n_ids=len(w.peer_rows))
    torch.cuda.synchronize()
    assert down(d_where, np.uint32).tolist() == [0x77777777]
    assert all((a == b).all() for a, b in zip(side.arrays(), before))
