"""The host forms of the staged queue (wgcs_staged_stage_host, _release_host,
_flush_host) against tests/staged_ref.py, the restatement of StagePackets,
FlushStagedPackets and SendStagedPackets: after every call every state word,
every peer's queue (so every live ring byte and size word), d_where, every
status, the want bits, the job table and its count are compared, and no byte
of the ring or the job table outside a packet has changed.  CPU only."""
import numpy as np
import pytest

import staged_cases as sc
from staged_ref import Packet, Queues
from wireguard_amd import staged
from wireguard_amd._lib import ERR_INVALID_ARG, PEER_NONE, WgcsError


class RefDriver:
    """the restatement and the host forms, call by call"""

    def __init__(self, w):
        self.w, self.ref, self.host = w, Queues(w.n_peers, w.cap, w.stride), sc.HostSide(w)
        self.calls = 0

    @property
    def st(self):
        return self.host.st

    def same_state(self):
        ln, hd, lost, entries, live = sc.live_state(self.st)
        assert ln == self.ref.lens() and hd == self.ref.heads() and lost == self.ref.losts()
        for r in range(self.w.n_peers):
            want = self.ref.entries(r)
            assert entries[r] == want and live[r] == [len(x) for x in want], f"row {r}"
        # outside the live packets the ring is what stage calls left: sentinel, or a packet that has gone
        ring = self.st.ring.reshape(-1, self.w.stride)
        assert (ring[:, :16] == sc.SENTINEL).all() and (ring[:, 16 + sc.LARGEST:] == sc.SENTINEL).all()

    def stage(self, jb):
        inputs = [a.copy() for a in (jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key)]
        want = self.ref.stage(jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key, jb.max_segs,
                              self.w.peer_rows)
        sizes_before, ring_before = self.st.slot_size.copy(), self.st.ring.copy()
        got = self.host.stage(jb)
        assert got.tolist() == want.tolist()
        self.same_state()
        # only the slots d_where names were written, and of those only [16, 16 + size)
        slots = np.zeros(self.w.n_peers * self.w.cap, bool)
        slots[got[got < sc.STAGED_EVICTED]] = True
        assert (self.st.slot_size[~slots] == sizes_before[~slots]).all()
        ring, before = self.st.ring.reshape(-1, self.w.stride), ring_before.reshape(-1, self.w.stride)
        assert (ring[~slots] == before[~slots]).all()
        for s in np.flatnonzero(slots):
            n = int(self.st.slot_size[s])
            assert (ring[s, :16] == before[s, :16]).all() and (ring[s, 16 + n:] == before[s, 16 + n:]).all()
        for a, b in zip(inputs, (jb.arena, jb.sizes, jb.peer, jb.count, jb.status_in, jb.status_out, jb.job_key)):
            assert (a == b).all()
        self.calls += 1
        return got

    def release(self, now, n_out_max):
        w = self.w
        status, want, packets = self.ref.release(now, w.table["peer"], w.kp, w.nonce, w.limit, n_out_max)
        rk, ring_before = w.rekey.copy(), self.st.ring.copy()
        o = self.host.release(now, n_out_max, rk)
        assert o.status.tolist() == status and o.n_out == len(packets) and o.packets(w.stride) == packets
        assert (rk["want"] == (w.rekey["want"] | np.array(want, np.uint32))).all()
        assert (rk["last_sent_ns"] == w.rekey["last_sent_ns"]).all() and (rk["flags"] == w.rekey["flags"]).all()
        w.rekey[:] = rk
        n = o.n_out
        assert o.count.tolist() == [1] * n + [0] * (n_out_max - n) and not o.out_status.any()
        assert o.peer[n:].tolist() == [PEER_NONE] * (n_out_max - n) and not o.sizes[n:].any()
        rows = o.out.reshape(n_out_max, w.stride) if n_out_max else o.out.reshape(0, w.stride)
        for k in range(n_out_max):
            size = int(o.sizes[k])
            assert (rows[k, :16] == sc.SENTINEL).all() and (rows[k, 16 + size:] == sc.SENTINEL).all()
        assert (self.st.ring == ring_before).all()
        self.same_state()
        self.calls += 1
        return o

    def flush(self, actions):
        self.ref.flush(actions)
        ring_before = self.st.ring.copy()
        self.host.flush(actions)
        assert (self.st.ring == ring_before).all()
        self.same_state()
        self.calls += 1


@pytest.mark.parametrize("case,n_peers,cap", sc.CASES, ids=[f"{c.__name__}-cap{cap}" for c, _, cap in sc.CASES])
def test_cases(case, n_peers, cap):
    rng = np.random.default_rng(77)
    d = RefDriver(sc.world(rng, n_peers, cap))
    case(d, rng)
    assert d.calls


def test_200_random_sequences():
    staged_total = released = 0
    shapes = set()
    for seed in range(200):
        d = RefDriver(sc.random_world(seed))
        a, b = sc.random_sequence(d, seed)
        staged_total, released = staged_total + a, released + b
        shapes.add((d.w.cap, d.w.n_peers))
    assert staged_total > 2000 and released > 300
    assert {c for c, _ in shapes} == {1, 4, 8} and {n for _, n in shapes} == set(range(10))


def test_send_staged_packets_whole():
    """release -> send-assign -> stage is SendStagedPackets with its nonce loop: the same packets go out under
    the same nonces, and the same two stay, in order"""
    rng = np.random.default_rng(5)
    w = sc.world(rng, 2, 8)
    d = RefDriver(w)
    pid = int(w.ids[0])
    five = sc.refused(rng, w, [(pid, [20 + k], 0) for k in range(5)])
    d.stage(five)
    w.set_current(0, sc.NOW, nonce=w.limit - 3)
    key = int(w.kp["current"]["send_key"][0])
    literal = Queues(2, 8, w.stride)
    for q in range(5):
        literal.stage_packet(0, Packet(five.packet(q)))
    nonce = w.nonce.copy()
    why, sent = literal.send_staged(0, sc.NOW, w.kp["current"][0], nonce, w.limit)
    assert why == sc.REKEY_WANT_REJECT_MESSAGES and nonce[key] == w.limit
    assert sent == [(w.limit - 3 + k, five.packet(k)) for k in range(3)]
    o = d.release(sc.NOW, 5)
    jb = sc.front(w, o.as_jobs(), sc.NOW)
    d.stage(jb)
    assert [jb.packet(k) for k in range(5) if jb.job_key[k] == key] == [p for _, p in sent]
    assert staged.entries(d.st, 0) == literal.entries(0) == [five.packet(3), five.packet(4)]
    assert (w.nonce == nonce).all() and w.rekey["want"][0] == why


def test_release_without_peers():
    w = sc.world(np.random.default_rng(1), 0, 4)
    d = RefDriver(w)
    o = d.release(sc.NOW, 3)
    assert o.n_out == 0 and o.peer.tolist() == [PEER_NONE] * 3 and not o.count.any()


def test_what_is_refused_writes_nothing():
    rng = np.random.default_rng(2)
    w = sc.world(rng, 3, 4)
    jb = sc.refused(rng, w, [(int(w.ids[0]), [20], 0)])
    where = np.full(1, 0x77, np.uint32)

    def stage(st, work=None, **kw):
        a = dict(arena=jb.arena, sizes=jb.sizes, peer=jb.peer, count=jb.count, status_in=jb.status_in,
                 status_out=jb.status_out, job_key=jb.job_key, max_segs=1, peer_rows=w.peer_rows, st=st, where=where)
        a.update(kw)
        staged.stage_host(work=work, **a)

    good = staged.state(3, 4, sc.STRIDE, fill=sc.SENTINEL)
    bad = [staged.State(*good.arrays(), 3, 3, sc.STRIDE), staged.State(*good.arrays(), 3, 0, sc.STRIDE),
           staged.State(*good.arrays(), 3, 2048, sc.STRIDE)]
    for st in bad:  # a cap that is no power of two, none at all, one past the bound
        st.slot_size, st.ring = np.zeros(3 * st.cap, np.int32), np.full(3 * st.cap * sc.STRIDE, sc.SENTINEL, np.uint8)
        with pytest.raises(WgcsError) as e:
            stage(st)
        assert e.value.code == ERR_INVALID_ARG
    with pytest.raises(WgcsError):
        stage(good, work=np.zeros(1, np.uint64))  # scratch for one job needs 16 bytes
    with pytest.raises(WgcsError):
        stage(good, max_segs=0, sizes=jb.sizes[:0], peer=jb.peer[:0], where=where[:0], arena=jb.arena[:0])
    assert where.tolist() == [0x77] and not good.len.any() and (good.ring == sc.SENTINEL).all()
    lib = staged._lib.load()
    n_out = np.zeros(1, np.uint32)
    assert lib.wgcs_staged_release_host(0, None, None, None, 0, 0, None, None, None, None, None, 0, 4, 128, 0, None, None,
                                        None, None, None, None, None) == ERR_INVALID_ARG  # no n_out
    assert lib.wgcs_staged_release_host(0, None, None, None, 0, 0, None, None, None, None, None, 0, 4, 120, 0, None, None,
                                        None, None, None, n_out.ctypes.data, None) == ERR_INVALID_ARG  # stride
    assert lib.wgcs_staged_flush_host(None, None, None, None, 3) == ERR_INVALID_ARG
    assert lib.wgcs_staged_flush_host(None, None, None, None, 0) == 0
    stage(good)
    assert where.tolist() == [0] and good.len.tolist() == [1, 0, 0]
