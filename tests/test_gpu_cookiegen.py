"""The cookie generator on the GPU (wgcs_cookie_initiated_batch, _responded_batch,
_consume_batch and _age_batch; the kernels of cookiegen_kernels.hip) against the
host forms of cookiegen.cpp: d_gen, d_peers, d_verdict and d_work compared
whole.  tests/test_cookiegen_ref.py pins the host forms to the restatement of
the reference.

Every output sits between sentinel bytes that must keep their fill, every
read-only input is compared with its upload afterwards, and replies sit at
offsets 0..3 mod 4 in a sentinel-filled arena that must come back untouched.
The sizes are one lane, a full wave, a wave plus one and a block plus one, over
5 peers: rows of one peer then lie in different waves and blocks, so a commit
that depended on their order would show."""
import numpy as np
import pytest
import torch

from cookiegen_cases import REFRESH, SECOND, UNKNOWN, arena_of, lookup_world, sent_arrays, sent_status
from wireguard_amd import cookiegen as cg, noise
from wireguard_amd._lib import (ERR_AUTH, ERR_INVALID_ARG, ERR_NO_HANDSHAKE, ERR_NO_PEER, HS_COOKIE_KEPT, HS_NONE,
                                HS_PEER_COOKIE, HS_PEER_SEEN, WgcsError)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
NOW = 1000 * SECOND
SIZES = [1, 64, 65, 257]


class Guarded:
    """A device buffer with GUARD sentinel bytes in front of and behind its payload."""

    def __init__(self, payload):
        b = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.n = len(b)
        self.whole = torch.from_numpy(np.concatenate([np.full(GUARD, FILL, np.uint8), b, np.full(GUARD, FILL, np.uint8)])).cuda()
        self.t = self.whole[GUARD:GUARD + self.n]

    def get(self, dtype) -> np.ndarray:
        a = self.whole.cpu().numpy()
        assert (a[:GUARD] == FILL).all() and (a[GUARD + self.n:] == FILL).all(), "sentinel bytes were written"
        return a[GUARD:GUARD + self.n].copy().view(dtype)


def up(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def same(a, b):
    assert a.tobytes() == b.tobytes()


class Tables:
    """A world's tables on the device: gen and peers guarded, the rest read-only uploads."""

    def __init__(self, w):
        self.w = w
        self.gen, self.peers = Guarded(w.gen), Guarded(w.peers)
        self.ro = {k: up(getattr(w, k)) for k in ("hs_slots", "states", "slots", "key_peer", "peer_rows")}

    def check(self):
        """The device tables are the world's (which the host forms have written), the read-only ones their uploads."""
        same(self.gen.get(cg.COOKIE_GEN_DTYPE), self.w.gen)
        same(self.peers.get(noise.HS_PEER_DTYPE), self.w.peers)
        for k, t in self.ro.items():
            same(t.cpu().numpy(), getattr(self.w, k))


def sent_both(dev, tb: Tables, kind: str, peer_row, status, stream=None):
    """One initiated / responded call on the host form (the world's gen) and enqueued on the device."""
    w = tb.w
    d, st, msgs, mac1s = sent_arrays(w.rng, kind, peer_row, status)
    (cg.initiated_host if kind == "init" else cg.responded_host)(d, st, msgs, w.gen)
    w.ref_sent(d["peer_row"], st, sent_status(kind), mac1s)  # so that replies made later open
    d_d, d_st, d_msgs = up(d), up(st), up(msgs)
    (cg.initiated_batch if kind == "init" else cg.responded_batch)(dev, d_d, d_st, d_msgs, tb.gen.t, stream=stream,
                                                                   n=len(d), n_peers=w.n_peers)

    def fetch():
        same(d_d.cpu().numpy(), d), same(d_st.cpu().numpy(), st), same(d_msgs.cpu().numpy(), msgs)

    return fetch


def consume_both(dev, tb: Tables, rows, now, stream=None):
    """One consume call on the host form and enqueued on the device: a function that compares the row outputs."""
    w = tb.w
    arena, pkts = arena_of([m for _, m in rows])
    types = np.array([t for t, _ in rows], np.int32)
    want = cg.consume_host(arena, pkts, types, now, w.hs_slots, w.states, w.slots, w.key_peer, w.peer_rows, w.gen, w.peers)
    n = len(rows)
    d_arena, d_pkts, d_types = up(arena), up(pkts), up(types)
    d_work, d_verdict = Guarded(np.full(16 * n, 0xEE, np.uint8)), Guarded(np.full(n, 0x6E6E6E6E, np.int32))
    cg.consume_batch(dev, d_arena, d_pkts, d_types, now, tb.ro["hs_slots"], tb.ro["states"], tb.ro["slots"],
                     tb.ro["key_peer"], tb.ro["peer_rows"], tb.gen.t, tb.peers.t, d_work.t, d_verdict.t, stream=stream,
                     n=n, n_hs_slots=len(w.hs_slots), n_states=len(w.states), n_slots=len(w.slots),
                     n_keys=len(w.key_peer), n_ids=len(w.peer_rows), n_peers=w.n_peers)

    def fetch():
        assert d_verdict.get(np.int32).tolist() == want.tolist()
        assert not d_work.get(np.uint8).any(), "a cookie was left in d_work"
        same(d_arena.cpu().numpy(), arena), same(d_pkts.cpu().numpy(), pkts), same(d_types.cpu().numpy(), types)
        return want.tolist()

    return fetch


def age_both(dev, tb: Tables, now, stream=None):
    cg.age_host(now, tb.w.gen, tb.w.peers)
    cg.age_batch(dev, now, tb.gen.t, tb.peers.t, stream=stream, n_peers=tb.w.n_peers)


def mixed_rows(w, n, rng):
    """n rows: replies that open for every peer through both tables, and every way a row can fail."""
    hs, kp = [(0x1001, 0), (0x1002, 3), (0x1003, 4), (0x2002, 1)], [(0x3001, 2), (0x3002, 1)]
    rows = []
    for _ in range(n):
        kind = rng.choice(["hs", "kp", "nopeer", "len", "other", "auth", "word"], p=[.3, .25, .1, .1, .1, .1, .05])
        if kind in ("hs", "kp"):
            index, row = (hs if kind == "hs" else kp)[int(rng.integers(0, 4 if kind == "hs" else 2))]
            rows.append((3, w.reply(index, row, fast=True)))
        elif kind == "nopeer":
            rows.append((3, w.reply(int(rng.choice([0x4001, UNKNOWN, 0x2001, 0x1004, 0x3003, 0x3004])), 0, fast=True)))
        elif kind == "len":
            rows.append((3, rng.bytes(int(rng.choice([0, 1, 63, 65, 92])))))
        elif kind == "other":
            rows.append((int(rng.choice([0, 1, 2, 4, -1])), rng.bytes(int(rng.choice([64, 32, 148])))))
        elif kind == "auth":
            good = bytearray(w.reply(0x1001, 0, fast=True))
            good[int(rng.integers(8, 64))] ^= 1 << int(rng.integers(0, 8))
            rows.append((3, bytes(good)))
        else:
            rows.append((3, b"\x01\0\0\0" + w.reply(0x1001, 0, fast=True)[4:]))
    return rows


@pytest.mark.parametrize("kind", ["init", "resp"])
@pytest.mark.parametrize("n", SIZES)
def test_sent_sizes(dev, kind, n):
    rng = np.random.default_rng(100 + n)
    tb = Tables(lookup_world(rng))
    ok = sent_status(kind)
    for _ in range(2):  # the second call meets rows that hold a MAC1
        fetch = sent_both(dev, tb, kind, rng.integers(0, tb.w.n_peers + 1, n), rng.choice([ok, HS_NONE, -1, 9 - ok], n, p=[.85, .05, .05, .05]))
        torch.cuda.synchronize()
        fetch()
        tb.check()
    assert not tb.w.gen["claim"].any()


@pytest.mark.parametrize("n", SIZES)
def test_consume_sizes(dev, n):
    rng = np.random.default_rng(200 + n)
    tb = Tables(lookup_world(rng))
    sent_both(dev, tb, "init", [0, 1, 2, 3], [sent_status("init")] * 4)  # peer 4 has no lastMAC1
    seen = set()
    for k in range(2):
        fetch = consume_both(dev, tb, mixed_rows(tb.w, n, rng), NOW + k)
        torch.cuda.synchronize()
        seen.update(fetch())
        tb.check()
    assert not tb.w.gen["claim"].any()
    if n == 257:
        assert seen == {HS_NONE, HS_COOKIE_KEPT, ERR_INVALID_ARG, ERR_NO_PEER, ERR_NO_HANDSHAKE, ERR_AUTH}
        assert (tb.w.peers["flags"] & HS_PEER_COOKIE).tolist() == [2, 2, 2, 2, 0]


def test_duplicates_in_other_waves_and_blocks(dev):
    rng = np.random.default_rng(300)
    tb = Tables(lookup_world(rng))
    w, n = tb.w, 600
    # descriptors of peer 2 in three blocks, of peer 0 in two waves of one block; everything else names peer 4
    rows = np.full(n, 4)
    rows[[3, 300, 598]], rows[[10, 100]] = 2, 0
    f1 = sent_both(dev, tb, "init", rows, [sent_status("init")] * n)
    rows = np.full(n, 1)
    rows[[258, 2]] = 3
    f2 = sent_both(dev, tb, "resp", rows, [sent_status("resp")] * n)
    # three replies with different cookies for peer 3 in three blocks, two for peer 0 a wave apart
    cookies = [bytes([c]) * 16 for c in (1, 2, 3, 4, 5)]
    msgs = [(4, b"")] * n
    for q, c in zip((5, 300, 599), cookies):
        msgs[q] = (3, w.reply(0x1002, 3, c))
    msgs[70], msgs[7] = (3, w.reply(0x1001, 0, cookies[3])), (3, w.reply(0x1001, 0, cookies[4]))
    msgs[400] = (3, w.reply(0x3001, 2, fast=True))
    f3 = consume_both(dev, tb, msgs, NOW)
    torch.cuda.synchronize()
    f1(), f2()
    got = f3()
    assert [got[q] for q in (5, 300, 599, 70, 7, 400)] == [HS_COOKIE_KEPT] * 6 and got.count(HS_NONE) == n - 6
    tb.check()
    assert w.peers["cookie"][3].tobytes() == cookies[2] and w.peers["cookie"][0].tobytes() == cookies[3]
    assert not w.gen["claim"].any()


def test_the_round_trip_back_to_back_on_one_stream(dev):
    rng = np.random.default_rng(400)
    tb = Tables(lookup_world(rng))
    w, ok = tb.w, sent_status("init")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        f = [sent_both(dev, tb, "init", [0, 3, 0, 2], [ok] * 4, stream=stream)]
        f.append(consume_both(dev, tb, [(3, w.reply(0x1001, 0)), (3, w.reply(0x1002, 3)), (3, w.reply(0x3001, 2))], NOW, stream=stream))
        age_both(dev, tb, NOW + REFRESH, stream=stream)  # exactly 120 s: kept
        f.append(consume_both(dev, tb, [(3, w.reply(0x1002, 3))], NOW + 9, stream=stream))
        age_both(dev, tb, NOW + REFRESH + 1, stream=stream)  # rows 0 and 2 go, row 3 was refreshed
        age_both(dev, tb, NOW - 5 * SECOND, stream=stream)  # a clock that went back changes nothing
    stream.synchronize()
    assert [x() for x in f] == [None, [HS_COOKIE_KEPT] * 3, [HS_COOKIE_KEPT]]
    tb.check()
    assert w.peers["flags"].tolist() == [HS_PEER_SEEN, 0, HS_PEER_SEEN, HS_PEER_COOKIE, HS_PEER_SEEN]


def test_age_over_more_than_a_block_of_peer_rows(dev):
    rng = np.random.default_rng(500)
    for n_peers in (1, 64, 65, 257):
        gen, peers = np.zeros(n_peers, cg.COOKIE_GEN_DTYPE), np.zeros(n_peers, noise.HS_PEER_DTYPE)
        gen["cookie_set_at_ns"] = NOW + rng.choice([0, -1, 1, -REFRESH, 5 * SECOND], n_peers)
        peers["flags"] = rng.integers(0, 4, n_peers)
        peers["cookie"] = rng.integers(0, 256, (n_peers, 16))
        d_gen, d_peers = Guarded(gen), Guarded(peers)
        cg.age_batch(dev, NOW + REFRESH, d_gen.t, d_peers.t, n_peers=n_peers)
        torch.cuda.synchronize()
        before = peers.copy()
        cg.age_host(NOW + REFRESH, gen, peers)
        same(d_peers.get(noise.HS_PEER_DTYPE), peers), same(d_gen.get(cg.COOKIE_GEN_DTYPE), gen)
        if n_peers == 257:
            assert 0 < ((before["flags"] ^ peers["flags"]) != 0).sum() < n_peers


def test_row_counts_of_zero(dev):
    tb = Tables(lookup_world(np.random.default_rng(600)))
    w = tb.w
    for kind in ("init", "resp"):
        sent_both(dev, tb, kind, [], [])
    consume_both(dev, tb, [], NOW)()
    cg.age_batch(dev, NOW, tb.gen.t, tb.peers.t, n_peers=0)
    cg.age_batch(dev, NOW, None, None, n_peers=0)
    # descriptors and replies, but tables of no rows: nothing to write, every reply without a peer
    d, st, msgs, _ = sent_arrays(w.rng, "init", [0, 1], [sent_status("init")] * 2)
    cg.initiated_batch(dev, up(d), up(st), up(msgs), None, n=2, n_peers=0)
    arena, pkts = arena_of([w.reply(0x1001, 0, fast=True), b"x" * 64])
    d_v, d_work = Guarded(np.zeros(2, np.int32)), Guarded(np.full(32, 0xEE, np.uint8))
    cg.consume_batch(dev, up(arena), up(pkts), up(np.array([3, 4], np.int32)), NOW, None, None, None, None, None, None, None,
                     d_work.t, d_v.t, n=2, n_hs_slots=0, n_states=0, n_slots=0, n_keys=0, n_ids=0, n_peers=0)
    torch.cuda.synchronize()
    assert d_v.get(np.int32).tolist() == [ERR_NO_PEER, HS_NONE] and not d_work.get(np.uint8).any()
    tb.check()


def test_bad_arguments_leave_everything_untouched(dev):
    tb = Tables(lookup_world(np.random.default_rng(700)))
    w = tb.w
    d, st, msgs, _ = sent_arrays(w.rng, "init", [0, 1], [sent_status("init")] * 2)
    d_d, d_st, d_msgs = up(d), up(st), up(np.concatenate([msgs, np.zeros(64, np.uint8)]))
    for args, kw in (((None, d_st, d_msgs, tb.gen.t), {}), ((d_d, None, d_msgs, tb.gen.t), {}),
                     ((d_d, d_st, None, tb.gen.t), {}), ((d_d, d_st, d_msgs, None), {}),
                     ((d_d, d_st, d_msgs[1:], tb.gen.t), {}), ((d_d, d_st, d_msgs, tb.gen.t[2:]), dict(n_peers=4)),
                     ((d_d, d_st, d_msgs, d_msgs[64:]), dict(n_peers=1)),  # d_gen inside d_msgs
                     ((d_d, d_st, d_msgs, tb.gen.t), dict(n=(1 << 28) + 1))):
        with pytest.raises(WgcsError) as e:
            cg.initiated_batch(dev, *args, **{**dict(n=2, n_peers=5), **kw})
        assert e.value.code == ERR_INVALID_ARG
    arena, pkts = arena_of([w.reply(0x1001, 0, fast=True)] * 2)
    d_arena, d_pkts, d_types = up(arena), up(np.concatenate([pkts.view(np.uint8), np.zeros(8, np.uint8)])), up(np.array([3, 3], np.int32))
    d_work, d_v = Guarded(np.full(32, 0xEE, np.uint8)), Guarded(np.full(2, 0x6E6E6E6E, np.int32))
    good = dict(arena=d_arena, pkts=d_pkts, types=d_types, hs_slots=tb.ro["hs_slots"], states=tb.ro["states"],
                slots=tb.ro["slots"], key_peer=tb.ro["key_peer"], peer_rows=tb.ro["peer_rows"], gen=tb.gen.t,
                peers=tb.peers.t, work=d_work.t, verdict=d_v.t)
    counts = dict(n=2, n_hs_slots=len(w.hs_slots), n_states=len(w.states), n_slots=len(w.slots), n_keys=len(w.key_peer),
                  n_ids=len(w.peer_rows), n_peers=5)
    bad = [{k: None} for k in good]  # every pointer is needed here
    bad += [dict(pkts=d_pkts[4:]), dict(types=d_types[1:]), dict(gen=tb.gen.t[2:], n_peers=4), dict(peers=tb.peers.t[1:], n_peers=4),
            dict(work=d_work.t[2:], n=1), dict(verdict=d_v.t[1:], n=1)]  # misaligned
    bad += [dict(peers=tb.gen.t), dict(work=tb.gen.t), dict(verdict=tb.peers.t), dict(work=d_v.t, n=1),
            dict(gen=tb.peers.t[64:], n_peers=2)]  # two outputs that share bytes
    bad += [dict(n_hs_slots=3), dict(n_slots=6), dict(n=(1 << 28) + 1), dict(n_peers=(1 << 24) + 1)]
    for b in bad:
        a = {**good, **counts, **b}
        with pytest.raises(WgcsError) as e:
            cg.consume_batch(dev, a["arena"], a["pkts"], a["types"], NOW, a["hs_slots"], a["states"], a["slots"],
                             a["key_peer"], a["peer_rows"], a["gen"], a["peers"], a["work"], a["verdict"],
                             **{k: a[k] for k in counts})
        assert e.value.code == ERR_INVALID_ARG, b
    for args, kw in (((None, tb.peers.t), {}), ((tb.gen.t, None), {}), ((tb.gen.t[1:], tb.peers.t), dict(n_peers=4)),
                     ((tb.gen.t, tb.gen.t[64:]), dict(n_peers=2)), ((tb.gen.t, tb.peers.t), dict(n_peers=(1 << 24) + 1))):
        with pytest.raises(WgcsError) as e:
            cg.age_batch(dev, NOW, *args, **{**dict(n_peers=5), **kw})
        assert e.value.code == ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (d_v.get(np.int32) == 0x6E6E6E6E).all() and (d_work.get(np.uint8) == 0xEE).all()
    tb.check()
