"""GPU parity of wgcs_checksum_batches where one launch walks many batches
(wireguard_amd/csrc/wgcs_batch_plan.h): every batch's results equal the
oracle's at batch counts around the 32-batch group limit, with empty batches
first, last and next to each other, at sizes around the block and the wave,
for every mode and stream count; the bytes behind every output stay untouched;
batches that grid-stride inside a group; the in-place and overlapping-output
fallbacks; and the ordering the call promises against its streams' other work
(join before the first launch, fork after the last)."""
import os

import numpy as np
import pytest
import torch

import oracle
from wireguard_amd import synth
from wireguard_amd.tun import (MODE_FOLD, MODE_IP4HDR, MODE_L4_FILL, MODE_PARTIAL, MODE_VALIDATE, Device)

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 7, 8, 9, 63, 64, 65, 700]
FLENS = [64, 576, 1500, 4000, 9000]
GUARD = 24  # bytes of 0xEE behind every output


class Pool:
    """Host batches (one per size, frame lengths cycling over FLENS), their
    device copies and the oracle's results, made once for the module."""

    def __init__(self):
        self.host, self.dev, self.ini, self._want = {}, {}, {}, {}
        for i, n in enumerate(s for s in SIZES if s):
            for j in range(2):  # two different batches of every size
                flen = FLENS[(i + 3 * j) % len(FLENS)]
                arena, pkts, _ = synth.make_batch(n, flen, kinds="mixed", seed=1000 + 10 * i + j)
                ini = (np.arange(n, dtype=np.uint64) + np.uint64(j)) * np.uint64(0x9E3779B97F4A7C15)
                self.host[(n, j)] = (arena, pkts)
                self.ini[(n, j)] = ini
                self.dev[(n, j)] = (torch.from_numpy(arena).cuda(), torch.from_numpy(pkts.view(np.uint8).copy()).cuda(),
                                    torch.from_numpy(ini.view(np.uint8).copy()).cuda())

    def want(self, mode, key, with_ini):
        k = (mode, key, with_ini)
        if k not in self._want:
            arena, pkts = self.host[key]
            self._want[k] = oracle.checksum_batch(mode, arena, pkts, self.ini[key] if with_ini else None)
        return self._want[k]


@pytest.fixture(scope="module")
def pool():
    return Pool()


def _sizes(K, seed):
    """K batch sizes from SIZES: empty batches first, last and adjacent where
    the list is long enough, every size present in the long lists."""
    rng = np.random.default_rng(seed)
    ns = [int(x) for x in rng.choice(SIZES, size=K)]
    if K >= 32:
        ns[:len(SIZES)] = SIZES[::-1]
        ns[0] = ns[-1] = 0
        ns[13] = ns[14] = ns[15] = 0
        ns[K // 2] = 700
    elif K == 3:
        ns = [0, 65, 0] if seed % 2 else [9, 0, 700]
    else:
        ns = [0, 64] if seed % 2 else [700, 1]
    return ns


def _run_list(dev, pool, mode, ns, n_streams, seed, device=None):
    """One call over the batches of sizes `ns` (each its own output slice with
    guard bytes behind it); checks results, guards and the bracket events."""
    d = device or dev
    rng = np.random.default_rng(seed)
    w = 1 if mode == MODE_VALIDATE else 2
    items, at = [], 0
    for n in ns:
        at += int(rng.integers(0, 3)) * w  # outputs at odd (VALIDATE) or merely even places
        items.append((n, int(rng.integers(0, 2)), bool(rng.integers(0, 2)), at))
        at += n * w + GUARD
    out = torch.full((at + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(64, dtype=torch.uint8, device="cuda")  # pointers of the empty batches
    bl = []
    for n, j, use_ini, off in items:
        if n == 0:
            bl.append((scratch, scratch, 0, out[off:]))
            continue
        a, p, ini = pool.dev[(n, j)]
        bl.append((a, p, n, out[off:], ini if (mode == MODE_FOLD and use_ini) else None))
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    torch.cuda.synchronize()
    d.checksum_batches(mode, d.batch_list(bl), streams, e0, e1)
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) >= 0.0
    got = out.cpu().numpy()
    keep = np.ones(len(got), dtype=bool)
    for k, (n, j, use_ini, off) in enumerate(items):
        if n == 0:
            continue
        want = pool.want(mode, (n, j), mode == MODE_FOLD and use_ini)
        res = got[off: off + n * w].view(np.uint8 if w == 1 else np.uint16)
        assert np.array_equal(res, want), f"batch {k} (n = {n})"
        keep[off: off + n * w] = False
    assert (got[keep] == 0xEE).all(), "bytes outside the outputs were written"


@pytest.mark.parametrize("mode", [MODE_VALIDATE, MODE_L4_FILL, MODE_FOLD])
@pytest.mark.parametrize("n_streams", [0, 1, 2, 3])
@pytest.mark.parametrize("K", [2, 3, 32, 33, 70])
def test_fused_batches_match_oracle(dev, pool, mode, n_streams, K):
    seed = K * 100 + mode * 10 + n_streams
    _run_list(dev, pool, mode, _sizes(K, seed), n_streams, seed)


@pytest.mark.parametrize("mode", [MODE_PARTIAL, MODE_IP4HDR])
def test_fused_partial_and_ip4hdr(dev, pool, mode):
    _run_list(dev, pool, mode, _sizes(33, 7 + mode), 2, 7 + mode)


def test_fused_equal_batches_take_the_shift_path(dev, pool):
    """Batches of one power-of-two block count (the benchmark's shape), the
    same tuple several times among them."""
    _run_list(dev, pool, MODE_VALIDATE, [64] * 5, 2, 1)
    _run_list(dev, pool, MODE_L4_FILL, [700] * 40, 2, 2)
    a, p, _ = pool.dev[(700, 0)]
    out = torch.full((700 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dev.checksum_batches(MODE_VALIDATE, dev.batch_list([(a, p, 700, out)] * 6), [torch.cuda.Stream()])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:700], pool.want(MODE_VALIDATE, (700, 0), False)) and (got[700:] == 0xEE).all()


def test_fused_batches_grid_stride():
    """A second Device with one block per CU: batches of 5,000 frames take
    several grid-stride passes inside their share of the launch."""
    old = os.environ.get("WGCS_BLOCKS_PER_CU")
    os.environ["WGCS_BLOCKS_PER_CU"] = "1"
    try:
        d2 = Device(0)
    finally:
        if old is None:
            del os.environ["WGCS_BLOCKS_PER_CU"]
        else:
            os.environ["WGCS_BLOCKS_PER_CU"] = old
    try:
        cap = d2.lib.wgcs_num_cu(d2.h) & ~7
        assert 5000 > cap * 8, "the batches must stride"
        hosts = [synth.make_batch(n, 576, kinds="mixed", seed=50 + i) for i, n in enumerate([5000, 5001, 4999, 9])]
        for mode, pick in ((MODE_VALIDATE, [0, 1, 2]), (MODE_L4_FILL, [0, 3, 1, 2])):  # equal block counts; unequal
            w = 1 if mode == MODE_VALIDATE else 2
            devs, outs = [], []
            for i in pick:
                arena, pkts, _ = hosts[i]
                devs.append((torch.from_numpy(arena).cuda(), torch.from_numpy(pkts.view(np.uint8).copy()).cuda()))
                outs.append(torch.full((len(pkts) * w + GUARD,), 0xEE, dtype=torch.uint8, device="cuda"))
            bl = d2.batch_list([(a, p, len(hosts[i][1]), o) for i, (a, p), o in zip(pick, devs, outs)])
            d2.checksum_batches(mode, bl, [torch.cuda.Stream(), torch.cuda.Stream()])
            torch.cuda.synchronize()
            for i, o in zip(pick, outs):
                arena, pkts, _ = hosts[i]
                n = len(pkts)
                got = o.cpu().numpy()
                want = oracle.checksum_batch(mode, arena, pkts)
                assert np.array_equal(got[: n * w].view(want.dtype), want) and (got[n * w:] == 0xEE).all()
    finally:
        d2.close()


def test_inplace_keeps_per_batch_launches(dev):
    """L4_FILL in place on one stream, two batches over one arena (the second
    re-fills some of the first's packets): results and written fields are the
    oracle's, batch after batch."""
    arena, pkts, _ = synth.make_batch(500, 1500, kinds="mixed", valid=False, seed=77)
    parts = [pkts[:300], pkts[200:]]
    a_cpu = arena.copy()
    wants = [oracle.checksum_batch(MODE_L4_FILL, a_cpu, p, inplace=True) for p in parts]
    d_arena = torch.from_numpy(arena).cuda()
    d_pk = [torch.from_numpy(p.view(np.uint8).copy()).cuda() for p in parts]
    outs = [torch.full((len(p) * 2 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for p in parts]
    bl = dev.batch_list([(d_arena, dp, len(p), o) for dp, p, o in zip(d_pk, parts, outs)])
    dev.checksum_batches(MODE_L4_FILL, bl, [torch.cuda.Stream()], inplace=True)
    torch.cuda.synchronize()
    for p, o, want in zip(parts, outs, wants):
        got = o.cpu().numpy()
        assert np.array_equal(got[: len(p) * 2].view(np.uint16), want) and (got[len(p) * 2:] == 0xEE).all()
    assert np.array_equal(d_arena.cpu().numpy(), a_cpu)
    assert not np.array_equal(a_cpu, arena)  # the fields were written


def test_overlapping_out_keeps_the_later_batch(dev, pool):
    """Two batches of different packets write one output on one stream: they
    are not fused, and the later batch's results stay."""
    out = torch.full((700 * 2 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    first, later = pool.dev[(700, 0)], pool.dev[(700, 1)]
    w0, w1 = pool.want(MODE_L4_FILL, (700, 0), False), pool.want(MODE_L4_FILL, (700, 1), False)
    assert not np.array_equal(w0, w1)
    for order, want in (((first, later), w1), ((later, first), w0)):
        bl = dev.batch_list([(a, p, 700, out) for a, p, _ in order])
        dev.checksum_batches(MODE_L4_FILL, bl, [torch.cuda.Stream()])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:1400].view(np.uint16), want) and (got[1400:] == 0xEE).all()


def test_join_before_first_launch(dev, pool):
    """Work queued on stream 1 before the call still comes before batch 1:
    stream 1 is held by a doorbell, then fills batch 1's arena (zeroes until
    then; all-zero frames validate 0); the call, the ring, and a wait on
    stream 1 alone must leave batch 1 validated against the real frames."""
    (a0, p0, _), (a1, p1, _) = pool.dev[(700, 0)], pool.dev[(700, 1)]
    late = torch.zeros_like(a1)
    outs = [torch.full((700 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    bell = dev.host_alloc(64).view(np.uint32)
    torch.cuda.synchronize()
    bell[0] = 0
    try:
        dev.stream_wait_flag(s1, bell, 1)
        with torch.cuda.stream(s1):
            late.copy_(a1, non_blocking=True)
        dev.checksum_batches(MODE_VALIDATE, dev.batch_list([(a0, p0, 700, outs[0]), (late, p1, 700, outs[1])]), [s0, s1])
    finally:
        bell[0] = 1  # ring: never leave a stream gated
    s1.synchronize()
    got = outs[1].cpu().numpy()
    torch.cuda.synchronize()
    want = pool.want(MODE_VALIDATE, (700, 1), False)
    assert want.all() and np.array_equal(got[:700], want) and (got[700:] == 0xEE).all()
    dev.host_free(bell.view(np.uint8))


def test_fork_after_last_launch(dev, pool):
    """Work queued on stream 1 after the call sees batch 0 done, although
    stream 0 (held by a doorbell while the copy is queued) is where batch 0
    belongs: a D2H of batch 0's output on stream 1, read after waiting on
    stream 1 alone."""
    (a0, p0, _), (a1, p1, _) = pool.dev[(700, 0)], pool.dev[(700, 1)]
    outs = [torch.full((700 * 2 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
    host = torch.zeros(700 * 2 + GUARD, dtype=torch.uint8).pin_memory()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    bell = dev.host_alloc(64).view(np.uint32)
    torch.cuda.synchronize()
    bell[0] = 0
    try:
        dev.stream_wait_flag(s0, bell, 1)
        dev.checksum_batches(MODE_L4_FILL, dev.batch_list([(a0, p0, 700, outs[0]), (a1, p1, 700, outs[1])]), [s0, s1])
        with torch.cuda.stream(s1):
            host.copy_(outs[0], non_blocking=True)
    finally:
        bell[0] = 1
    s1.synchronize()
    got = host.numpy().copy()
    torch.cuda.synchronize()
    assert np.array_equal(got[:1400].view(np.uint16), pool.want(MODE_L4_FILL, (700, 0), False))
    assert (got[1400:] == 0xEE).all()
    dev.host_free(bell.view(np.uint8))
