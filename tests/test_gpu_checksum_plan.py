"""GPU parity of checksum_batch_kernel where its per-packet plan
(wireguard_amd/csrc/wgcs_cs_plan.h) takes different paths, against
oracle.checksum_batch: the two rows of a wave with different geometry (every
ordered pair of a dozen packet shapes), rows of equal geometry at every
alignment and in both row positions, batch sizes around the wave and the block,
the grid-stride path with its prefetched descriptors, all five modes (FOLD
with `initial`, L4_FILL in place), fused calls of three batches, and the 16-
and 64-lane builds.  Every output has 0xEE guard bytes behind it and the arenas
are compared whole."""
import os

import numpy as np
import pytest
import torch

import oracle
from wireguard_amd import synth
from wireguard_amd.tun import (MODE_FOLD, MODE_IP4HDR, MODE_L4_FILL, MODE_PARTIAL, MODE_VALIDATE, PKT_DTYPE, PKT_V6,
                               Device, set_pkt_off)

pytestmark = pytest.mark.gpu

GUARD = 24  # bytes of 0xEE behind every output
MODES = [MODE_FOLD, MODE_L4_FILL, MODE_VALIDATE, MODE_PARTIAL, MODE_IP4HDR]

# (name, kind for synth.build_frames or None for random bytes, len, csum_start, csum_offset, proto, flags)
SHAPES = [
    ("tcp4_1500", synth.KIND_TCP4, 1500, 20, 16, 6, 0),
    ("udp4_64", synth.KIND_UDP4, 64, 20, 6, 17, 0),
    ("tcp6_1500", synth.KIND_TCP6, 1500, 40, 16, 6, PKT_V6),
    ("udp6_100", synth.KIND_UDP6, 100, 40, 6, 17, PKT_V6),
    ("len0", None, 0, 20, 6, 17, 0),
    ("len1", None, 1, 20, 6, 17, 0),
    ("len19", None, 19, 20, 6, 17, 0),
    ("len39", None, 39, 20, 6, 17, 0),
    ("start_past_len", None, 30, 40, 6, 17, PKT_V6),
    ("ip4_options", None, 200, 24, 16, 6, 0),  # the address range is not merged into the summed range
    ("odd_start", None, 300, 21, 16, 6, 0),
    ("len65535", None, 65535, 20, 16, 6, 0),
]


def _oracle_takes(mode, shape):
    """The oracle's PARTIAL and IP4HDR follow the reference, which slices
    pkt[csum_start:] and writes the field: only descriptors it accepts."""
    _, _, ln, cs, co, _, _ = shape
    if mode == MODE_PARTIAL:
        return cs + co + 2 <= ln
    if mode == MODE_IP4HDR:
        return 12 <= cs <= ln
    return True


def _build(shapes, seed, aligns=None):
    """One arena holding the given shapes in order, each packet in its own
    slot (64 spare bytes behind it: the address slices of short packets are
    read from there), at the given or at scattered alignments."""
    rng = np.random.default_rng(seed)
    n = len(shapes)
    offs, at = [], 128
    for i, s in enumerate(shapes):
        a = aligns[i] if aligns is not None else int(rng.integers(0, 128))
        at = (at + 127) // 128 * 128 + a
        offs.append(at)
        at += s[2] + 64
    arena = rng.integers(0, 256, size=at + 256, dtype=np.uint8)
    pkts = np.zeros(n, dtype=PKT_DTYPE)
    set_pkt_off(pkts, np.array(offs, dtype=np.uint64))
    for i, (_, kind, ln, cs, co, proto, flags) in enumerate(shapes):
        if kind is not None:
            arena[offs[i]: offs[i] + ln] = synth.build_frames(np.array([kind]), ln, rng, valid=(i % 3 != 2))[0]
        pkts[i] = (pkts[i]["off_lo"], pkts[i]["off_hi"], proto, flags, ln, cs, co)
    ini = rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64)
    ini[::5] = 0
    return arena, pkts, ini


def _pairs(mode, seed):
    """Every ordered pair of the shapes the mode's oracle takes: packets 2 i
    and 2 i + 1 are the two rows of one wave."""
    ok = [s for s in SHAPES if _oracle_takes(mode, s)]
    return _build([s for a in ok for b in ok for s in (a, b)], seed)


def _check(device, mode, arena, pkts, ini=None, inplace=False, run=None):
    """Device-resident batch against the oracle: results, guard bytes, arena."""
    n = len(pkts)
    w = 1 if mode == MODE_VALIDATE else 2
    a_cpu = arena.copy()
    want = oracle.checksum_batch(mode, a_cpu, pkts, initial=ini, inplace=inplace)
    d_arena = torch.from_numpy(arena.copy()).cuda()
    d_pkts = torch.from_numpy(pkts.view(np.uint8).copy()).cuda()
    d_ini = torch.from_numpy(ini.view(np.uint8).copy()).cuda() if ini is not None else None
    out = torch.full((n * w + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    if run is None:
        device.checksum_batch(mode, d_arena, d_pkts, n, out, initial=d_ini, inplace=inplace)
    else:
        run(d_arena, d_pkts, n, out, d_ini)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    res = got[: n * w].view(want.dtype)
    bad = np.flatnonzero(res != want)
    assert len(bad) == 0, f"mode {mode}: {len(bad)} of {n} differ, first at {bad[:8]}"
    assert (got[n * w:] == 0xEE).all(), "bytes behind the output were written"
    assert np.array_equal(d_arena.cpu().numpy(), a_cpu), "arena differs"
    return want


def _device(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Device(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("mode", MODES)
def test_rows_of_one_wave_with_different_geometry(dev, mode):
    arena, pkts, ini = _pairs(mode, 100 + mode)
    if mode in (MODE_FOLD, MODE_L4_FILL, MODE_VALIDATE):
        assert len(pkts) == 288
    want = _check(dev, mode, arena, pkts, ini if mode == MODE_FOLD else None)
    if mode == MODE_VALIDATE:
        assert want.any() and not want.all()
    if mode == MODE_FOLD:
        _check(dev, mode, arena, pkts, None)
    if mode == MODE_L4_FILL:
        a2 = arena.copy()
        _check(dev, mode, a2, pkts, None, inplace=True)


@pytest.mark.parametrize("mode", [MODE_VALIDATE, MODE_FOLD, MODE_L4_FILL])
def test_equal_geometry_at_every_alignment(dev, mode):
    """Three lengths x 128 alignments, each packet once as the first and once
    as the second row of its wave, its neighbour of the same geometry."""
    shapes, aligns = [], []
    for kind, ln in ((None, 1), (synth.KIND_TCP4, 141), (synth.KIND_TCP4, 1500)):
        s = ("eq", kind, ln, 20, 16, 6, 0)
        run = [(s, a) for a in range(128)]
        for sh, a in run + [(s, 77)] + run + [(s, 3)]:  # the second copy sits one row further on
            shapes.append(sh)
            aligns.append(a)
    arena, pkts, ini = _build(shapes, 7, aligns)
    _check(dev, mode, arena, pkts, ini if mode == MODE_FOLD else None)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 17])
def test_batch_sizes(dev, n):
    arena, pkts, ini = _pairs(MODE_VALIDATE, 300 + n)
    for mode in (MODE_VALIDATE, MODE_L4_FILL, MODE_FOLD):
        for first in (0, 5):  # the batch starts on either kind of row
            _check(dev, mode, arena, pkts[first: first + n].copy(), ini[:n] if mode == MODE_FOLD else None)


def test_grid_stride_takes_prefetched_descriptors():
    """A second Device with one block per CU: 5,000 mixed 576-byte frames take
    several steps per wave, the later ones on prefetched descriptors."""
    d2 = _device(WGCS_BLOCKS_PER_CU="1")
    try:
        cap = d2.lib.wgcs_num_cu(d2.h) & ~7
        assert 5000 > cap * 8, "the batch must stride"
        arena, pkts, _ = synth.make_batch(5000, 576, kinds="mixed", seed=61, stride=579)
        pkts["len"][::11] = 1  # rows of other geometry among them
        rng = np.random.default_rng(3)
        ini = rng.integers(0, 2**64 - 1, size=5000, dtype=np.uint64)
        for mode in (MODE_VALIDATE, MODE_L4_FILL, MODE_FOLD):
            _check(d2, mode, arena, pkts, ini if mode == MODE_FOLD else None)
        _check(d2, MODE_VALIDATE, arena, pkts[:4999].copy())  # an odd count: the last wave's second row is idle
    finally:
        d2.close()


@pytest.mark.parametrize("equal", [True, False])
@pytest.mark.parametrize("mode", [MODE_VALIDATE, MODE_L4_FILL, MODE_FOLD])
def test_one_fused_call_of_three_batches(dev, mode, equal):
    w = 1 if mode == MODE_VALIDATE else 2
    hosts = [_pairs(mode, 500 + k) for k in range(3)]
    if not equal:  # 288, 17 and 139 packets: unequal block counts
        hosts[1] = tuple(x[:17].copy() if i else x for i, x in enumerate(hosts[1]))
        hosts[2] = tuple(x[5:144].copy() if i else x for i, x in enumerate(hosts[2]))
    devs, outs = [], []
    for arena, pkts, ini in hosts:
        devs.append((torch.from_numpy(arena).cuda(), torch.from_numpy(pkts.view(np.uint8).copy()).cuda(),
                     torch.from_numpy(ini.view(np.uint8).copy()).cuda()))
        outs.append(torch.full((len(pkts) * w + GUARD,), 0xEE, dtype=torch.uint8, device="cuda"))
    bl = dev.batch_list([(a, p, len(h[1]), o, i if mode == MODE_FOLD else None)
                         for (a, p, i), h, o in zip(devs, hosts, outs)])
    dev.checksum_batches(mode, bl, [torch.cuda.Stream(), torch.cuda.Stream()])
    torch.cuda.synchronize()
    for (arena, pkts, ini), (a, _, _), o in zip(hosts, devs, outs):
        n = len(pkts)
        a_cpu = arena.copy()
        want = oracle.checksum_batch(mode, a_cpu, pkts, initial=ini if mode == MODE_FOLD else None)
        got = o.cpu().numpy()
        assert np.array_equal(got[: n * w].view(want.dtype), want) and (got[n * w:] == 0xEE).all()
        assert np.array_equal(a.cpu().numpy(), a_cpu)


@pytest.mark.parametrize("lanes", ["16", "64"])
def test_lane_widths(lanes):
    d2 = _device(WGCS_LANES_PER_PKT=lanes)
    try:
        for mode in MODES:
            arena, pkts, ini = _pairs(mode, 100 + mode)
            _check(d2, mode, arena, pkts, ini if mode == MODE_FOLD else None)
    finally:
        d2.close()
