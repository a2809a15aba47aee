"""Peer-lookup measurement: the
device-resident wgcs_route_dst_batch / wgcs_recv_classify_batch /
wgcs_recv_source_batch on one MI355X.

  python -m wireguard_amd.route_bench --mode dst|classify|source [--steps 200 --warmup 20]

Workload: 65,536 packets of 1,420 B per launch, laid out as the kernel before
this one leaves them -- dst: GSO-split slots of 1,440 B with the packet 16 bytes
in; classify and source: 1,452-B transport messages in slots of 1,456 B -- and
one table per --tables entry (16, 1,024 and 16,384): that many allowed-IPs
prefixes (three quarters IPv4 /12../32, one quarter IPv6 /32../128, one peer
per four prefixes) for dst and source, that many sessions (in twice as many
slots, rounded up to a power of two) for classify.  Nine packets in ten carry
an address inside a random prefix of the table (a receiver index of the table),
the rest a random one.  The arena exists in 4 copies that the launches rotate
over.  A kernel reads one or two 128-B lines of each packet and writes 4 to 28
bytes per packet, so the byte counts are small and the figure of merit is time
per launch and packets per second, not bandwidth.  One enqueue of K launches
sits between a HIP event pair, after W warmup launches; every result is
compared with the host router (wgcs_router_find) or a dict first.

Prints one JSON line: per table, us per launch and packets per second, and as
context one CPU core calling wgcs_router_find once per address through ctypes
(call overhead included).
"""
from __future__ import annotations

import argparse
import json
import struct
import time

import numpy as np

from . import router
from .router import PEER_NONE
from .transport import AEAD_PKT_DTYPE

PKT = 1420
MSG = 16 + PKT + 16
DST_STRIDE, MSG_STRIDE = 1440, 1456
COPIES = 4


def make_router(n_prefixes: int, rng):
    """(Router, [(addr bytes, cidr, peer)])."""
    r, out, seen = router.Router(), [], set()
    while len(out) < n_prefixes:
        if len(out) % 4 != 3:
            addr, cidr = bytes([10 + len(out) % 3]) + rng.bytes(3), int(rng.integers(12, 33))
        else:
            addr, cidr = b"\x20\x01\x0d\xb8" + rng.bytes(12), int(rng.integers(32, 129))
        bits = 8 * len(addr)
        masked = (int.from_bytes(addr, "big") >> (bits - cidr) << (bits - cidr)).to_bytes(len(addr), "big")
        if (masked, cidr) in seen:
            continue
        seen.add((masked, cidr))
        peer = len(out) // 4
        r.insert(masked, cidr, peer)
        out.append((masked, cidr, peer))
    return r, out


def addresses(prefixes, n: int, rng):
    """n addresses: nine in ten inside a random prefix, the rest random."""
    out = []
    pick = rng.integers(0, len(prefixes), n)
    for i in range(n):
        addr, cidr, _ = prefixes[pick[i]]
        bits = 8 * len(addr)
        if i % 10 == 9:
            out.append(rng.bytes(len(addr)))
        else:
            host = int.from_bytes(rng.bytes(len(addr)), "big") & ((1 << (bits - cidr)) - 1)
            out.append((int.from_bytes(addr, "big") | host).to_bytes(len(addr), "big"))
    return out


def cpu_find(r, addrs):
    """(peers by wgcs_router_find, seconds): one core, one ctypes call per address."""
    find, h = r.lib.wgcs_router_find, r.h
    t0 = time.perf_counter()
    peers = [find(h, a, len(a)) for a in addrs]
    return peers, time.perf_counter() - t0


def fill_packets(arena, stride, at, addrs, field4, field6):
    """An IP header at slot * stride + at of every slot, the address in its source or destination field."""
    a = arena.reshape(-1, stride)
    for i, addr in enumerate(addrs):
        if len(addr) == 4:
            a[i, at] = 0x45
            a[i, at + 2:at + 4] = (PKT >> 8, PKT & 0xFF)
            a[i, at + field4:at + field4 + 4] = np.frombuffer(addr, np.uint8)
        else:
            a[i, at] = 0x60
            a[i, at + 4:at + 6] = ((PKT - 40) >> 8, (PKT - 40) & 0xFF)
            a[i, at + field6:at + field6 + 16] = np.frombuffer(addr, np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("dst", "classify", "source"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--packets", type=int, default=65536)
    ap.add_argument("--tables", type=int, nargs="+", default=[16, 1024, 16384])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0 or args.packets < 1 or min(args.tables) < 1:
        ap.error("--steps >= 1, --warmup >= 0, --packets >= 1, --tables >= 1")

    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("route_bench: no GPU (this measurement does not fall back)")
    torch.cuda.set_device(args.device)
    dev = Device(args.device)
    n = args.packets
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    results = []
    for size in args.tables:
        rng = np.random.default_rng(20261019 + size)
        stride = DST_STRIDE if args.mode == "dst" else MSG_STRIDE
        arena = rng.integers(0, 256, n * stride, dtype=np.uint8)
        rec = {"table": size}
        if args.mode == "classify":
            idx = np.unique(rng.integers(0, 2**32, 2 * size, dtype=np.uint64).astype(np.uint32))[:size]
            idx = rng.permutation(idx)
            sessions = dict(zip(idx.tolist(), range(len(idx))))
            slots = router.session_table(idx, np.arange(len(idx), dtype=np.uint32))
            receivers = np.where(np.arange(n) % 10 == 9, rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32),
                                 idx[rng.integers(0, len(idx), n)])
            a = arena.reshape(n, stride)
            a[:, 0:4] = np.frombuffer(struct.pack("<I", 4), np.uint8)
            a[:, 4:8] = receivers.astype("<u4").view(np.uint8).reshape(n, 4)
            want_key = np.array([sessions.get(int(x), 0xFFFFFFFF) for x in receivers], np.uint32)
            d_sizes = torch.full((n,), MSG, dtype=torch.int32, device="cuda")
            d_slots = torch.from_numpy(slots.view(np.uint8).reshape(-1)).cuda()
            d_pkts = torch.zeros(n * AEAD_PKT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_type = torch.zeros(n, dtype=torch.int32, device="cuda")
            rec.update(sessions=len(idx), slots=len(slots), listed_share=round(float((want_key != 0xFFFFFFFF).mean()), 3))

            def launch(buf):
                router.classify_batch(dev, buf, d_sizes, d_slots, d_pkts, d_type, stride=stride, stream=stream, n=n,
                                      n_slots=len(slots))

            def check():
                pk = d_pkts.cpu().numpy().view(AEAD_PKT_DTYPE)
                assert np.array_equal(pk["key"], want_key), "classify keys != dict"
                assert np.array_equal(d_type.cpu().numpy(), np.where(want_key != 0xFFFFFFFF, 4, 0)), "classify types"
                assert np.array_equal(pk["off"], np.arange(n, dtype=np.uint64) * np.uint64(stride)) and (pk["len"] == MSG).all()
        else:
            r, prefixes = make_router(size, rng)
            addrs = addresses(prefixes, n, rng)
            want, cpu_s = cpu_find(r, addrs)
            want = np.array(want, np.uint32)
            image = r.image()
            d_image = torch.from_numpy(image).cuda()
            rec.update(prefixes=size, image_bytes=len(image), routed_share=round(float((want != PEER_NONE).mean()), 3),
                       cpu_one_core_find_mpps=round(n / cpu_s / 1e6, 3))
            d_peer = torch.zeros(n, dtype=torch.int32, device="cuda")
            if args.mode == "dst":
                fill_packets(arena, stride, 16, addrs, 16, 24)
                d_sizes = torch.full((n,), PKT, dtype=torch.int32, device="cuda")

                def launch(buf):
                    router.route_dst_batch(dev, buf, d_sizes, d_image, d_peer, stride=stride, offset=16, stream=stream, n=n,
                                           image_bytes=len(image))

                def check():
                    assert np.array_equal(d_peer.cpu().numpy().view(np.uint32), want), "route_dst != wgcs_router_find"
            else:
                fill_packets(arena, stride, 16, addrs, 12, 8)
                n_keys = max(p[2] for p in prefixes) + 1  # key k is peer k's
                pk = np.zeros(n, AEAD_PKT_DTYPE)
                pk["off"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
                pk["len"] = MSG
                pk["key"] = np.where(want != PEER_NONE, want, 0)
                pk["key"][::16] = (pk["key"][::16] + 1) % n_keys  # one in 16 from another peer's session
                key_peer = np.arange(n_keys, dtype=np.uint32)
                want_v = np.where(want == key_peer[pk["key"]], PKT, -19).astype(np.int32)
                d_pk = torch.from_numpy(pk.view(np.uint8).reshape(-1)).cuda()
                d_len = torch.full((n,), PKT, dtype=torch.int32, device="cuda")
                d_key_peer = torch.from_numpy(key_peer.view(np.uint8)).cuda()
                d_verdict = torch.zeros(n, dtype=torch.int32, device="cuda")
                rec.update(allowed_share=round(float((want_v > 0).mean()), 3))

                def launch(buf):
                    router.source_batch(dev, buf, d_pk, d_len, d_key_peer, d_image, d_verdict, peer=d_peer, stream=stream,
                                        n=n, n_keys=n_keys, image_bytes=len(image))

                def check():
                    assert np.array_equal(d_peer.cpu().numpy().view(np.uint32), want), "source peers != wgcs_router_find"
                    assert np.array_equal(d_verdict.cpu().numpy(), want_v), "source verdicts"
        first = torch.from_numpy(arena).cuda()
        copies = [first] + [first.clone() for _ in range(COPIES - 1)]
        launch(copies[0])
        torch.cuda.synchronize()
        check()
        for k in range(args.warmup):
            launch(copies[k % COPIES])
        e0.record(stream)
        for k in range(args.steps):
            launch(copies[(args.warmup + k) % COPIES])
        e1.record(stream)
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.steps
        check()
        rec.update(us_per_launch=round(us, 2), mpps=round(n / us, 1))
        results.append(rec)
        del copies, first
    kernel = {"dst": "route_dst_kernel", "classify": "recv_classify_kernel", "source": "recv_source_kernel"}[args.mode]
    print(json.dumps({"metric": f"route_{args.mode}_mpps", "unit": "Mpackets/s", "kernel": kernel, "steps": args.steps,
                      "warmup": args.warmup,
                      "workload": {"packets": n, "packet_bytes": PKT, "slot_stride": stride, "arena_copies": COPIES},
                      "tables": results}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
