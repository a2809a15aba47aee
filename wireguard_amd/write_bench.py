"""Write-call builder measurement: the device-resident
wgcs_write_build_batch on one MI355X, the host path it replaces, and what the
fixed layout's empty call rows cost wgcs_handle_gro_batch.

  python -m wireguard_amd.write_bench [--steps 200 --warmup 20]

Workload: 512 receive batches of 128 rows per launch with 1, 4, 16 and 128
peers per batch (one key row per peer, every peer present in every batch, its
rows dealt at random), calls_per_batch = the peer count.  About 90 % of the
rows carry a packet of 1 to 1,420 bytes, the rest are keepalives, rejected
sources, replays and authentication failures.  One enqueue of K launches sits
between a HIP event pair on a stream of the bench's own, after W warmup
launches; every output of the first launch is compared with
wgcs_write_build_host first.

Per peer count the JSON line carries: us per builder launch, and the host path
measured in this process -- D2H of d_pkts and d_verdict, wgcs_write_build_host
on one core, H2D of the three tables.  `empty_gro` carries us per
wgcs_handle_gro_batch launch over 512 * calls_per_batch call rows that all
have n == 0, for calls_per_batch = 1, 8 and 128.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from . import _lib, writeplan
from .transport import AEAD_PKT_DTYPE
from .tun import GRO_BUF_DTYPE, GRO_CALL_DTYPE
from .writeplan import WRITE_GROUP_DTYPE

N_MSGS, OFFSET, CAP = 128, 16, 2048
TABLES = (("bufs", GRO_BUF_DTYPE), ("calls", GRO_CALL_DTYPE), ("groups", WRITE_GROUP_DTYPE))


def workload(n_batches, peers, rng):
    n = n_batches * N_MSGS
    pk = np.zeros(n, AEAD_PKT_DTYPE)
    pk["off"] = np.arange(n, dtype=np.uint64) * np.uint64(CAP)
    keys = np.stack([rng.permutation(N_MSGS) % peers for _ in range(n_batches)]).reshape(-1)
    u = rng.random(n)
    verdict = rng.integers(1, 1421, n).astype(np.int32)
    for lo, code in ((0.90, 0), (0.94, _lib.ERR_SOURCE), (0.96, _lib.ERR_REPLAY), (0.98, _lib.ERR_AUTH)):
        verdict[u >= lo] = code
    pk["key"] = keys
    pk["len"] = np.where(verdict > 0, verdict + 32, 32).astype(np.uint32)
    return pk, verdict, np.arange(1, peers + 1, dtype=np.uint32)


def timed(stream, e0, e1, warmup, steps, fn):
    import torch

    for _ in range(warmup):
        fn()
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, default=512)
    ap.add_argument("--peers", type=int, nargs="+", default=[1, 4, 16, 128])
    ap.add_argument("--empty-calls", type=int, nargs="+", default=[1, 8, 128])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0 or not 1 <= args.batches <= 1 << 21 or \
            not all(1 <= p <= N_MSGS for p in args.peers + args.empty_calls):
        ap.error("--steps >= 1, --warmup >= 0, 1 <= --batches <= 2^21, 1 <= --peers, --empty-calls <= 128")

    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("write_bench: no GPU (this measurement does not fall back)")
    torch.cuda.set_device(args.device)
    dev = Device(args.device)
    nb, n = args.batches, args.batches * N_MSGS
    stream = torch.cuda.Stream()  # the launches and torch's fills alike (see keystate_bench)
    torch.cuda.set_stream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def device_tables(cpb):
        rows = dict(bufs=n, calls=nb * cpb, groups=nb * cpb)
        t = {k: torch.zeros(rows[k] * dt.itemsize, dtype=torch.uint8, device="cuda") for k, dt in TABLES}
        t["n_groups"], t["status"] = (torch.zeros(nb, dtype=torch.int32, device="cuda") for _ in range(2))
        return t

    results = []
    for peers in args.peers:
        cpb = peers
        pk, verdict, key_peer = workload(nb, peers, np.random.default_rng(20261021 + peers))
        d_pk, d_verdict, d_kp = up(pk), up(verdict), up(key_peer)
        t = device_tables(cpb)

        def launch():
            writeplan.write_build_batch(dev, d_pk, d_verdict, N_MSGS, d_kp, OFFSET, CAP, cpb, t["bufs"], t["calls"],
                                        t["groups"], t["n_groups"], t["status"], stream=stream, n_batches=nb,
                                        n_keys=peers)

        # the host path: D2H of what the step reads, one core, H2D of the three tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_pk, h_verdict = d_pk.cpu().numpy().view(AEAD_PKT_DTYPE), d_verdict.cpu().numpy().view(np.int32)
        t1 = time.perf_counter()
        h = {k: np.zeros(t[k].numel() // dt.itemsize, dt) for k, dt in TABLES}
        h["n_groups"], h["status"] = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
        for a in h.values():
            a.view(np.uint8).fill(0)  # touch the pages
        t2 = time.perf_counter()
        writeplan.write_build_host(h_pk, h_verdict, N_MSGS, key_peer, OFFSET, CAP, cpb, h["bufs"], h["calls"],
                                   h["groups"], h["n_groups"], h["status"])
        t3 = time.perf_counter()
        for k, _ in TABLES:
            up(h[k])
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        launch()
        torch.cuda.synchronize()
        for k in h:
            assert t[k].cpu().numpy().tobytes() == h[k].tobytes(), f"{k} != wgcs_write_build_host"
        assert (h["status"] == 0).all() and h["n_groups"].max() == peers
        us = timed(stream, e0, e1, args.warmup, args.steps, launch)
        results.append(dict(peers=peers, calls_per_batch=cpb, kept_rows=int((h["calls"]["n"]).sum()),
                            empty_calls=int((h["calls"]["n"] == 0).sum()), us_per_launch=round(us, 2),
                            mrows_per_s=round(n / us, 1), host_d2h_us=round((t1 - t0) * 1e6, 1),
                            host_one_core_us=round((t3 - t2) * 1e6, 1), host_h2d_us=round((t4 - t3) * 1e6, 1),
                            host_path_us=round((t1 - t0 + t3 - t2 + t4 - t3) * 1e6, 1)))

    # the price of the fixed layout's empty rows: handle_gro over calls that all have n == 0
    empty = []
    pk, _, key_peer = workload(nb, 1, np.random.default_rng(1))
    d_pk, d_kp = up(pk), up(key_peer)
    d_verdict = torch.full((n,), _lib.ERR_REPLAY, dtype=torch.int32, device="cuda")
    d_arena = torch.zeros(4096, dtype=torch.uint8, device="cuda")  # no call reads it
    for cpb in args.empty_calls:
        t = device_tables(cpb)
        writeplan.write_build_batch(dev, d_pk, d_verdict, N_MSGS, d_kp, OFFSET, CAP, cpb, t["bufs"], t["calls"],
                                    t["groups"], t["n_groups"], t["status"], stream=stream, n_batches=nb, n_keys=1)
        st, nw = (torch.full((nb * cpb,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        tw = torch.full((n,), -7, dtype=torch.int32, device="cuda")

        def gro():
            dev.handle_gro_batch(d_arena, t["bufs"], t["calls"], nb * cpb, st, nw, tw, stream=stream)

        gro()
        torch.cuda.synchronize()
        assert not t["n_groups"].any() and not st.any() and not nw.any() and bool((tw == -7).all())
        us = timed(stream, e0, e1, args.warmup, args.steps, gro)
        empty.append(dict(calls_per_batch=cpb, calls=nb * cpb, us_per_launch=round(us, 2)))
    print(json.dumps({"metric": "write_build_us", "unit": "us/launch", "steps": args.steps, "warmup": args.warmup,
                      "workload": {"batches": nb, "rows": n}, "peers": results, "empty_gro": empty}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
