"""Peer endpoint measurement: wgcs_endpoint_recv_batch,
wgcs_endpoint_set_received_batch, wgcs_endpoint_dst_jobs_batch and the receive
chain with the recv call in it, on one MI355X, each beside its comparison in
the same process, alternating.  Not part of bench.py.

  python -m wireguard_amd.endpoint_bench --mode recv|set|dst|chain [--steps 200 --warmup 10]

  recv  65,536 and 1,024 slots, every slot with an IP_PKTINFO control message
        behind a UDP_GRO one, beside a plain device copy of the same 64-byte rows.
  set   wgcs_endpoint_set_received_batch over 65,536 and 1,024 group rows, over
        1,024 peers and over one peer (every row then claims one row of the
        table), beside wgcs_timers_received_batch over the same groups.
  dst   wgcs_endpoint_dst_jobs_batch over 65,536 and 1,024 jobs of one segment,
        1,024 peers and one peer, beside wgcs_timers_sent_batch over the same jobs.
        Half the peers' WGCS_TIMERS_CLEAR_SRC flags are set again in front of every
        timed call by a stream-ordered copy of the two tables (timed alone too), so
        every call takes the clear path.
  chain split -> endpoint_recv -> classify -> screen under load on one stream,
        65,536 and 1,024 slots (batches of 128 slots, two UDP-GRO messages of 64
        initiations each), beside split -> synchronise -> read d_src -> gather the
        addresses on the host -> upload -> classify -> screen.  Wall clock around K
        calls and a final synchronise: the host's part is what is compared.
The device's outputs and tables are compared with the host forms' before
anything is timed.  Prints one JSON line per row count and variant.
"""
from __future__ import annotations

import argparse
import json
import struct

import numpy as np

from . import endpoint as ep, timers
from .cookie import SRC_ADDR_DTYPE
from .writeplan import WRITE_GROUP_DTYPE

NOW = 1_000_000_000_000
OOB_STRIDE = 64


def _cmsg(level: int, typ: int, data: bytes) -> bytes:
    body = struct.pack("<Qii", 16 + len(data), level, typ) + data
    return body + bytes(-len(body) % 8)


CONTROL = _cmsg(17, 104, struct.pack("<H", 1400)) + _cmsg(0, 8, struct.pack("<i4s4s", 2, bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])))


def peer_table(n_peers: int):
    tab, claim = ep.table(n_peers)
    for r in range(n_peers):
        tab[r] = ep.row(bytes([10, 1, r >> 8, r & 255]), 51820, CONTROL[24:])[0]
    return tab, claim


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("recv", "set", "dst", "chain"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("endpoint_bench: no GPU (this measurement does not fall back)")
    dev = Device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def events(fn):
        for _ in range(args.warmup):
            fn()
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.steps * 1e3, 2)

    def med(rounds, i):
        return float(np.median([r[i] for r in rounds]))

    base = {"steps": args.steps, "warmup": args.warmup}
    timing = "HIP events around K calls, three rounds, the variants alternating in one process"
    P = 1024

    if args.mode == "chain":
        import time

        from . import cookie, router
        from .cookie_bench import make_batch

        ck, _, _, _, _, msgs = make_batch(64)
        dgram = np.frombuffer(b"".join(msgs), np.uint8)  # one UDP-GRO message: 64 initiations of 148 bytes
        n_msgs, first, out_stride = 128, 126, 160
        in_stride = len(dgram)
        slots = router.session_table(np.array([1], np.uint32), np.array([0], np.uint32))
        for n in (65536, 1024):
            nb = n // n_msgs
            rng = np.random.default_rng(n)
            land = np.tile(dgram, nb * (n_msgs - first))
            n_in, gso = np.zeros((nb, n_msgs), np.int32), np.zeros((nb, n_msgs), np.int32)
            n_in[:, first:], gso[:, first:] = len(dgram), 148
            addr = np.zeros((nb, n_msgs), SRC_ADDR_DTYPE)
            addr["b"][:, first, :6], addr["len"][:, first] = rng.integers(0, 256, (nb, 6), dtype=np.uint8), 6
            addr["b"][:, first + 1], addr["len"][:, first + 1] = rng.integers(0, 256, (nb, 18), dtype=np.uint8), 18
            oob, nn = np.zeros((n, OOB_STRIDE), np.uint8), np.zeros((nb, n_msgs), np.int32)
            oob.reshape(nb, n_msgs, OOB_STRIDE)[:, first:, :len(CONTROL)] = np.frombuffer(CONTROL, np.uint8)
            nn[:, first:] = len(CONTROL)
            d_land, d_n_in, d_gso, d_addr, d_oob, d_nn = (up(x) for x in (land, n_in, gso, addr, oob, nn))
            d_slots, d_ck, d_nonce = up(slots), up(ck), up(rng.integers(0, 256, 24 * n, dtype=np.uint8))
            u8 = lambda m: torch.zeros(m, dtype=torch.uint8, device="cuda")  # noqa: E731
            i32 = lambda m: torch.zeros(m, dtype=torch.int32, device="cuda")  # noqa: E731
            d_arena, d_n_out, d_from, d_count, d_status = u8(n * out_stride), i32(n), i32(n), i32(nb), i32(nb)
            d_ep, d_addr_out, d_src = u8(64 * n), u8(20 * n), u8(20 * n)
            d_pkts, d_type = u8(24 * n), i32(n)
            out = [(i32(n), u8(64 * n)) for _ in range(2)]  # verdicts and replies of the two chains
            base_slot = np.repeat(np.arange(nb) * n_msgs, n_msgs)
            flat = addr.reshape(-1)

            def split():
                dev._check(dev.lib.wgcs_split_messages_batch(
                    dev.h, d_land.data_ptr(), in_stride, in_stride, d_n_in.data_ptr(), d_gso.data_ptr(), n_msgs, first, nb,
                    d_arena.data_ptr(), out_stride, d_n_out.data_ptr(), d_from.data_ptr(), d_count.data_ptr(),
                    d_status.data_ptr(), stream.cuda_stream))

            def screen(d_srcs, o):
                router.classify_batch(dev, d_arena, d_n_out, d_slots, d_pkts, d_type, stride=out_stride, stream=stream, n=n,
                                      n_slots=len(slots))
                cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_ck, d_srcs, o[0], under_load=True, nonce=d_nonce,
                                    reply=o[1], stream=stream, n=n)

            def chain():
                split()
                ep.recv_batch(dev, d_addr, d_from, d_n_out, d_oob, OOB_STRIDE, d_nn, n_msgs, nb, d_ep, d_addr_out, stream=stream)
                screen(d_addr_out, out[0])

            def host_chain():
                split()
                frm = d_from.cpu().numpy()  # synchronises
                src = flat[np.where(frm >= 0, base_slot + frm, np.arange(n))]
                d_src.copy_(torch.from_numpy(src.view(np.uint8).reshape(-1)), non_blocking=True)
                screen(d_src, out[1])

            def wall(fn):
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                return round((time.perf_counter() - t0) / args.steps * 1e6, 2)

            chain(), host_chain()
            torch.cuda.synchronize()
            assert d_count.cpu().tolist() == [n_msgs] * nb and not bool(d_status.any())
            assert bool((out[0][0] == cookie.HS_COOKIE).all()), "every row is an initiation without MAC2 under load"
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), "the two chains differ"
            rounds = [(wall(chain), wall(host_chain)) for _ in range(3)]
            print(json.dumps({**base, "metric": "endpoint_chain_us", "unit": "us", "rows": n, "value": med(rounds, 0),
                              "chain_us": [r[0] for r in rounds], "read_back_chain_us": [r[1] for r in rounds],
                              "chain": "split, endpoint_recv, classify, screen under load; enqueued back to back",
                              "read_back_chain": "split, synchronise, read d_src, gather on the host, upload, classify, screen",
                              "timing": "wall clock around K calls and a final synchronise, three rounds, alternating"}),
                  flush=True)
        return

    if args.mode == "recv":
        for n in (65536, 1024):
            addr = np.zeros(n, SRC_ADDR_DTYPE)
            addr["b"][:, :6] = np.frombuffer(bytes([203, 0, 113, 5, 0x41, 0x9C]), np.uint8)
            addr["len"] = 6
            size, nn = np.full(n, 148, np.int32), np.full(n, len(CONTROL), np.int32)
            oob = np.zeros((n, OOB_STRIDE), np.uint8)
            oob[:, :len(CONTROL)] = np.frombuffer(CONTROL, np.uint8)
            want, want_addr = ep.recv_host(addr, None, size, oob, OOB_STRIDE, nn, 128, n // 128)
            d = [up(x) for x in (addr, size, oob, nn)]
            d_ep, d_out = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
            d_copy = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")

            def recv():
                ep.recv_batch(dev, d[0], None, d[1], d[2], OOB_STRIDE, d[3], 128, n // 128, d_ep, d_out, stream=stream)

            def copy():
                d_copy.copy_(d_ep)

            recv()
            torch.cuda.synchronize()
            assert d_ep.cpu().numpy().tobytes() == want.tobytes() and d_out.cpu().numpy().tobytes() == want_addr.tobytes()
            rounds = [(events(recv), events(copy)) for _ in range(3)]
            print(json.dumps({**base, "metric": "endpoint_recv_us", "unit": "us", "rows": n, "value": med(rounds, 0),
                              "recv_us": [r[0] for r in rounds], "plain_copy_us_same_rows": [r[1] for r in rounds],
                              "kernel": "each_kernel<EndpointRecv>", "timing": timing}), flush=True)
        return

    for n in (65536, 1024):
        for variant, distinct in (("1024_peers", P), ("one_peer", 1)):
            tab, claim = peer_table(P)
            tm = timers.timers_table(P, 25)
            peer_rows = np.arange(P, dtype=np.uint32)
            d_rows = up(peer_rows)
            if args.mode == "set":
                eps = np.tile(tab, n // P)
                groups = np.zeros(n, WRITE_GROUP_DTYPE)
                groups["peer"], groups["tail"], groups["n_valid"] = np.arange(n) % distinct, np.arange(n), 1
                d_groups, d_eps = up(groups), up(eps)
                d_tab, d_claim, d_tm, d_tm2 = up(tab), up(claim), up(tm), up(tm)
                ep.set_received_host(groups, 128, eps, peer_rows, tab, claim, tm)

                def ours():
                    ep.set_received_batch(dev, d_groups, 128, d_eps, d_rows, d_tab, d_claim, d_tm, stream=stream,
                                          n_batches=n // 128, n_rows=n, n_ids=P, n_peers=P)

                def beside():
                    timers.received_batch(dev, d_groups, 128, NOW, d_rows, d_tm2, stream=stream, n_batches=n // 128, n_ids=P,
                                          n_peers=P)

                ours()
                torch.cuda.synchronize()
                assert d_tab.cpu().numpy().tobytes() == tab.tobytes() and not bool(d_claim.any())
                names = ("endpoint_set_received_us", "timers_received_us_same_groups",
                         "each_kernel<EndpointSetClaim<GroupRows>> + each_kernel<EndpointSetCommit<GroupRows>>")
            else:
                tm["flags"][::2] |= ep.TIMERS_CLEAR_SRC
                peer = (np.arange(n) % distinct).astype(np.uint32)
                count, status, key = np.ones(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
                lens, sizes = np.full(n, 1452, np.int32), np.full(n, 1420, np.int32)
                d_in = [up(x) for x in (peer, count, status, key, lens, sizes)]
                d_tab, d_tm, d_tm2, d_nbufs = up(tab), up(tm), up(tm), up(count)
                d_tab0, d_tm0 = up(tab), up(tm)  # the tables with the flags set, as every timed call finds them
                d_dst = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
                d_v6, d_ds = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
                d_tx = torch.zeros(n, dtype=torch.int64, device="cuda")
                nbufs = count.copy()
                want = ep.dst_jobs_host(peer, count, status, key, 1, lens, nbufs, peer_rows, tab, tm)

                def rearm():
                    d_tab.copy_(d_tab0), d_tm.copy_(d_tm0)

                def ours():
                    rearm()
                    ep.dst_jobs_batch(dev, d_in[0], d_in[1], d_in[2], d_in[3], 1, d_in[4], d_nbufs, d_rows, d_tab, d_tm, d_dst,
                                      d_v6, d_ds, d_tx, stream=stream, n_jobs=n, n_ids=P, n_peers=P)

                def beside():
                    timers.sent_batch(dev, d_in[5], d_in[0], d_in[1], d_in[2], d_in[3], 1, NOW, 7, d_rows, d_tm2, stream=stream,
                                      n_jobs=n, n_ids=P, n_peers=P)

                ours()
                torch.cuda.synchronize()
                assert d_dst.cpu().numpy().tobytes() == want[0].tobytes() and d_tab.cpu().numpy().tobytes() == tab.tobytes()
                assert d_tx.cpu().numpy().view(np.uint64).tolist() == want[3].tolist()
                names = ("endpoint_dst_jobs_us", "timers_sent_us_same_jobs",
                         "each_kernel<EndpointDstJobs> + each_kernel<EndpointDstClear<KeptJobRows>>")
            if args.mode == "dst":
                rounds = [(events(ours), events(beside), events(rearm)) for _ in range(3)]
                more = {"includes_rearm_us": [r[2] for r in rounds],
                        "rearm": "two stream-ordered table copies in front of every timed call: half the peers' flags set"}
            else:
                rounds, more = [(events(ours), events(beside)) for _ in range(3)], {}
            print(json.dumps({**base, "metric": names[0], "unit": "us", "rows": n, "peers": P, "variant": variant,
                              "value": med(rounds, 0), names[0]: [r[0] for r in rounds], names[1]: [r[1] for r in rounds],
                              **more, "kernel": names[2], "timing": timing}), flush=True)


if __name__ == "__main__":
    main()
