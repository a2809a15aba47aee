"""Keypair rotation measurement: the device-resident
wgcs_keypairs_begin_responder_batch and wgcs_keypairs_received_batch on one
MI355X, beside wgcs_replay_batch over the same rows and beside the way through
one host core.  Not part of bench.py.

  python -m wireguard_amd.keypairs_bench --mode begin|received|chain
                                         [--rows 65536 --peers 1024 --steps 20 --warmup 3]

Workload: `peers` peers, each with a current keypair it is the responder of
(key rows 4r, 4r + 1), every receiver index and peer id registered ahead.
  received  `rows` packets (and then 1,024) spread evenly over the peers'
            current receive keys, all past the filter.  Two variants: "none",
            no peer has a next keypair (the steady state of the per-packet
            path), and "one_per_peer", every peer has a next keypair (rows
            4r + 2, 4r + 3) and one packet under it at a random row, so every
            peer rotates.  That variant commits, so device copies restore the
            five tables before every call, inside the timed window; the restore
            is timed alone as well.  "none" writes only d_rotated and restores
            nothing.
            wgcs_replay_batch over the same rows is timed in the same process
            in alternating runs (an elementwise add moves the counters on
            before each call, so no launch sees a replay).
  begin     `rows` (default 1,024 for this mode) responder descriptors, one
            per peer in turn, each a fresh index and two fresh key rows,
            against tables restored before every call.
  chain     replay -> received -> send-assign (one job per peer) on one stream,
            both variants, and beside it the way through one host core from
            the parent's interfaces: replay, synchronise, read the verdicts
            back, ReceivedWithNewKeypair on the host
            (wgcs_keypairs_received_host), and where a peer rotated rebuild
            both slot tables (wgcs_session_table_build) and upload them, then
            send-assign.  Timed by a host clock around one call that ends in
            a synchronise, the two ways alternating.
The device's tables are compared with the host form's before anything is
timed.  Prints one JSON line per batch size and variant.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from . import keypairs, keystate, noise, router
from .keypairs import SESSION_NO_KEYPAIR
from .noise import HS_RESP_DTYPE, PEER_KEY_DTYPE
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

NOW = 1_700_000_000_000_000_000
TABLES = ("kp", "slots", "peer_keys", "keys", "key_peer")


def make_world(n_peers: int, with_next: bool, extra_indices: int = 0, seed: int = 20261026):
    """The tables after every peer's first session (and, with_next, a second handshake it responded to)."""
    rng = np.random.default_rng(seed)
    table = np.zeros(n_peers, PEER_KEY_DTYPE)
    table["public_key"] = rng.integers(0, 256, (n_peers, 32), dtype=np.uint8)
    table["peer"] = np.arange(n_peers, dtype=np.uint32)
    peer_rows = noise.peer_rows_build(table, n_peers)
    idx = (rng.choice(1 << 30, 2 * n_peers + extra_indices, replace=False) + 1).astype(np.uint32)
    n_keys = 4 * n_peers + 2 * extra_indices
    t = dict(kp=keypairs.keypairs_table(n_peers),
             slots=router.session_table(idx, np.full(len(idx), SESSION_NO_KEYPAIR, np.uint32)),
             peer_keys=router.session_table(table["peer"], np.full(n_peers, SESSION_NO_KEYPAIR, np.uint32)),
             keys=np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy(), key_peer=np.full(n_keys, 0xFFFFFFFF, np.uint32))
    r = np.arange(n_peers, dtype=np.uint32)

    def begin(indices, send):
        resp = np.zeros(n_peers, HS_RESP_DTYPE)
        resp["peer_row"], resp["local_index"], resp["send_key"], resp["recv_key"] = r, indices, send, send + 1
        status = np.zeros(n_peers, np.int32)
        keypairs.begin_responder_host(resp, np.full(n_peers, noise.HS_RESPONDED, np.int32), NOW, table, t["kp"], t["slots"],
                                      t["peer_keys"], t["keys"], t["key_peer"], status)
        assert (status == keypairs.HS_BEGUN).all()

    begin(idx[:n_peers], 4 * r)
    first = np.zeros(n_peers, AEAD_PKT_DTYPE)
    first["key"] = 4 * r + 1
    rotated = np.zeros(n_peers, np.uint32)
    keypairs.received_host(first, np.full(n_peers, 100, np.int32), t["key_peer"], peer_rows, t["kp"], t["slots"],
                           t["peer_keys"], t["keys"], rotated)
    assert rotated.all()
    if with_next:
        begin(idx[n_peers:2 * n_peers], 4 * r + 2)
    return table, peer_rows, t, idx, n_keys


def make_rows(n: int, n_peers: int, with_next: bool, seed: int = 20261027):
    rng = np.random.default_rng(seed)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    pkts["key"] = 4 * (np.arange(n, dtype=np.uint32) % n_peers) + 1
    if with_next:
        who = np.arange(min(n, n_peers), dtype=np.uint32)
        pkts["key"][rng.choice(n, len(who), replace=False)] = 4 * who + 3
    pkts["len"] = 132
    return pkts, np.full(n, 100, np.int32), np.arange(n, dtype=np.uint64) // n_peers


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("begin", "received", "chain"), required=True)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--peers", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    from .tun import Device

    dev = Device(0)
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def events(fn):
        for _ in range(args.warmup):
            fn()
        e0.record(stream)
        for _ in range(args.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.steps * 1e3, 2)

    def wall(fn):
        out = []
        for k in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e6)
        return round(float(np.median(out)), 2), round(min(out), 2)

    P = args.peers
    if args.mode == "begin":
        n = args.rows or 1024
        table, peer_rows, t, idx, n_keys = make_world(P, False, extra_indices=n)
        resp = np.zeros(n, HS_RESP_DTYPE)
        q = np.arange(n, dtype=np.uint32)
        resp["peer_row"], resp["local_index"] = q % P, idx[2 * P:]
        resp["send_key"], resp["recv_key"] = 4 * P + 2 * q, 4 * P + 2 * q + 1
        gate = np.full(n, noise.HS_RESPONDED, np.int32)
        d0 = {k: up(v) for k, v in t.items()}
        d = {k: v.clone() for k, v in d0.items()}
        d_resp, d_gate, d_table = up(resp), up(gate), up(table)
        d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_work = torch.zeros(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")

        def restore():
            for k in TABLES:
                d[k].copy_(d0[k])

        def call():
            restore()
            keypairs.begin_responder_batch(dev, d_resp, d_gate, NOW + 1, d_table, d["kp"], d["slots"], d["peer_keys"],
                                           d["keys"], d["key_peer"], d_status, d_work, stream=stream, n=n, n_peers=P,
                                           n_slots=len(t["slots"]), n_peer_slots=len(t["peer_keys"]), n_keys=n_keys)

        h = {k: v.copy() for k, v in t.items()}
        h_status = np.zeros(n, np.int32)
        t0 = time.perf_counter()
        keypairs.begin_responder_host(resp, gate, NOW + 1, table, h["kp"], h["slots"], h["peer_keys"], h["keys"],
                                      h["key_peer"], h_status)
        host_us = (time.perf_counter() - t0) * 1e6
        call()
        torch.cuda.synchronize()
        assert np.array_equal(d_status.cpu().numpy(), h_status) and (h_status == keypairs.HS_BEGUN).all()
        for k in TABLES:
            assert d[k].cpu().numpy().tobytes() == h[k].tobytes(), f"device {k} != host form"
        us, restore_us = events(call), events(restore)
        print(json.dumps({
            "metric": "keypairs_begin_descriptors_per_s", "value": round(n / (us * 1e-6)), "unit": "descriptors/s",
            "us_per_call": us, "table_restore_us": restore_us, "steps": args.steps, "warmup": args.warmup,
            "kernel": "kp_begin_resp_keys_kernel + key order (radix sort, heads) + kp_begin_resp_groups_kernel",
            "timing": "HIP events around K calls; each call is five device copies that restore the tables, then the call",
            "workload": {"descriptors": n, "peers": P, "per_peer": round(n / P, 2), "n_keys": n_keys, "n_slots": len(t["slots"])},
            "host_one_core": {"us_per_batch": round(host_us, 2), "path": "wgcs_keypairs_begin_responder_host, one ctypes call"},
        }), flush=True)
        return

    for n in dict.fromkeys((args.rows or 65536, min(args.rows or 65536, 1024))):
        for variant in ("none", "one_per_peer"):
            with_next = variant == "one_per_peer"
            table, peer_rows, t, idx, n_keys = make_world(P, with_next)
            pkts, pkt_len, counter = make_rows(n, P, with_next)
            d0 = {k: up(v) for k, v in t.items()}
            d = {k: v.clone() for k, v in d0.items()}
            d_pkts, d_len, d_rows = up(pkts), up(pkt_len), up(peer_rows)
            d_counter = torch.from_numpy(counter.view(np.int64)).cuda()
            d_filters = torch.zeros(keystate.REPLAY_FILTER_DTYPE.itemsize * n_keys, dtype=torch.uint8, device="cuda")
            d_verdict = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_rotated = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_work = torch.zeros(keystate.work_bytes(max(n, P)), dtype=torch.uint8, device="cuda")
            sizes = dict(n_keys=n_keys, n_ids=P, n_peers=P, n_slots=len(t["slots"]), n_peer_slots=len(t["peer_keys"]))
            step = (n + P - 1) // P

            def restore():  # a call without a candidate commits nothing: only the rotating variant restores
                if with_next:
                    for k in TABLES:
                        d[k].copy_(d0[k])

            def replay():
                d_counter.add_(step)
                keystate.replay_batch(dev, d_pkts, d_len, d_counter, d_filters, d_verdict, d_work, stream=stream, n=n,
                                      n_keys=n_keys)

            def received():
                keypairs.received_batch(dev, d_pkts, d_verdict, d["key_peer"], d_rows, d["kp"], d["slots"], d["peer_keys"],
                                        d["keys"], d_rotated, stream=stream, n=n, **sizes)

            def received_restored():
                restore(), received()

            # the send side: one job of one packet per peer
            d_sizes = torch.full((P,), 100, dtype=torch.int32, device="cuda")
            d_peer = torch.arange(P, dtype=torch.int32, device="cuda")
            d_count, d_jstatus = torch.ones(P, dtype=torch.int32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
            d_nonce = torch.zeros(n_keys, dtype=torch.int64, device="cuda")
            d_spkts = torch.zeros(24 * P, dtype=torch.uint8, device="cuda")
            d_nbufs, d_job_key = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")

            def assign(peer_keys):
                keystate.send_assign_batch(dev, d_sizes, d_peer, d_count, d_jstatus, 1, 256, peer_keys, d_nonce, d_spkts, d_nbufs,
                                           d_job_key, d_work, stream=stream, n_jobs=P, n_slots=len(t["peer_keys"]), n_keys=n_keys)

            def device_chain():
                restore(), replay(), received(), assign(d["peer_keys"])

            # the parent's way: the rotation and both slot tables are the host's
            h_verdict = torch.empty(4 * n, dtype=torch.uint8).pin_memory()
            np_verdict = h_verdict.numpy().view(np.int32)
            h_rotated = np.zeros(n, np.uint32)
            d_hslots, d_hpk = d0["slots"].clone(), d0["peer_keys"].clone()
            host_s = []

            def host_chain():
                if with_next:
                    d_hslots.copy_(d0["slots"]), d_hpk.copy_(d0["peer_keys"])
                h = {k: v.copy() for k, v in t.items()} if with_next else t
                replay()
                h_verdict.copy_(d_verdict.view(torch.uint8), non_blocking=True)
                stream.synchronize()
                t0 = time.perf_counter()
                keypairs.received_host(pkts, np_verdict, h["key_peer"], peer_rows, h["kp"], h["slots"], h["peer_keys"], h["keys"],
                                       h_rotated)
                if h_rotated.any():  # sessions changed: both tables are built again and uploaded, as before this call existed
                    live = h["slots"][h["slots"]["key"] < n_keys]
                    slots = router.session_table(live["index"], live["key"], n_slots=len(h["slots"]))
                    cur = h["kp"]["current"]
                    pk = router.session_table(table["peer"], cur["send_key"], n_slots=len(h["peer_keys"]))
                    host_s.append(time.perf_counter() - t0)
                    d_hslots.copy_(torch.from_numpy(slots.view(np.uint8).reshape(-1)), non_blocking=True)
                    d_hpk.copy_(torch.from_numpy(pk.view(np.uint8).reshape(-1)), non_blocking=True)
                else:
                    host_s.append(time.perf_counter() - t0)
                assign(d_hpk)
                return h

            # the device's tables are the host form's
            restore(), replay(), received()
            torch.cuda.synchronize()
            h = {k: v.copy() for k, v in t.items()}
            want = np.zeros(n, np.uint32)
            keypairs.received_host(pkts, d_verdict.cpu().numpy(), h["key_peer"], peer_rows, h["kp"], h["slots"], h["peer_keys"],
                                   h["keys"], want)
            assert np.array_equal(d_rotated.cpu().numpy().view(np.uint32), want), "device d_rotated != host form"
            assert int(want.sum()) == (min(n, P) if with_next else 0)
            for k in TABLES:
                assert d[k].cpu().numpy().tobytes() == h[k].tobytes(), f"device {k} != host form"
            assert (d_verdict.cpu().numpy() == 100).all()
            res = {"metric": "keypairs_received_rows_per_s", "unit": "rows/s", "steps": args.steps, "warmup": args.warmup,
                   "variant": variant,
                   "workload": {"rows": n, "peers": P, "candidates": int(want.sum()), "n_keys": n_keys,
                                "n_slots": len(t["slots"])},
                   "kernel": "kp_received_claim_kernel + kp_received_commit_kernel"}
            if args.mode == "received":
                rounds = [(events(received_restored), events(replay)) for _ in range(3)]  # alternating, in one process
                restore_us = events(restore) if with_next else 0.0
                us = float(np.median([r[0] for r in rounds]))
                res.update({"value": round(n / (us * 1e-6)), "us_per_call": [r[0] for r in rounds],
                            "table_restore_us_inside_each_call": restore_us,
                            "replay_batch_us_same_rows": [r[1] for r in rounds],
                            "timing": "HIP events around K calls, three rounds alternating with wgcs_replay_batch "
                                      "(its figure includes one elementwise add over the counters)"})
            else:
                chain_us = events(device_chain)
                t0 = time.perf_counter()
                for _ in range(10):
                    {k: v.copy() for k, v in t.items()}
                copy_us = round((time.perf_counter() - t0) * 1e5, 2)  # the bench's own: host_chain starts from fresh host tables
                rounds = [(wall(device_chain), wall(host_chain)) for _ in range(3)]
                res.update({"metric": "keypairs_chain_us", "unit": "us", "value": float(np.median([r[0][0] for r in rounds])),
                            "chain": "replay, received, send-assign of one job per peer, on one stream; one_per_peer restores the five "
                                     "tables first, by device copies",
                            "device_events_us": chain_us,
                            "device_wall_us_median_min": [r[0] for r in rounds],
                            "parent_way_wall_us_median_min": [r[1] for r in rounds],
                            "parent_way_host_part_us_median": round(float(np.median(host_s)) * 1e6, 2),
                            "parent_way_bench_table_copy_us": copy_us,
                            "parent_way": "replay, stream synchronise, verdicts to pinned memory, "
                                          "wgcs_keypairs_received_host on one core over a copy of the host tables, and where a "
                                          "peer rotated wgcs_session_table_build of both slot tables and their upload; then "
                                          "send-assign",
                            "wall": "host clock around one call ending in a device synchronise; three rounds, alternating"})
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
