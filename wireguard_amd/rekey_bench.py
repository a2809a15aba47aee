"""Keypair expiry and rekey measurement: the six
wgcs_rekey_*_batch calls on one MI355X, each beside its comparison in the same
process, alternating.  Not part of bench.py.

  python -m wireguard_amd.rekey_bench --mode gates|start|chain [--peers 1024 --steps 200 --warmup 10]

Workload: `peers` peers, each with a current keypair ten seconds old (key rows
2r, 2r + 1; every other peer its initiator), at 65,536 and 1,024 rows.
  gates  the receive gate over `rows` packets spread over the peers' receive
         keys, beside wgcs_keypairs_received_batch over the same rows (the same
         three dependent loads, no candidate); the send gate plus sent over
         `rows` jobs of one packet, beside wgcs_send_assign_batch over them.
         Nothing is stale, so nothing but the gate's statuses is written.
  start  wgcs_rekey_start_batch over the peer rows with no wish at all and with
         a wish for every peer and a ticket for each.  That variant commits,
         so a device copy restores the table before every call, inside the
         timed window, and the restore is timed alone as well; a call without
         a wish writes nothing to the table and restores nothing.
  chain  send-gate -> send-assign -> sent -> start -> initiate on one stream
         ending in one synchronise, with 64 peers' keypairs 181 s old and 64
         tickets; beside it the parent's way: synchronise, read the keypairs
         and nonces back, wgcs_rekey_send_gate_host on one core, upload the
         statuses, send-assign, synchronise, read its outputs back,
         wgcs_rekey_sent_host and wgcs_rekey_start_host, upload the
         descriptors, initiate, synchronise.  Timed by a host clock.
The device's outputs are compared with the host forms' before anything is
timed.  Prints one JSON line per batch size and variant.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from . import keypairs, keystate, noise, rekey, router
from ._lib import KEYPAIR_INITIATOR, KEYPAIR_SET, REJECT_AFTER_MESSAGES
from .noise import HS_PEER_DTYPE, HS_START_DTYPE
from .rekey import REKEY_DTYPE
from .transport import AEAD_PKT_DTYPE

NOW = 1_700_000_000_000_000_000
SECOND = 1_000_000_000
LIMIT = REJECT_AFTER_MESSAGES


def make_world(n_peers: int, stale: int = 0, seed: int = 20261101):
    """Peer ids 0 .. n_peers - 1 on rows of their own; row r's current keypair is (2r, 2r + 1), 181 s old for
    the first `stale` rows and 10 s for the others."""
    rng = np.random.default_rng(seed)
    own, own_public = noise.responder_init(rng.bytes(32))
    publics = [noise.responder_init(rng.bytes(32))[1] for _ in range(n_peers)]
    table = noise.peer_keys_build(own, publics, np.arange(n_peers))
    peer_rows = noise.peer_rows_build(table, n_peers)
    r = np.arange(n_peers, dtype=np.uint32)
    kp = keypairs.keypairs_table(n_peers)
    kp["current"]["send_key"], kp["current"]["recv_key"], kp["current"]["local_index"] = 2 * r, 2 * r + 1, 0x1000 + r
    kp["current"]["flags"] = KEYPAIR_SET | np.where(r % 2 == 0, KEYPAIR_INITIATOR, 0).astype(np.uint32)
    kp["current"]["created_ns"] = NOW - np.where(r < stale, 181, 10) * SECOND
    key_peer = np.repeat(table["peer"], 2).astype(np.uint32)
    hs_peers = np.zeros(n_peers, HS_PEER_DTYPE)
    hs_peers["claim"] = 0xFFFFFFFF
    return dict(table=table, peer_rows=peer_rows, kp=kp, key_peer=key_peer, send_nonce=np.zeros(2 * n_peers, np.uint64),
                hs_peers=hs_peers, rekey=rekey.rekey_table(n_peers, NOW), own_public=np.frombuffer(own_public, np.uint8),
                peer_keys=router.session_table(table["peer"], 2 * r))


def make_tickets(n: int, seed: int = 20261102) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.frombuffer(rng.bytes(96 * n), HS_START_DTYPE).copy()
    q = np.arange(n, dtype=np.uint32)
    t["state_row"], t["local_index"], t["send_key"], t["recv_key"] = q, 0x400000 + q, 2 * q, 2 * q + 1
    return t


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("gates", "start", "chain"), required=True)
    ap.add_argument("--peers", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch

    from .tun import Device

    dev = Device(0)
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = args.peers

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def i32(n, fill=0):
        return torch.full((max(n, 1),), fill, dtype=torch.int32, device="cuda")

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

    base = {"steps": args.steps, "warmup": args.warmup, "peers": P}
    if args.mode == "start":
        w = make_world(P)
        tickets = make_tickets(P)
        for variant, want in (("no_candidates", 0), ("every_peer", 0x40)):
            table0 = w["rekey"].copy()
            table0["want"] = want
            d0, d_rekey = up(table0), up(table0)
            d_hs, d_tickets = up(w["hs_peers"]), up(tickets)
            d_start, d_sp, d_count, d_status, d_reasons = torch.zeros(96 * P, dtype=torch.uint8, device="cuda"), i32(P), i32(1), i32(P), i32(P)
            d_work = torch.zeros(keystate.work_bytes(P), dtype=torch.uint8, device="cuda")

            def restore():  # a call without a wish writes nothing to the table: only the other variant restores
                if want:
                    d_rekey.copy_(d0)

            def call():
                restore()
                rekey.start_batch(dev, NOW, d_rekey, d_hs, d_tickets, d_start, d_sp, d_count, d_status, d_reasons, d_work,
                                  stream=stream, n_peers=P, n_tickets=P)

            h = table0.copy()
            h_start, h_sp, h_count = np.zeros(P, HS_START_DTYPE), np.zeros(P, np.uint32), np.zeros(1, np.uint32)
            h_status, h_reasons = np.zeros(P, np.int32), np.zeros(P, np.uint32)
            t0 = time.perf_counter()
            rekey.start_host(NOW, h, w["hs_peers"], tickets, h_start, h_sp, h_count, h_status, h_reasons)
            host_us = (time.perf_counter() - t0) * 1e6
            call()
            torch.cuda.synchronize()
            assert d_rekey.cpu().numpy().tobytes() == h.tobytes() and d_start.cpu().numpy().tobytes() == h_start.tobytes()
            assert np.array_equal(d_status.cpu().numpy()[:P], h_status) and d_count.cpu().numpy()[0] == h_count[0] == (P if want else 0)
            rounds = [(events(call), events(restore) if want else 0.0) for _ in range(3)]
            print(json.dumps({**base, "metric": "rekey_start_us", "unit": "us", "variant": variant,
                              "value": float(np.median([r[0] for r in rounds])), "us_per_call": [r[0] for r in rounds],
                              "table_restore_us_inside_each_call": [r[1] for r in rounds], "candidates": int(h_count[0]),
                              "tickets": P, "host_one_core_us": round(host_us, 2),
                              "kernel": "rekey_start_verdict_kernel + compact_scan_kernel + rekey_start_commit_kernel",
                              "timing": "HIP events around K calls, three rounds alternating with the restore alone"}), flush=True)
        return

    for n in (65536, 1024):
        if args.mode == "gates":
            w = make_world(P)
            d = {k: up(v) for k, v in w.items()}
            pkts = np.zeros(n, AEAD_PKT_DTYPE)
            pkts["key"], pkts["len"] = 2 * (np.arange(n, dtype=np.uint32) % P) + 1, 132
            d_pkts, d_verdict, d_rotated = up(pkts), i32(n, 100), i32(n)
            d_keys = torch.zeros(48 * 2 * P, dtype=torch.uint8, device="cuda")

            def recv_gate():
                rekey.recv_gate_batch(dev, d_pkts, NOW, d["key_peer"], d["peer_rows"], d["kp"], stream=stream, n=n, n_keys=2 * P,
                                      n_ids=P, n_peers=P)

            def kp_received():
                keypairs.received_batch(dev, d_pkts, d_verdict, d["key_peer"], d["peer_rows"], d["kp"], None, None, d_keys,
                                        d_rotated, stream=stream, n=n, n_keys=2 * P, n_ids=P, n_peers=P, n_slots=0, n_peer_slots=0)

            peer = (np.arange(n, dtype=np.uint32) % P).astype(np.uint32)
            d_peer, d_count, d_status_in, d_status = up(peer), i32(n, 1), i32(n), i32(n, 7)
            d_sizes, d_spkts, d_nbufs, d_job_key = i32(n, 100), torch.zeros(24 * n, dtype=torch.uint8, device="cuda"), i32(n), i32(n)
            d_work = torch.zeros(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")

            def send_gate_sent():
                rekey.send_gate_batch(dev, d_peer, d_count, d_status_in, 1, NOW, d["peer_rows"], d["kp"], d["send_nonce"], LIMIT,
                                      d["rekey"], d_status, stream=stream, n_jobs=n, n_ids=P, n_peers=P, n_keys=2 * P)
                rekey.sent_batch(dev, d_peer, d_count, d_status, d_job_key, 1, NOW, d["peer_rows"], d["kp"], d["send_nonce"],
                                 LIMIT, d["rekey"], stream=stream, n_jobs=n, n_ids=P, n_peers=P, n_keys=2 * P)

            def assign():
                d["send_nonce"].zero_()
                keystate.send_assign_batch(dev, d_sizes, d_peer, d_count, d_status_in, 1, 256, d["peer_keys"], d["send_nonce"],
                                           d_spkts, d_nbufs, d_job_key, d_work, stream=stream, n_jobs=n,
                                           n_slots=len(w["peer_keys"]), n_keys=2 * P)

            assign(), recv_gate(), send_gate_sent()
            torch.cuda.synchronize()
            assert d_pkts.cpu().numpy().tobytes() == pkts.tobytes() and not d_status.cpu().numpy()[:n].any()
            assert d["rekey"].cpu().numpy().tobytes() == w["rekey"].tobytes(), "nothing is stale: no wish"
            rounds = [(events(recv_gate), events(kp_received), events(send_gate_sent), events(assign)) for _ in range(3)]
            print(json.dumps({**base, "metric": "rekey_gates_us", "unit": "us", "rows": n,
                              "value": float(np.median([r[0] for r in rounds])),
                              "recv_gate_us": [r[0] for r in rounds], "keypairs_received_us_same_rows": [r[1] for r in rounds],
                              "send_gate_plus_sent_us": [r[2] for r in rounds],
                              "send_assign_us_same_jobs": [r[3] for r in rounds],
                              "timing": "HIP events around K calls, three rounds, the four alternating in one process; "
                                        "send-assign's figure includes a memset of the nonces"}), flush=True)
            continue

        stale, n_tickets = 64, 64
        w = make_world(P, stale=stale)
        tickets = make_tickets(n_tickets)
        d = {k: up(v) for k, v in w.items()}
        d_rekey0 = up(w["rekey"])
        peer = (np.arange(n, dtype=np.uint32) % P).astype(np.uint32)
        count, status_in = np.ones(n, np.int32), np.zeros(n, np.int32)
        d_peer, d_count, d_status_in, d_status = up(peer), up(count), up(status_in), i32(n, 7)
        d_sizes, d_spkts, d_nbufs, d_job_key = i32(n, 100), torch.zeros(24 * n, dtype=torch.uint8, device="cuda"), i32(n), i32(n)
        d_work = torch.zeros(keystate.work_bytes(max(n, P)), dtype=torch.uint8, device="cuda")
        d_tickets, d_start, d_sp, d_n, d_sstatus, d_reasons = up(tickets), torch.zeros(96 * n_tickets, dtype=torch.uint8, device="cuda"), i32(n_tickets), i32(1), i32(P), i32(P)
        d_states = torch.zeros(128 * n_tickets, dtype=torch.uint8, device="cuda")
        d_msgs, d_istatus = torch.zeros(160 * n_tickets, dtype=torch.uint8, device="cuda"), i32(n_tickets)

        def restore():
            d["rekey"].copy_(d_rekey0)
            d["send_nonce"].zero_()

        def gate(status_out=d_status):
            rekey.send_gate_batch(dev, d_peer, d_count, d_status_in, 1, NOW, d["peer_rows"], d["kp"], d["send_nonce"], LIMIT,
                                  d["rekey"], status_out, stream=stream, n_jobs=n, n_ids=P, n_peers=P, n_keys=2 * P)

        def assign():
            keystate.send_assign_batch(dev, d_sizes, d_peer, d_count, d_status, 1, 256, d["peer_keys"], d["send_nonce"], d_spkts,
                                       d_nbufs, d_job_key, d_work, stream=stream, n_jobs=n, n_slots=len(w["peer_keys"]),
                                       n_keys=2 * P)

        def initiate():
            noise.initiate_batch(dev, d_start, d["own_public"], d["table"], d_states, d_msgs, d_istatus, 2 * P, stream=stream,
                                 n=n_tickets, n_peers=P, n_states=n_tickets)

        def device_chain():
            restore(), gate(), assign()
            rekey.sent_batch(dev, d_peer, d_count, d_status, d_job_key, 1, NOW, d["peer_rows"], d["kp"], d["send_nonce"], LIMIT,
                             d["rekey"], stream=stream, n_jobs=n, n_ids=P, n_peers=P, n_keys=2 * P)
            rekey.start_batch(dev, NOW, d["rekey"], d["hs_peers"], d_tickets, d_start, d_sp, d_n, d_sstatus, d_reasons, d_work,
                              stream=stream, n_peers=P, n_tickets=n_tickets)
            initiate()

        pin = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8).pin_memory()  # noqa: E731
        p_kp, p_nonce, p_rekey, p_status = pin(80 * P), pin(16 * P), pin(16 * P), pin(4 * n)
        p_job_key, p_start = pin(4 * n), pin(96 * n_tickets)
        host_s = []

        def host_chain():
            restore()
            p_kp.copy_(d["kp"], non_blocking=True), p_nonce.copy_(d["send_nonce"], non_blocking=True)
            p_rekey.copy_(d["rekey"], non_blocking=True)
            stream.synchronize()
            t0 = time.perf_counter()
            h_rekey = p_rekey.numpy().view(REKEY_DTYPE)
            rekey.send_gate_host(peer, count, status_in, 1, NOW, w["peer_rows"], p_kp.numpy().view(keypairs.KEYPAIRS_DTYPE),
                                 p_nonce.numpy().view(np.uint64), LIMIT, h_rekey, p_status.numpy().view(np.int32))
            t1 = time.perf_counter()
            d_status.view(torch.uint8)[:4 * n].copy_(p_status, non_blocking=True)
            assign()
            p_job_key.copy_(d_job_key.view(torch.uint8)[:4 * n], non_blocking=True), p_nonce.copy_(d["send_nonce"], non_blocking=True)
            stream.synchronize()
            t2 = time.perf_counter()
            rekey.sent_host(peer, count, p_status.numpy().view(np.int32), p_job_key.numpy().view(np.uint32), 1, NOW,
                            w["peer_rows"], p_kp.numpy().view(keypairs.KEYPAIRS_DTYPE), p_nonce.numpy().view(np.uint64), LIMIT,
                            h_rekey)
            rekey.start_host(NOW, h_rekey, w["hs_peers"], tickets, p_start.numpy().view(HS_START_DTYPE), h_sp, h_n, h_sstatus,
                             h_reasons)
            host_s.append(t1 - t0 + time.perf_counter() - t2)
            d_start.copy_(p_start, non_blocking=True), d["rekey"].copy_(p_rekey, non_blocking=True)
            initiate()

        h_sp, h_n, h_sstatus, h_reasons = np.zeros(n_tickets, np.uint32), np.zeros(1, np.uint32), np.zeros(P, np.int32), np.zeros(P, np.uint32)
        # the two ways agree before anything is timed
        device_chain()
        torch.cuda.synchronize()
        got = (d["rekey"].cpu().numpy().tobytes(), d_start.cpu().numpy().tobytes(), d_msgs.cpu().numpy().tobytes(),
               d_istatus.cpu().numpy().tolist())
        host_chain()
        torch.cuda.synchronize()
        assert got == (d["rekey"].cpu().numpy().tobytes(), d_start.cpu().numpy().tobytes(), d_msgs.cpu().numpy().tobytes(),
                       d_istatus.cpu().numpy().tolist()), "the device chain and the parent's way differ"
        assert h_n[0] == min(stale, P) and d_istatus.cpu().numpy()[:h_n[0]].tolist() == [noise.HS_INITIATED] * int(h_n[0])
        host_s.clear()
        chain_us = events(device_chain)
        rounds = [(wall(device_chain), wall(host_chain)) for _ in range(3)]
        print(json.dumps({**base, "metric": "rekey_chain_us", "unit": "us", "jobs": n, "stale_peers": stale, "tickets": n_tickets,
                          "value": float(np.median([r[0][0] for r in rounds])), "device_events_us": chain_us,
                          "device_wall_us_median_min": [r[0] for r in rounds],
                          "parent_way_wall_us_median_min": [r[1] for r in rounds],
                          "parent_way_host_part_us_median": round(float(np.median(host_s)) * 1e6, 2),
                          "chain": "restore (a table copy and a memset), send-gate, send-assign, sent, start, initiate over 64 "
                                   "descriptors, one synchronise",
                          "parent_way": "restore, keypairs / nonces / rekey table to pinned memory, synchronise, "
                                        "wgcs_rekey_send_gate_host, statuses up, send-assign, job keys and nonces back, "
                                        "synchronise, wgcs_rekey_sent_host and wgcs_rekey_start_host, descriptors and table up, "
                                        "initiate, synchronise",
                          "wall": "host clock around one call ending in a device synchronise; three rounds, alternating"}),
              flush=True)


if __name__ == "__main__":
    main()
