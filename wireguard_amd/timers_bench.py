"""Peer-timer measurement: the seven wgcs_timers_*_batch calls
on one MI355X, each beside its comparison in the same process, alternating.
Not part of bench.py.

  python -m wireguard_amd.timers_bench --mode events|expire|chain [--peers 1024 --steps 200 --warmup 10]

Workload: the world of rekey_bench (`peers` peers, each with a current keypair
ten seconds old), every timer row active with a keepalive interval of 25 s.
  events  timers_sent over `rows` kept jobs of one data packet beside
          wgcs_rekey_sent_batch over the same jobs, and timers_received over
          `rows` data groups beside wgcs_rekey_received_batch over them, at
          65,536 and 1,024 rows spread over the peers.
  expire  wgcs_timers_expire_batch over the peer rows with nothing due and
          with every row owing a keepalive and a job for each.  That variant
          clears the flag it serves, so a device copy restores the table
          before every call, inside the timed window, and the restore is
          timed alone as well.  wgcs_timers_expire_host on one core beside it.
  chain   expire -> start -> initiate -> timers_initiated on one stream ending
          in one synchronise, with resendHandshake due for 64 peers and 64
          tickets; beside it the parent's way: the two tables to pinned
          memory, synchronise, wgcs_timers_expire_host on one core, the tables
          up again, start, initiate, timers_initiated, synchronise.  Timed by
          a host clock.
The device's outputs are compared with the host forms' before anything is
timed.  Prints one JSON line per batch size and variant.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from . import keystate, noise, rekey, timers
from ._lib import GROUP_DATA, REJECT_AFTER_MESSAGES, TIMERS_KEEPALIVE_NOW
from .rekey import REKEY_DTYPE
from .rekey_bench import NOW, SECOND, make_tickets, make_world
from .timers import TIMERS_DTYPE
from .transport import AEAD_KEY_DTYPE
from .writeplan import WRITE_GROUP_DTYPE

LIMIT = REJECT_AFTER_MESSAGES
SEED = 20261201


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("events", "expire", "chain"), required=True)
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
    w = make_world(P)
    table0 = timers.timers_table(P, 25)
    keys = np.zeros(2 * P, AEAD_KEY_DTYPE)
    no_slots = np.zeros(0, timers.SESSION_SLOT_DTYPE)

    def host_expire(now, tm, rk, room):
        o = dict(ka_peer=np.zeros(room, np.uint32), ka_count=np.zeros(room, np.int32), ka_sizes=np.zeros(room, np.int32),
                 ka_status=np.zeros(room, np.int32), n_ka=np.zeros(1, np.uint32), actions=np.zeros(P, np.uint32))
        t0 = time.perf_counter()
        timers.expire_host(now, tm, rk, w["table"], None, w["kp"].copy(), no_slots.copy(), w["peer_keys"].copy(), keys.copy(),
                           w["key_peer"].copy(), o["ka_peer"], o["ka_count"], o["ka_sizes"], o["ka_status"], o["n_ka"],
                           o["actions"])
        return o, (time.perf_counter() - t0) * 1e6

    if args.mode == "events":
        for n in (65536, 1024):
            d = {k: up(v) for k, v in w.items()}
            d_timers = up(table0)
            peer = (np.arange(n, dtype=np.uint32) % P).astype(np.uint32)
            count, status, job_key, sizes = np.ones(n, np.int32), np.zeros(n, np.int32), np.full(n, 7, np.uint32), np.full(n, 100, np.int32)
            d_peer, d_count, d_status, d_job_key, d_sizes = up(peer), up(count), up(status), up(job_key), up(sizes)
            groups = np.zeros(n, WRITE_GROUP_DTYPE)
            groups["peer"], groups["tail"], groups["flags"], groups["n_valid"] = peer, np.arange(n), GROUP_DATA, 1
            d_groups = up(groups)
            cpb = 128

            def t_sent():
                timers.sent_batch(dev, d_sizes, d_peer, d_count, d_status, d_job_key, 1, NOW, SEED, d["peer_rows"], d_timers,
                                  stream=stream, n_jobs=n, n_ids=P, n_peers=P)

            def r_sent():
                rekey.sent_batch(dev, d_peer, d_count, d_status, d_job_key, 1, NOW, d["peer_rows"], d["kp"], d["send_nonce"],
                                 LIMIT, d["rekey"], stream=stream, n_jobs=n, n_ids=P, n_peers=P, n_keys=2 * P)

            def t_rcvd():
                timers.received_batch(dev, d_groups, cpb, NOW, d["peer_rows"], d_timers, stream=stream, n_batches=n // cpb,
                                      n_ids=P, n_peers=P)

            def r_rcvd():
                rekey.received_batch(dev, d_groups, cpb, NOW, d["peer_rows"], d["kp"], d["rekey"], stream=stream,
                                     n_batches=n // cpb, n_ids=P, n_peers=P)

            h = table0.copy()
            timers.sent_host(sizes, peer, count, status, job_key, 1, NOW, SEED, w["peer_rows"], h)
            timers.received_host(groups, cpb, NOW, w["peer_rows"], h)
            t_sent(), t_rcvd(), r_sent(), r_rcvd()
            torch.cuda.synchronize()
            assert d_timers.cpu().numpy().tobytes() == h.tobytes(), "timers_sent / timers_received differ from the host forms"
            assert d["rekey"].cpu().numpy().tobytes() == w["rekey"].tobytes(), "nothing is stale: no wish"
            rounds = [(events(t_sent), events(r_sent), events(t_rcvd), events(r_rcvd)) for _ in range(3)]
            print(json.dumps({**base, "metric": "timers_events_us", "unit": "us", "rows": n,
                              "value": float(np.median([r[0] for r in rounds])), "timers_sent_us": [r[0] for r in rounds],
                              "rekey_sent_us_same_jobs": [r[1] for r in rounds], "timers_received_us": [r[2] for r in rounds],
                              "rekey_received_us_same_groups": [r[3] for r in rounds],
                              "timing": "HIP events around K calls, three rounds, the four alternating in one process; after "
                                        "the first call every timer the rows arm is armed already"}), flush=True)
        return

    d = {k: up(v) for k, v in w.items()}
    d_keys = up(keys)
    d_work = torch.zeros(keystate.work_bytes(P), dtype=torch.uint8, device="cuda")
    ka = dict(ka_peer=i32(P), ka_count=i32(P), ka_sizes=i32(P), ka_status=i32(P), n_ka=i32(1), actions=i32(P))

    def expire(now, d_timers, room=P):
        timers.expire_batch(dev, now, d_timers, d["rekey"], d["table"], None, d["kp"], None, d["peer_keys"], d_keys,
                            d["key_peer"], ka["ka_peer"], ka["ka_count"], ka["ka_sizes"], ka["ka_status"], ka["n_ka"],
                            ka["actions"], d_work, stream=stream, n_peers=P, n_slots=0, n_peer_slots=len(w["peer_keys"]),
                            n_keys=2 * P, n_ka_max=room)

    def same(o, room):
        return all(ka[k].cpu().numpy().view(np.uint8)[:o[k].nbytes].tobytes() == o[k].tobytes() for k in o)

    if args.mode == "expire":
        for variant, flag in (("nothing_due", 0), ("every_row_owes_a_keepalive", TIMERS_KEEPALIVE_NOW)):
            t0 = table0.copy()
            t0["flags"] |= flag
            d0, d_timers = up(t0), up(t0)

            def restore():  # a call with nothing due writes nothing to the table: only the other variant restores
                if flag:
                    d_timers.copy_(d0)

            def call():
                restore()
                expire(NOW, d_timers)

            h, hr = t0.copy(), w["rekey"].copy()
            o, host_us = host_expire(NOW, h, hr, P)
            call()
            torch.cuda.synchronize()
            assert d_timers.cpu().numpy().tobytes() == h.tobytes() and same(o, P), "expire differs from the host form"
            assert o["n_ka"][0] == (P if flag else 0)
            rounds = [(events(call), events(restore) if flag else 0.0) for _ in range(3)]
            print(json.dumps({**base, "metric": "timers_expire_us", "unit": "us", "variant": variant,
                              "value": float(np.median([r[0] for r in rounds])), "us_per_call": [r[0] for r in rounds],
                              "table_restore_us_inside_each_call": [r[1] for r in rounds], "keepalive_jobs": int(o["n_ka"][0]),
                              "host_one_core_us": round(host_us, 2),
                              "kernel": "timers_expire_verdict_kernel + compact_scan_kernel + timers_expire_commit_kernel",
                              "timing": "HIP events around K calls, three rounds alternating with the restore alone"}), flush=True)
        return

    due, n_tickets = 64, 64
    t0 = table0.copy()
    t0["pending"][:due], t0["deadline_ns"][:due, 1], t0["attempts"][:due] = 0b00010, NOW - SECOND, 1
    now = NOW + 10 * SECOND  # past RekeyTimeout of the tables' lastSentHandshake
    tickets = make_tickets(n_tickets)
    d0, d_timers, d_rekey0 = up(t0), up(t0), up(w["rekey"])
    d_tickets, d_start, d_sp, d_n, d_sstatus, d_reasons = up(tickets), torch.zeros(96 * n_tickets, dtype=torch.uint8, device="cuda"), i32(n_tickets), i32(1), i32(P), i32(P)
    d_states = torch.zeros(128 * n_tickets, dtype=torch.uint8, device="cuda")
    d_msgs, d_istatus = torch.zeros(160 * n_tickets, dtype=torch.uint8, device="cuda"), i32(n_tickets)

    def restore():
        d_timers.copy_(d0), d["rekey"].copy_(d_rekey0)

    def start_to_initiated():
        rekey.start_batch(dev, now, d["rekey"], d["hs_peers"], d_tickets, d_start, d_sp, d_n, d_sstatus, d_reasons, d_work,
                          stream=stream, n_peers=P, n_tickets=n_tickets)
        noise.initiate_batch(dev, d_start, d["own_public"], d["table"], d_states, d_msgs, d_istatus, 2 * P, stream=stream,
                             n=n_tickets, n_peers=P, n_states=n_tickets)
        timers.initiated_batch(dev, d_reasons, d_sp, d_istatus, now, SEED, d_timers, stream=stream, n_tickets=n_tickets,
                               n_peers=P)

    def device_chain():
        restore()
        expire(now, d_timers, room=due)
        start_to_initiated()

    pin = lambda nbytes: torch.empty(nbytes, dtype=torch.uint8).pin_memory()  # noqa: E731
    p_timers, p_rekey = pin(64 * P), pin(16 * P)
    host_s = []

    def host_chain():
        restore()
        p_timers.copy_(d_timers, non_blocking=True), p_rekey.copy_(d["rekey"], non_blocking=True)
        stream.synchronize()
        _, us = host_expire(now, p_timers.numpy().view(TIMERS_DTYPE), p_rekey.numpy().view(REKEY_DTYPE), due)
        host_s.append(us)
        d_timers.copy_(p_timers, non_blocking=True), d["rekey"].copy_(p_rekey, non_blocking=True)
        start_to_initiated()

    def state():
        torch.cuda.synchronize()
        return (d_timers.cpu().numpy().tobytes(), d["rekey"].cpu().numpy().tobytes(), d_start.cpu().numpy().tobytes(),
                d_msgs.cpu().numpy().tobytes(), d_istatus.cpu().numpy().tolist())

    device_chain()
    got = state()
    host_chain()
    assert got == state(), "the device chain and the parent's way differ"
    tm = np.frombuffer(got[0], TIMERS_DTYPE)
    assert d_n.cpu().numpy()[0] == due and (tm["attempts"][:due] == 2).all() and (tm["pending"][:due] & 2).all()
    assert got[4][:due] == [noise.HS_INITIATED] * due
    host_s.clear()
    chain_us = events(device_chain)
    rounds = [(wall(device_chain), wall(host_chain)) for _ in range(3)]
    print(json.dumps({**base, "metric": "timers_chain_us", "unit": "us", "due_peers": due, "tickets": n_tickets,
                      "value": float(np.median([r[0][0] for r in rounds])), "device_events_us": chain_us,
                      "device_wall_us_median_min": [r[0] for r in rounds],
                      "parent_way_wall_us_median_min": [r[1] for r in rounds],
                      "parent_way_host_part_us_median": round(float(np.median(host_s)), 2),
                      "chain": "restore (two table copies), expire, start, initiate over 64 descriptors, timers_initiated, one "
                               "synchronise",
                      "parent_way": "restore, timers and rekey tables to pinned memory, synchronise, wgcs_timers_expire_host, "
                                    "both tables up, start, initiate, timers_initiated, synchronise",
                      "wall": "host clock around one call ending in a device synchronise; three rounds, alternating"}),
          flush=True)


if __name__ == "__main__":
    main()
