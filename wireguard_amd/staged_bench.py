"""Staged-queue measurement: the wgcs_staged_*_batch calls on
one MI355X, each beside its comparison in the same process, in alternating
rounds.  Not part of bench.py.

  python -m wireguard_amd.staged_bench --mode stage|release|chain [--peers 1024 --steps 200 --warmup 10 --rounds 3]

Workload: `peers` peers with rings of 128 slots of 1,472 bytes, packets of
1,420 bytes, single-segment jobs spread evenly over the peers.
  stage    at 65,536 and 1,024 jobs: every job refused (the rings are full after
           the first calls, so every call evicts as many packets as it copies),
           beside a plain device-to-device copy of jobs * 1,420 bytes (one pair
           of buffers, which the Infinity Cache holds, and three pairs in turn,
           which it does not); nothing
           refused, beside wgcs_rekey_sent_batch over the same jobs, and gate ->
           send-assign -> sent -> stage beside the same chain without the stage
           call; and wgcs_staged_stage_host on one core, once, for scale.
  release  over the peer rows: no peer ready; every peer ready with 64 packets,
           beside a plain copy of the same bytes (the lengths are restored by a
           4-KiB device copy inside the timed window, timed alone as well);
           every peer ready with one packet; and the host form on one core.
  chain    64 jobs of one peer without a keypair: gate -> send-assign -> stage
           -> (the keypair appears: a device copy of one table row) -> release
           -> send-assign -> sent -> seal on one stream, one synchronise;
           beside the parent's way: gate, synchronise, read the statuses, keep
           the refused jobs on the host, (the keypair appears), upload them
           again, gate -> send-assign -> sent -> seal, synchronise.  Timed by a
           host clock.
Everything runs on one stream.  Times are HIP events around `steps` calls,
microseconds per call; the device's
outputs are compared with the host forms' before anything is timed.  Prints one
JSON line per variant and round.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from . import keystate, rekey, staged, transport
from ._lib import ERR_KEY_EXPIRED, REJECT_AFTER_MESSAGES
from .rekey_bench import NOW, make_world
from .transport import AEAD_KEY_DTYPE

LIMIT = REJECT_AFTER_MESSAGES
CAP, STRIDE, SIZE, MTU = 128, 1472, 1420, 1420
NO_KEY = 0xFFFFFFFF


def make_jobs(n_jobs: int, n_peers: int, seed: int = 20261201):
    """n_jobs single-segment jobs of SIZE bytes, job j for peer j % n_peers"""
    rng = np.random.default_rng(seed)
    arena = rng.integers(0, 256, n_jobs * STRIDE, dtype=np.uint8)
    return dict(arena=arena, sizes=np.full(n_jobs, SIZE, np.int32), peer=(np.arange(n_jobs) % n_peers).astype(np.uint32),
                count=np.ones(n_jobs, np.int32), status_in=np.zeros(n_jobs, np.int32))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("stage", "release", "chain"), required=True)
    ap.add_argument("--peers", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    from .tun import Device

    dev = Device(0)
    stream = torch.cuda.Stream()  # the calls and the copies beside them on one stream of their own: a copy on the
    torch.cuda.set_stream(stream)  # null stream between two calls would add a cross-stream wait to what is timed
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = args.peers

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def i32(n, fill=0):
        return torch.full((max(n, 1),), fill, dtype=torch.int32, device="cuda")

    def down(t, dt):
        return t.cpu().numpy().view(dt)

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

    def rounds(base, variants, timer=events):
        """the variants in turn, `rounds` times over"""
        for rnd in range(args.rounds):
            for name, fn in variants:
                t = timer(fn)
                row = dict(base, variant=name, round=rnd)
                row.update({"us_median": t[0], "us_min": t[1]} if isinstance(t, tuple) else {"us_per_call": t})
                print(json.dumps(row), flush=True)

    def device_state(h):
        return staged.State(*[up(a) for a in h.arrays()], h.n_peers, h.cap, h.stride)

    base = {"mode": args.mode, "steps": args.steps, "warmup": args.warmup, "peers": P, "cap": CAP, "stride": STRIDE,
            "size": SIZE}
    w = make_world(P)
    d_rows, d_kp, d_nonce, d_rekey = up(w["peer_rows"]), up(w["kp"]), up(w["send_nonce"]), up(w["rekey"])
    d_table, d_peer_keys = up(w["table"]), up(w["peer_keys"])
    n_keys, n_slots = len(w["send_nonce"]), len(w["peer_keys"])

    if args.mode == "stage":
        for n in (65536, 1024):
            jb = make_jobs(n, P)
            d = {k: up(v) for k, v in jb.items()}
            d_work = torch.zeros(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")
            d_where, d_gate, d_pkts, d_nbufs, d_key = i32(n), i32(n), torch.zeros(24 * n, dtype=torch.uint8, device="cuda"), i32(n), i32(n)
            d_refused, d_nokey = i32(n, ERR_KEY_EXPIRED), i32(n, -1)
            d_sent, d_key0 = i32(n, 0), up((2 * jb["peer"]).astype(np.uint32))
            st = device_state(staged.state(P, CAP, STRIDE))
            src, dst = torch.zeros(n * SIZE, dtype=torch.uint8, device="cuda"), torch.zeros(n * SIZE, dtype=torch.uint8, device="cuda")
            # the same copy over three pairs of buffers in turn: at 65,536 jobs 558 MB, past the 256 MiB Infinity Cache,
            # as the arena and the rings of the stage call are (96 + 193 MB)
            pairs, turn = [(torch.zeros_like(src), torch.zeros_like(dst)) for _ in range(3)], [0]

            def rotating_copy():
                a, b = pairs[turn[0] % 3]
                turn[0] += 1
                b.copy_(a)

            def stage(status_out, job_key):
                staged.stage_batch(dev, d["arena"], d["sizes"], d["peer"], d["count"], d["status_in"], status_out, job_key, 1,
                                   d_rows, st, d_where, d_work, stream=stream, n_jobs=n, n_ids=P)

            # the device's outputs against the host form's, twice: onto empty rings and onto rings that hold packets
            h = staged.state(P, CAP, STRIDE)
            h_where = np.zeros(n, np.uint32)
            for _ in range(2):
                staged.stage_host(jb["arena"], jb["sizes"], jb["peer"], jb["count"], jb["status_in"],
                                  np.full(n, ERR_KEY_EXPIRED, np.int32), np.full(n, NO_KEY, np.uint32), 1, w["peer_rows"], h,
                                  h_where)
                stage(d_refused, d_nokey)
            torch.cuda.synchronize()
            assert down(d_where, np.uint32).tobytes() == h_where.tobytes(), "d_where differs from the host form's"
            for got, want in zip(st.arrays(), h.arrays()):
                assert down(got, np.uint8).tobytes() == np.ascontiguousarray(want).view(np.uint8).tobytes(), "state differs"
            t0 = time.perf_counter()
            staged.stage_host(jb["arena"], jb["sizes"], jb["peer"], jb["count"], jb["status_in"],
                              np.full(n, ERR_KEY_EXPIRED, np.int32), np.full(n, NO_KEY, np.uint32), 1, w["peer_rows"], h, h_where)
            print(json.dumps(dict(base, jobs=n, variant="stage_host_one_core", us_per_call=round((time.perf_counter() - t0) * 1e6, 1))),
                  flush=True)

            def gate():
                rekey.send_gate_batch(dev, d["peer"], d["count"], d["status_in"], 1, NOW, d_rows, d_kp, d_nonce, LIMIT, d_rekey,
                                      d_gate, stream=stream, n_jobs=n, n_ids=P, n_peers=P, n_keys=n_keys)

            def assign():
                keystate.send_assign_batch(dev, d["sizes"], d["peer"], d["count"], d_gate, 1, STRIDE, d_peer_keys, d_nonce, d_pkts,
                                           d_nbufs, d_key, d_work, stream=stream, n_jobs=n, n_slots=n_slots, n_keys=n_keys)

            def sent(status=None, key=None):
                rekey.sent_batch(dev, d["peer"], d["count"], d_gate if status is None else status, d_key if key is None else key,
                                 1, NOW, d_rows, d_kp, d_nonce, LIMIT, d_rekey, stream=stream, n_jobs=n, n_ids=P, n_peers=P,
                                 n_keys=n_keys)

            def chain(with_stage):
                gate(), assign(), sent()
                if with_stage:
                    stage(d_gate, d_key)

            rounds(dict(base, jobs=n, bytes=n * SIZE), [
                ("stage_all_refused", lambda: stage(d_refused, d_nokey)),
                ("plain_copy_same_bytes", lambda: dst.copy_(src)),
                ("plain_copy_three_buffer_pairs", rotating_copy),
                ("stage_nothing_refused", lambda: stage(d_sent, d_key0)),
                ("rekey_sent_same_jobs", lambda: sent(d_sent, d_key0)),
                ("chain_with_stage", lambda: chain(True)),
                ("chain_without_stage", lambda: chain(False)),
            ])
    elif args.mode == "release":
        rng = np.random.default_rng(20261202)
        d_work = torch.zeros(keystate.work_bytes(P), dtype=torch.uint8, device="cuda")
        d_status, d_n_out = i32(P), i32(1)
        for variant, per_peer in (("none_ready", 0), ("all_ready_64_each", 64), ("all_ready_1_each", 1)):
            h = staged.state(P, CAP, STRIDE)
            h.ring[:] = rng.integers(0, 256, len(h.ring), dtype=np.uint8)
            h.len[:], h.head[:], h.slot_size[:] = per_peer, 100, SIZE  # the 64 packets straddle the wrap
            n_out = max(P * per_peer, 1)
            st, d_len0, d_head0 = device_state(h), up(h.len), up(h.head)
            d_out = torch.zeros(n_out * STRIDE, dtype=torch.uint8, device="cuda")
            d_op, d_oc, d_oz, d_os = i32(n_out), i32(n_out), i32(n_out), i32(n_out)
            src = torch.zeros(max(P * per_peer * SIZE, 1), dtype=torch.uint8, device="cuda")
            dst = torch.zeros_like(src)

            def restore():
                if per_peer:
                    st.len.copy_(d_len0), st.head.copy_(d_head0)

            def release():
                restore()
                staged.release_batch(dev, NOW, d_table, d_kp, d_nonce, LIMIT, d_rekey, st, n_out, d_out, d_op, d_oc, d_oz, d_os,
                                     d_n_out, d_status, d_work, stream=stream, n_keys=n_keys)

            release()
            torch.cuda.synchronize()
            hk = dict(out=np.zeros(n_out * STRIDE, np.uint8), peer=np.zeros(n_out, np.uint32), count=np.zeros(n_out, np.int32),
                      sizes=np.zeros(n_out, np.int32), status=np.zeros(n_out, np.int32))
            h_n, h_status = np.zeros(1, np.uint32), np.zeros(P, np.int32)
            t0 = time.perf_counter()
            staged.release_host(NOW, w["table"], w["kp"], w["send_nonce"], LIMIT, w["rekey"].copy(), h, n_out, hk["out"], hk["peer"],
                                hk["count"], hk["sizes"], hk["status"], h_n, h_status)
            host_us = round((time.perf_counter() - t0) * 1e6, 1)
            assert down(d_n_out, np.uint32)[0] == h_n[0] == P * per_peer and down(d_status, np.int32)[:P].tobytes() == h_status.tobytes()
            assert down(d_out, np.uint8).tobytes() == hk["out"].tobytes() and down(d_oz, np.int32)[:n_out].tobytes() == hk["sizes"].tobytes()
            print(json.dumps(dict(base, variant=variant + "_host_one_core", us_per_call=host_us)), flush=True)
            rounds(dict(base, packets=P * per_peer, bytes=P * per_peer * SIZE),
                   [(variant, release), (variant + "_restore_alone", restore)] +
                   ([(variant + "_plain_copy_same_bytes", lambda: dst.copy_(src))] if per_peer else []))
    else:
        n, r = 64, 7  # 64 jobs of peer row r, which has no keypair until the handshake completes
        rng = np.random.default_rng(20261203)
        jb = make_jobs(n, 1)
        jb["peer"][:] = w["table"]["peer"][r]
        kp_none = w["kp"].copy()
        kp_none["current"][r] = (0, 0, 0, 0, 0)
        d_kp_none, d_kp_set = up(kp_none), up(w["kp"])
        keys = np.frombuffer(rng.bytes(48 * n_keys), AEAD_KEY_DTYPE).copy()
        d_keys = up(keys)
        d = {k: up(v) for k, v in jb.items()}
        d_work = torch.zeros(keystate.work_bytes(max(n, P)), dtype=torch.uint8, device="cuda")
        d_where, d_gate, d_pkts, d_nbufs, d_key, d_len = i32(n), i32(n), torch.zeros(24 * n, dtype=torch.uint8, device="cuda"), i32(n), i32(n), i32(n)
        st = device_state(staged.state(P, CAP, STRIDE))
        d_out = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
        d_op, d_oc, d_oz, d_os, d_n_out, d_status = i32(n), i32(n), i32(n), i32(n), i32(1), i32(P)
        d_again = torch.zeros_like(d["arena"])
        pinned = torch.from_numpy(jb["arena"].copy()).pin_memory()

        def front(arena, peer, count, status_in, sizes, jobs, seal):
            rekey.send_gate_batch(dev, peer, count, status_in, 1, NOW, d_rows, d_kp, d_nonce, LIMIT, d_rekey, d_gate, stream=stream,
                                  n_jobs=jobs, n_ids=P, n_peers=P, n_keys=n_keys)
            keystate.send_assign_batch(dev, sizes, peer, count, d_gate, 1, STRIDE, d_peer_keys, d_nonce, d_pkts, d_nbufs, d_key,
                                       d_work, stream=stream, n_jobs=jobs, n_slots=n_slots, n_keys=n_keys)
            rekey.sent_batch(dev, peer, count, d_gate, d_key, 1, NOW, d_rows, d_kp, d_nonce, LIMIT, d_rekey, stream=stream,
                             n_jobs=jobs, n_ids=P, n_peers=P, n_keys=n_keys)
            if seal:
                transport.seal_batch(dev, arena, d_pkts, d_keys, MTU, d_len, stream=stream, n=jobs, n_keys=n_keys)

        def on_device():
            d_kp.copy_(d_kp_none), d_nonce.zero_()
            front(d["arena"], d["peer"], d["count"], d["status_in"], d["sizes"], n, False)
            staged.stage_batch(dev, d["arena"], d["sizes"], d["peer"], d["count"], d["status_in"], d_gate, d_key, 1, d_rows, st,
                               d_where, d_work, stream=stream, n_jobs=n, n_ids=P)
            d_kp.copy_(d_kp_set)  # the handshake completes
            staged.release_batch(dev, NOW, d_table, d_kp, d_nonce, LIMIT, d_rekey, st, n, d_out, d_op, d_oc, d_oz, d_os, d_n_out,
                                 d_status, d_work, stream=stream, n_keys=n_keys)
            front(d_out, d_op, d_oc, d_os, d_oz, n, True)

        def parents_way():
            d_kp.copy_(d_kp_none), d_nonce.zero_()
            front(d["arena"], d["peer"], d["count"], d["status_in"], d["sizes"], n, False)
            torch.cuda.synchronize()
            refused = d_gate.cpu().numpy()[:n] == ERR_KEY_EXPIRED  # the host reads the statuses and keeps the jobs
            assert refused.all()
            d_kp.copy_(d_kp_set)  # the handshake completes
            d_again.copy_(pinned, non_blocking=True)  # the host submits the same jobs again
            front(d_again, d["peer"], d["count"], d["status_in"], d["sizes"], n, True)

        on_device()
        torch.cuda.synchronize()
        assert down(d_n_out, np.uint32)[0] == n and (down(d_len, np.int32)[:n] >= SIZE + 32).all()
        rounds(dict(base, jobs=n), [("stage_release_on_one_stream", on_device), ("sync_read_resubmit", parents_way)], timer=wall)
    dev.close()


if __name__ == "__main__":
    main()
