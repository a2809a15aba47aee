"""Cookie generator measurement: wgcs_cookie_consume_batch,
wgcs_cookie_initiated_batch and the retry chain with the new launch in it, on
one MI355X, each beside its comparisons in the same process, alternating.  Not
part of bench.py.

  python -m wireguard_amd.cookiegen_bench --mode consume|sent|chain [--steps 200 --warmup 10]

  consume  65,536 and 1,024 rows, every row a reply that opens, over 1,024 peers
           and over one peer (every row then claims one row of the table).
           Beside it wgcs_handshake_screen_batch under load at the same row count
           (cookie_bench's batch: the nearest existing kernel by work per lane)
           and wgcs_cookie_consume_reply on one host core.
  sent     wgcs_cookie_initiated_batch over 65,536 and 1,024 descriptors and
           1,024 peers beside wgcs_timers_initiated_batch over the same tickets.
  chain    expire -> start -> initiate -> timers_initiated -> cookie_initiated
           over 1,024 peers, 1,024 and 64 of them due, beside the same chain
           without the last call (the parent commit's calls).
The device's tables and verdicts are compared with the host forms' before
anything is timed.  Prints one JSON line per row count and variant.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import time

import numpy as np

from . import _lib, cookie, keystate, noise, rekey, router, timers
from . import cookiegen as cg
from ._lib import HS_COOKIE, HS_COOKIE_KEPT, HS_INITIATED
from .cookie_bench import make_batch
from .noise import HS_PEER_DTYPE, HS_START_DTYPE, HS_STATE_DTYPE
from .rekey_bench import NOW, SECOND, make_tickets, make_world
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

SEED = 20261221
PITCH = 66  # replies 66 bytes apart: offsets 0 and 2 mod 4


def reply_world(n_peers: int, seed: int = 20261220):
    """n_peers peers that each hold a lastMAC1 and a handshake in flight (index 0x500000 + r -> state row r),
    and one reply per peer that opens."""
    rng = np.random.default_rng(seed)
    table = np.zeros(n_peers, noise.PEER_KEY_DTYPE)
    table["public_key"] = rng.integers(0, 256, (n_peers, 32), dtype=np.uint8)
    table["peer"] = np.arange(n_peers)
    gen = cg.gen_build(table)
    gen["last_mac1"] = rng.integers(0, 256, (n_peers, 16), dtype=np.uint8)
    gen["flags"] = cg.COOKIE_GEN_HAS_MAC1
    r = np.arange(n_peers, dtype=np.uint32)
    states = np.zeros(n_peers, HS_STATE_DTYPE)
    states["state"], states["local_index"], states["peer_row"], states["claim"] = 1, 0x500000 + r, r, 0xFFFFFFFF
    hs_slots = router.session_table(0x500000 + r, r)
    peers = np.zeros(n_peers, HS_PEER_DTYPE)
    peers["claim"] = 0xFFFFFFFF
    replies = []
    for p in range(n_peers):  # sealed by CreateReply of a responder whose static key is the peer's
        ck = cookie.checker_init(table["public_key"][p].tobytes(), rng.bytes(32))
        msg = b"\x01\0\0\0" + int(0x500000 + p).to_bytes(4, "little") + bytes(108) + gen["last_mac1"][p].tobytes() + bytes(16)
        replies.append(cookie.create_reply(ck, msg, cookie.src_addr("10.0.0.1", 7), rng.bytes(24)))
    return dict(table=table, gen=gen, states=states, hs_slots=hs_slots, peers=peers,
                peer_rows=noise.peer_rows_build(table, n_peers)), replies


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("consume", "sent", "chain"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("cookiegen_bench: no GPU (this measurement does not fall back)")
    dev = Device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

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

    def med(rounds, i):
        return float(np.median([r[i] for r in rounds]))

    base = {"steps": args.steps, "warmup": args.warmup}
    timing = "HIP events around K calls, three rounds, the variants alternating in one process"
    P = 1024

    if args.mode == "consume":
        w, replies = reply_world(P)
        no_slots, no_keys = np.zeros(0, router.SESSION_SLOT_DTYPE), np.zeros(0, np.uint32)
        L = _lib.load()
        for n in (65536, 1024):
            # the yardstick: the screen under load over cookie_bench's batch at this row count
            ck, s_arena, s_pkts, s_src, s_nonce, _ = make_batch(n)
            ds = [up(x) for x in (s_arena, s_pkts, ck, s_src, s_nonce)]
            d_stype, d_sverdict = torch.ones(n, dtype=torch.int32, device="cuda"), i32(n)
            d_sreply = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")

            def screen():
                cookie.screen_batch(dev, ds[0], ds[1], d_stype, ds[2], ds[3], d_sverdict, under_load=True, nonce=ds[4],
                                    reply=d_sreply, stream=stream, n=n)

            for variant, distinct in (("1024_peers", P), ("one_peer", 1)):
                arena = np.zeros(n * PITCH + 8, np.uint8)
                pkts = np.zeros(n, AEAD_PKT_DTYPE)
                pkts["off"], pkts["len"], pkts["key"] = np.arange(n, dtype=np.uint64) * np.uint64(PITCH), 64, 0xFFFFFFFF
                rows = np.frombuffer(b"".join(replies[q % distinct] for q in range(n)), np.uint8).reshape(n, 64)
                arena[:n * PITCH].reshape(n, PITCH)[:, :64] = rows
                types = np.full(n, 3, np.int32)
                gen, peers = w["gen"].copy(), w["peers"].copy()
                want = cg.consume_host(arena, pkts, types, NOW, w["hs_slots"], w["states"], no_slots, no_keys, w["peer_rows"],
                                       gen, peers)
                assert (want == HS_COOKIE_KEPT).all()
                d_arena, d_pkts, d_types = up(arena), up(pkts), up(types)
                d_hs, d_states, d_rows = up(w["hs_slots"]), up(w["states"]), up(w["peer_rows"])
                d_gen, d_peers = up(w["gen"]), up(w["peers"])
                d_work, d_verdict = torch.zeros(16 * n, dtype=torch.uint8, device="cuda"), i32(n)

                def consume():
                    cg.consume_batch(dev, d_arena, d_pkts, d_types, NOW, d_hs, d_states, None, None, d_rows, d_gen, d_peers,
                                     d_work, d_verdict, stream=stream, n=n, n_hs_slots=len(w["hs_slots"]), n_states=P,
                                     n_slots=0, n_keys=0, n_ids=P, n_peers=P)

                consume(), screen()
                torch.cuda.synchronize()
                assert d_verdict.cpu().numpy().tolist() == want.tolist() and bool((d_sverdict == HS_COOKIE).all())
                assert d_gen.cpu().numpy().tobytes() == gen.tobytes() and d_peers.cpu().numpy().tobytes() == peers.tobytes()
                assert not bool(d_work.any()), "a cookie was left in d_work"
                # one host core: ConsumeReply per row through the C ABI's host function
                count, out = min(n, 8192), C.create_string_buffer(16)
                keys = [w["gen"]["cookie_key"][q % distinct].tobytes() for q in range(count)]
                macs = [w["gen"]["last_mac1"][q % distinct].tobytes() for q in range(count)]
                t0 = time.perf_counter()
                for q in range(count):
                    if L.wgcs_cookie_consume_reply(keys[q], macs[q], replies[q % distinct], out) != 1:
                        raise SystemExit("cookiegen_bench: the host function did not open a reply")
                host_us = (time.perf_counter() - t0) / count * 1e6
                rounds = [(events(consume), events(screen)) for _ in range(3)]
                us = med(rounds, 0)
                print(json.dumps({**base, "metric": "cookie_consume_us", "unit": "us", "rows": n, "variant": variant,
                                  "value": us, "consume_us": [r[0] for r in rounds],
                                  "screen_under_load_us_same_rows": [r[1] for r in rounds],
                                  "consume_over_screen": round(us / med(rounds, 1), 3),
                                  "replies_per_s": round(n / (us * 1e-6)),
                                  "host_one_core": {"us_per_reply": round(host_us, 3), "replies": count,
                                                    "path": "wgcs_cookie_consume_reply, one ctypes call per reply",
                                                    "device_over_host": round(n / us * host_us, 1)},
                                  "kernel": "each_kernel<CookieOpen> + each_kernel<CookieCommit>", "timing": timing}),
                      flush=True)
        return

    if args.mode == "sent":
        for n in (65536, 1024):
            rng = np.random.default_rng(SEED + n)
            start = np.zeros(n, HS_START_DTYPE)
            start["peer_row"] = np.arange(n) % P
            status = np.full(n, HS_INITIATED, np.int32)
            msgs = rng.integers(0, 256, n * 160, dtype=np.uint8)
            gen = cg.gen_build(np.zeros(P, noise.PEER_KEY_DTYPE))
            d_start, d_status, d_msgs, d_gen = up(start), up(status), up(msgs), up(gen)
            cg.initiated_host(start, status, msgs, gen)
            reasons, start_peer = np.full(P, rekey.REKEY_WANT_NO_KEYPAIR, np.uint32), start["peer_row"].astype(np.uint32)
            d_reasons, d_sp, d_timers = up(reasons), up(start_peer), up(timers.timers_table(P, 25))

            def c_sent():
                cg.initiated_batch(dev, d_start, d_status, d_msgs, d_gen, stream=stream, n=n, n_peers=P)

            def t_sent():
                timers.initiated_batch(dev, d_reasons, d_sp, d_status, NOW, SEED, d_timers, stream=stream, n_tickets=n,
                                       n_peers=P)

            c_sent(), t_sent()
            torch.cuda.synchronize()
            assert d_gen.cpu().numpy().tobytes() == gen.tobytes(), "cookie_initiated differs from the host form"
            rounds = [(events(c_sent), events(t_sent)) for _ in range(3)]
            print(json.dumps({**base, "metric": "cookie_initiated_us", "unit": "us", "rows": n, "peers": P,
                              "value": med(rounds, 0), "cookie_initiated_us": [r[0] for r in rounds],
                              "timers_initiated_us_same_tickets": [r[1] for r in rounds],
                              "kernel": "each_kernel<CookieSentClaim> + each_kernel<CookieSentCommit> (two launches, "
                                        "as timers_initiated's two)", "timing": timing}), flush=True)
        return

    w = make_world(P)
    d = {k: up(v) for k, v in w.items()}
    d_keys = up(np.zeros(2 * P, AEAD_KEY_DTYPE))
    d_work = torch.zeros(keystate.work_bytes(P), dtype=torch.uint8, device="cuda")
    gen0 = cg.gen_build(w["table"])
    for due in (1024, 64):
        t0 = timers.timers_table(P, 25)
        t0["pending"][:due], t0["deadline_ns"][:due, 1], t0["attempts"][:due] = 0b00010, NOW - SECOND, 1
        now = NOW + 10 * SECOND  # past RekeyTimeout of the tables' lastSentHandshake
        d0, d_timers, d_rekey0, d_gen = up(t0), up(t0), up(w["rekey"]), up(gen0)
        ka = dict(ka_peer=i32(due), ka_count=i32(due), ka_sizes=i32(due), ka_status=i32(due), n_ka=i32(1), actions=i32(P))
        d_tickets, d_start, d_sp, d_n = up(make_tickets(due)), torch.zeros(96 * due, dtype=torch.uint8, device="cuda"), i32(due), i32(1)
        d_sstatus, d_reasons = i32(P), i32(P)
        d_states = torch.zeros(128 * due, dtype=torch.uint8, device="cuda")
        d_msgs, d_istatus = torch.zeros(160 * due, dtype=torch.uint8, device="cuda"), i32(due)

        def parent_chain():
            d_timers.copy_(d0), d["rekey"].copy_(d_rekey0)
            timers.expire_batch(dev, now, d_timers, d["rekey"], d["table"], None, d["kp"], None, d["peer_keys"], d_keys,
                                d["key_peer"], ka["ka_peer"], ka["ka_count"], ka["ka_sizes"], ka["ka_status"], ka["n_ka"],
                                ka["actions"], d_work, stream=stream, n_peers=P, n_slots=0, n_peer_slots=len(w["peer_keys"]),
                                n_keys=2 * P, n_ka_max=due)
            rekey.start_batch(dev, now, d["rekey"], d["hs_peers"], d_tickets, d_start, d_sp, d_n, d_sstatus, d_reasons, d_work,
                              stream=stream, n_peers=P, n_tickets=due)
            noise.initiate_batch(dev, d_start, d["own_public"], d["table"], d_states, d_msgs, d_istatus, 2 * P, stream=stream,
                                 n=due, n_peers=P, n_states=due)
            timers.initiated_batch(dev, d_reasons, d_sp, d_istatus, now, SEED, d_timers, stream=stream, n_tickets=due,
                                   n_peers=P)

        def chain():
            parent_chain()
            cg.initiated_batch(dev, d_start, d_istatus, d_msgs, d_gen, stream=stream, n=due, n_peers=P)

        chain()
        torch.cuda.synchronize()
        gen, istatus = gen0.copy(), d_istatus.cpu().numpy()
        assert int(d_n.cpu().numpy()[0]) == due and istatus[:due].tolist() == [HS_INITIATED] * due
        cg.initiated_host(d_start.cpu().numpy().view(HS_START_DTYPE), istatus[:due], d_msgs.cpu().numpy(), gen)
        assert d_gen.cpu().numpy().tobytes() == gen.tobytes() and int(gen["flags"].sum()) == due
        rounds = [(events(chain), events(parent_chain)) for _ in range(3)]
        print(json.dumps({**base, "metric": "cookie_chain_us", "unit": "us", "peers": P, "due_peers": due,
                          "value": med(rounds, 0), "chain_us": [r[0] for r in rounds],
                          "parent_chain_us": [r[1] for r in rounds],
                          "added_us": round(med(rounds, 0) - med(rounds, 1), 2),
                          "chain": "restore (two table copies), expire, start, initiate, timers_initiated, cookie_initiated",
                          "parent_chain": "the same without cookie_initiated", "timing": timing}), flush=True)


if __name__ == "__main__":
    main()
