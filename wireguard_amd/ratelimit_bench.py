"""Rate limiter measurement: wgcs_ratelimit_batch and
wgcs_ratelimit_cleanup_batch on one MI355X, each beside its comparisons in the
same process, alternating.  Not part of bench.py.

  python -m wireguard_amd.ratelimit_bench --mode allow|cleanup|chain [--steps 200 --warmup 10]

  allow    65,536 and 1,024 rows, every gate a pass, in a table of 2^18 slots,
           with four address mixes: every row an address of its own that the
           table does not know (a device memset empties the table before every
           call, inside the timed window, and is timed alone as well), every row
           an address of its own that it knows, 16 addresses, one address.  The
           clock moves 50 ms per call, so a known address passes one row a call.
           Beside it wgcs_ratelimit_batch_host on one core, and wgcs_replay_batch
           over 16,384 keys at the same row count (keystate_bench's workload;
           its filters zeroed before every call, as there): both calls are a
           kernel, the key order's sort and a kernel.
  cleanup  2^18 and 2^12 slots, a quarter of them live, with no entry idle and
           with half of them idle; wgcs_ratelimit_cleanup_host on one core
           beside it.
  chain    screen (under load) -> ratelimit -> consume on one stream over valid-MAC2
           initiations from 16 addresses, 65,536 and 1,024 rows, beside screen ->
           consume without the limiter: what the limiter keeps from the Noise code.
The device's verdicts and entries are compared with the host form's before
anything is timed.  Prints one JSON line per row count and variant.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np

from . import cookie, keystate, noise
from . import ratelimit as rl
from ._lib import HS_CONSUMED, HS_PASS
from .cookie import SRC_ADDR_DTYPE
from .keystate import REPLAY_FILTER_DTYPE
from .keystate_bench import deal_keys, replay_counters
from .transport import AEAD_PKT_DTYPE

NOW = 1_700_000_000_000_000_000
COST = rl.RL_PACKET_COST_NS


def addresses(n: int, distinct: int, port_of_row: bool = True) -> np.ndarray:
    """n SRC_ADDR_DTYPE rows over `distinct` IPv4 addresses 10.x.y.z, dealt round robin; the port is the
    row's (the limiter ignores it) or, for the screen, whose cookie covers it, the address's."""
    s = np.zeros(n, SRC_ADDR_DTYPE)
    ip = (0x0A000000 + np.arange(n, dtype=np.uint32) % distinct).astype(">u4")
    s["b"][:, :4] = ip.view(np.uint8).reshape(n, 4)
    port = np.arange(n) if port_of_row else np.arange(n) % distinct
    s["b"][:, 4:6] = (port & 0xFFFF).astype("<u2").view(np.uint8).reshape(n, 2)
    s["len"] = 6
    return s


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("allow", "cleanup", "chain"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("ratelimit_bench: no GPU (this measurement does not fall back)")
    dev = Device(0)
    # a stream of this bench's own for the launches and torch's fills alike
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

    if args.mode == "allow":
        n_slots = 1 << 18
        for n in (65536, 1024):
            work = torch.empty(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")
            gate = np.full(n, HS_PASS, np.int32)
            d_gate, d_verdict = up(gate), torch.zeros(n, dtype=torch.int32, device="cuda")
            d_stats = torch.zeros(4, dtype=torch.int32, device="cuda")
            # the yardstick: wgcs_replay_batch over 16,384 keys at this row count
            rng = np.random.default_rng(20261020 + 16384)
            n_keys = 16384
            keys = deal_keys(n, n_keys, rng)
            counter, _, _ = replay_counters(keys, n_keys, rng)
            pk = np.zeros(n, AEAD_PKT_DTYPE)
            pk["off"], pk["len"], pk["key"] = np.arange(n, dtype=np.uint64) * 1456, 1452, keys
            d_pk, d_ctr = up(pk), torch.from_numpy(counter.view(np.int64)).cuda()
            d_len = torch.full((n,), 1420, dtype=torch.int32, device="cuda")
            d_f = torch.zeros(n_keys * REPLAY_FILTER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_rv = torch.zeros(n, dtype=torch.int32, device="cuda")

            def replay():
                d_f.zero_()
                keystate.replay_batch(dev, d_pk, d_len, d_ctr, d_f, d_rv, work, stream=stream, n=n, n_keys=n_keys)

            for mix, distinct, known in (("distinct_new", n, False), ("distinct_known", n, True), ("16_addresses", 16, True),
                                         ("one_address", 1, True)):
                src = addresses(n, distinct)
                d_src = up(src)
                tab = rl.table(n_slots)
                if known:
                    rl.allow_host(gate, src, tab, NOW - 10 * COST)
                d_tab, clock = up(tab), [NOW]

                def call():
                    if not known:
                        d_tab.zero_()
                    clock[0] += COST
                    rl.allow_batch(dev, d_gate, d_src, d_tab, clock[0], d_verdict, work, stats=d_stats, stream=stream, n=n,
                                   n_slots=n_slots)

                def reset():
                    d_tab.zero_()

                # one call against the host form, then the host form on one core
                host_tab = rl.table(n_slots) if not known else tab.copy()
                t0 = time.perf_counter()
                want = rl.allow_host(gate, src, host_tab, NOW + COST)
                host_us = (time.perf_counter() - t0) * 1e6
                call()
                torch.cuda.synchronize()
                got_tab = d_tab.cpu().numpy().view(rl.RL_ENTRY_DTYPE)
                assert np.array_equal(d_verdict.cpu().numpy(), want), "allow_batch differs from the host form"
                assert rl.entries(got_tab) == rl.entries(host_tab), "the tables differ"
                passed = int((want == HS_PASS).sum())
                rounds = [(events(call), events(replay), events(reset) if not known else 0.0) for _ in range(3)]
                print(json.dumps({**base, "metric": "ratelimit_allow_us", "unit": "us", "rows": n, "mix": mix,
                                  "n_slots": n_slots, "value": med(rounds, 0), "allow_us": [r[0] for r in rounds],
                                  "replay_16384_keys_us_same_rows": [r[1] for r in rounds],
                                  "ratio_to_replay": round(med(rounds, 0) / med(rounds, 1), 3),
                                  "table_memset_us_inside_each_call": [r[2] for r in rounds],
                                  "host_one_core_us": round(host_us, 2), "passed_first_call": passed,
                                  "kernel": "rl_find_kernel + radix sort + heads_kernel + rl_position_kernel",
                                  "timing": timing}), flush=True)
        return

    if args.mode == "cleanup":
        for n_slots in (1 << 18, 1 << 12):
            live = n_slots // 4
            src = addresses(live, live)
            gate = np.full(live, HS_PASS, np.int32)
            for variant, idle in (("none_idle", 0), ("half_idle", live // 2)):
                tab = rl.table(n_slots)
                rl.allow_host(gate[:idle], src[:idle], tab, NOW - 1)
                rl.allow_host(gate[idle:], src[idle:], tab, NOW)
                d_old, d_new = up(tab), torch.empty(tab.nbytes, dtype=torch.uint8, device="cuda")
                d_live = torch.zeros(1, dtype=torch.int32, device="cuda")
                now = NOW + rl.RL_CLEANUP_NS

                def call():
                    rl.cleanup_batch(dev, d_old, d_new, now, d_live, stream=stream, n_slots=n_slots)

                t0 = time.perf_counter()
                want, want_live = rl.cleanup_host(tab, now)
                host_us = (time.perf_counter() - t0) * 1e6
                call()
                torch.cuda.synchronize()
                assert int(d_live.item()) == want_live == live - idle
                assert rl.entries(d_new.cpu().numpy().view(rl.RL_ENTRY_DTYPE)) == rl.entries(want), "the tables differ"
                rounds = [(events(call),) for _ in range(3)]
                print(json.dumps({**base, "metric": "ratelimit_cleanup_us", "unit": "us", "n_slots": n_slots,
                                  "variant": variant, "live_before": live, "kept": want_live, "value": med(rounds, 0),
                                  "cleanup_us": [r[0] for r in rounds], "host_one_core_us": round(host_us, 2),
                                  "kernel": "memset of the new table + rl_cleanup_kernel", "timing": timing}), flush=True)
        return

    # chain: 16 addresses, one authentic initiation with a valid MAC2 for each, dealt round robin over the rows
    rng = np.random.default_rng(20261021)
    responder, public = noise.responder_init(rng.bytes(32))
    checker = cookie.checker_init(public, rng.bytes(32))
    mac1_key, cookie_key = checker["mac1_key"][0].tobytes(), checker["cookie_key"][0].tobytes()
    publics, msgs = [], []
    for i in range(16):
        private = rng.bytes(32)
        msg = noise.create_initiation(private, public, rng.bytes(32), rng.bytes(12), i + 1)[0]
        with_mac1, mac1 = cookie.add_macs(mac1_key, msg)
        src = addresses(16, 16, port_of_row=False)[i:i + 1]
        ck = cookie.consume_reply(cookie_key, mac1, cookie.create_reply(checker, with_mac1, src, rng.bytes(24)))
        msgs.append(np.frombuffer(cookie.add_macs(mac1_key, msg, ck)[0], np.uint8))
        publics.append(noise.responder_init(private)[1])  # the public key of the initiator's static key
    table = noise.peer_keys_build(responder, publics, list(range(16)))
    d_responder, d_table, d_checker = up(responder), up(table), up(checker)
    for n in (65536, 1024):
        stride = 160
        arena = np.zeros(n * stride, np.uint8)
        for q in range(n):
            arena[q * stride:q * stride + 148] = msgs[q % 16]
        pk = np.zeros(n, AEAD_PKT_DTYPE)
        pk["off"], pk["len"] = np.arange(n, dtype=np.uint64) * stride, 148
        d_arena, d_pk, d_type = up(arena), up(pk), torch.ones(n, dtype=torch.int32, device="cuda")
        d_src, d_nonce = up(addresses(n, 16, port_of_row=False)), torch.zeros(24 * n, dtype=torch.uint8, device="cuda")
        d_reply = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        d_screen, d_limited, d_consumed = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
        d_init = torch.zeros(128 * n, dtype=torch.uint8, device="cuda")
        d_tab = up(rl.table(1 << 12))
        work = torch.empty(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")
        clock = [NOW]

        def screen():
            cookie.screen_batch(dev, d_arena, d_pk, d_type, d_checker, d_src, d_screen, under_load=True, nonce=d_nonce,
                                reply=d_reply, stream=stream, n=n)

        def with_limiter():
            screen()
            clock[0] += 5 * COST  # every bucket is full again: 5 rows of each address reach the Noise code
            rl.allow_batch(dev, d_screen, d_src, d_tab, clock[0], d_limited, work, stream=stream, n=n, n_slots=1 << 12)
            noise.consume_batch(dev, d_arena, d_pk, d_type, d_limited, d_responder, d_table, d_consumed, d_init,
                                stream=stream, n=n, n_peers=16)

        def without_limiter():
            screen()
            noise.consume_batch(dev, d_arena, d_pk, d_type, d_screen, d_responder, d_table, d_consumed, d_init,
                                stream=stream, n=n, n_peers=16)

        without_limiter()
        torch.cuda.synchronize()
        assert (d_screen.cpu().numpy() == HS_PASS).all() and (d_consumed.cpu().numpy() == HS_CONSUMED).all()
        with_limiter()
        torch.cuda.synchronize()
        reach = int((d_consumed.cpu().numpy() == HS_CONSUMED).sum())
        assert reach == min(n, 80) and int((d_limited.cpu().numpy() == rl.ERR_RATE_LIMITED).sum()) == n - reach
        rounds = [(events(with_limiter), events(without_limiter), events(screen)) for _ in range(3)]
        print(json.dumps({**base, "metric": "ratelimit_chain_us", "unit": "us", "rows": n, "addresses": 16,
                          "value": med(rounds, 0), "screen_ratelimit_consume_us": [r[0] for r in rounds],
                          "screen_consume_us": [r[1] for r in rounds], "screen_alone_us": [r[2] for r in rounds],
                          "rows_reaching_consume_with_limiter": reach, "rows_reaching_consume_without": n,
                          "timing": timing}), flush=True)


if __name__ == "__main__":
    main()
