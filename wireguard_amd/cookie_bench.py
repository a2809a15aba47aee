"""Handshake-screen measurement: the
device-resident wgcs_handshake_screen_batch on one MI355X.

  python -m wireguard_amd.cookie_bench --mode mac1|load [--steps 20 --warmup 5]

Workload: 65,536 initiations of 148 B with a valid MAC1, each at an odd byte
offset of one arena (pitch 150), from IPv4 and IPv6 sources in turn.
  mac1   under_load = 0: one MAC1 per message (three BLAKE2s compressions)
  load   under_load = 1 and no message carries a MAC2: MAC1, the cookie, MAC2
         and the sealed cookie reply for every message (nine compressions, three
         ChaCha20 permutations, Poly1305 over three blocks)
One enqueue of K launches sits between a HIP event pair, after W warmup
launches; the kernel only reads its inputs, so every launch does the same work.

Prints one JSON line: us per launch and messages per second, the VALU-issue
ceiling of DESIGN §4.13 (the guide's figures, named as assumptions), and in the
same line the host functions of the C ABI (wgcs_cookie_check_mac1, and in load
mode wgcs_cookie_check_mac2 and wgcs_cookie_create_reply) on one CPU core over
the same messages, called through ctypes.  The device's verdicts and replies
are checked against those host results before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import struct
import time

import numpy as np

from . import _lib, cookie
from .cookie import COOKIE_CHECKER_DTYPE, SRC_ADDR_DTYPE
from .transport import AEAD_PKT_DTYPE

MSG, PITCH = 148, 150
N_CU, SIMDS, LANES_PER_CYCLE, CLOCK_HZ = 256, 4, 32, 2.4e9  # VALU ceiling: guide figures for the MI355X
# VALU issue slots per message, worked out in DESIGN §4.13
VALU_SLOTS = {"mac1": 3 * 1150 + 600, "load": 9 * 1150 + 3 * 1000 + 600 + 1400}


def make_batch(n: int, seed: int = 20261020):
    rng = np.random.default_rng(seed)
    ck = cookie.checker_init(rng.bytes(32), rng.bytes(32))
    mac1_key = ck["mac1_key"][0].tobytes()
    arena = np.zeros(n * PITCH + 64, np.uint8)
    body = rng.integers(0, 256, (n, MSG), dtype=np.uint8)
    body[:, 0:4] = np.frombuffer(struct.pack("<I", 1), np.uint8)
    body[:, MSG - 32:] = 0
    msgs = []
    for q in range(n):
        m, _ = cookie.add_macs(mac1_key, body[q].tobytes())
        msgs.append(m)
        arena[1 + q * PITCH:1 + q * PITCH + MSG] = np.frombuffer(m, np.uint8)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    pkts["off"] = 1 + np.arange(n, dtype=np.uint64) * np.uint64(PITCH)
    pkts["len"], pkts["key"] = MSG, 0xFFFFFFFF
    src = np.zeros(n, SRC_ADDR_DTYPE)
    src["b"] = rng.integers(0, 256, (n, 18), dtype=np.uint8)
    src["len"] = np.where(np.arange(n) % 2 == 0, 6, 18)
    src["b"][src["len"] == 6, 6:] = 0
    nonce = rng.integers(0, 256, n * 24, dtype=np.uint8)
    return ck, arena, pkts, src, nonce, msgs


def host_one_core(mode: str, ck, msgs, src, nonce, count: int):
    """(us per message, the replies of the first `count` messages) on one core."""
    L = _lib.load()
    count = min(count, len(msgs))
    ckp, out = ck.ctypes.data, C.create_string_buffer(64)
    srcp = [src[q:q + 1].ctypes.data for q in range(count)]
    nn = [nonce[24 * q:24 * q + 24].tobytes() for q in range(count)]
    replies = []
    t0 = time.perf_counter()
    for q in range(count):
        m = msgs[q]
        if L.wgcs_cookie_check_mac1(ckp, m, MSG) != 1:
            raise SystemExit("cookie_bench: host MAC1 mismatch")
        if mode == "load":
            if L.wgcs_cookie_check_mac2(ckp, m, MSG, srcp[q]) != 0:
                raise SystemExit("cookie_bench: host MAC2 matched")
            L.wgcs_cookie_create_reply(ckp, m, MSG, srcp[q], nn[q], out)
            replies.append(out.raw)
    el = time.perf_counter() - t0
    return el / count * 1e6, replies


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("mac1", "load"), required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--messages", type=int, default=65536)
    ap.add_argument("--host-messages", type=int, default=8192, help="messages the one-core host path is timed over")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0 or args.messages < 1:
        ap.error("--steps >= 1, --warmup >= 0, --messages >= 1")

    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("cookie_bench: no GPU (this measurement does not fall back)")
    torch.cuda.set_device(args.device)
    dev = Device(args.device)
    n, load = args.messages, args.mode == "load"
    ck, arena, pkts, src, nonce, msgs = make_batch(n)
    host_us, host_replies = host_one_core(args.mode, ck, msgs, src, nonce, args.host_messages)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_arena, d_pkts, d_ck, d_src, d_nonce = up(arena), up(pkts), up(ck), up(src), up(nonce)
    d_type = torch.ones(n, dtype=torch.int32, device="cuda")
    d_verdict = torch.full((n,), -99, dtype=torch.int32, device="cuda")
    d_reply = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def screen():
        cookie.screen_batch(dev, d_arena, d_pkts, d_type, d_ck, d_src, d_verdict, under_load=load, nonce=d_nonce,
                            reply=d_reply, stream=stream, n=n)

    screen()
    torch.cuda.synchronize()
    assert bool((d_verdict == (cookie.HS_COOKIE if load else cookie.HS_PASS)).all()), "verdicts"
    if load:  # the device agrees with the host functions on the replies
        head = d_reply[:64 * len(host_replies)].cpu().numpy().tobytes()
        assert head == b"".join(host_replies), "device replies != host replies"
    for _ in range(args.warmup):
        screen()
    e0.record(stream)
    for _ in range(args.steps):
        screen()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    slots = VALU_SLOTS[args.mode]
    ceiling = N_CU * SIMDS * LANES_PER_CYCLE * CLOCK_HZ / slots
    rate = n / (ms * 1e-3)
    res = {
        "metric": f"handshake_screen_{args.mode}_msgs_per_s", "value": round(rate), "unit": "messages/s",
        "us_per_launch": round(ms * 1e3, 2), "steps": args.steps, "warmup": args.warmup,
        "workload": {"messages": n, "message_bytes": MSG, "pitch": PITCH, "under_load": int(load),
                     "sources": "IPv4 and IPv6 in turn", "verdict": "COOKIE" if load else "PASS"},
        "kernel": "hs_screen_kernel",
        "valu": {"issue_slots_per_message": slots, "counted": "DESIGN §4.13", "ceiling_msgs_per_s": round(ceiling),
                 "measured_over_ceiling": round(rate / ceiling, 4),
                 "assumes": f"{N_CU} CUs x {SIMDS} SIMDs x {LANES_PER_CYCLE} lanes/cycle at {CLOCK_HZ / 1e9} GHz"},
        "host_one_core": {"us_per_message": round(host_us, 3), "msgs_per_s": round(1e6 / host_us),
                          "messages": min(args.host_messages, n),
                          "path": "the C ABI's host functions, one ctypes call per function and message",
                          "device_over_host": round(rate / (1e6 / host_us), 1)},
    }
    print(json.dumps(res), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
