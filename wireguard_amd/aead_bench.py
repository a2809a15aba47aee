"""Transport AEAD measurement: the
device-resident wgcs_aead_seal_batch / wgcs_aead_open_batch on one MI355X.

  python -m wireguard_amd.aead_bench --mode seal|open [--steps 20 --warmup 5]

Workload: 65,536 packets of 1,420 B (random bytes behind an IPv4 header whose
total length is 1,420), mtu 1420, so 1,452-B transport messages packed back to
back (95 MB per arena).  The arena exists in >= 4 copies that the launches
rotate over, so no launch finds its bytes in the 256 MB last-level cache.  One
enqueue of K launches sits between a HIP event pair, after W warmup launches.
Open works in place and a message opens only once, so every open launch gets a
freshly sealed copy: the timed launches run in chunks of at most --open-copies
and the copies are restored from a sealed master between chunks, outside the
event pairs.

Prints one JSON line: plaintext GiB/s, us per launch, the share of 8 TB/s that
the bytes read + written amount to, the VALU ceiling (the kernel's own
instruction count from scripts/aead_valu_count.py, a 64-bit multiply-add at
four issue slots, over 256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz) and,
as context, one CPU core of the local OpenSSL on the same bytes when present.
"""
from __future__ import annotations

import argparse
import ctypes as C
import ctypes.util
import importlib.util
import json
import os
import struct
import time

import numpy as np

from . import transport
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0
N_CU, SIMDS, LANES_PER_CYCLE, CLOCK_HZ = 256, 4, 32, 2.4e9  # VALU ceiling: guide figures for the MI355X
PKT, MTU = 1420, 1420
MSG = 16 + PKT + 16
N_KEYS = 8


def make_arena(n: int, seed: int = 20261019):
    rng = np.random.default_rng(seed)
    arena = rng.integers(0, 256, n * MSG, dtype=np.uint8)
    a = arena.reshape(n, MSG)
    a[:, 16] = 0x45  # IPv4, total length PKT: open's trim keeps the whole packet
    a[:, 18] = PKT >> 8
    a[:, 19] = PKT & 0xFF
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    pkts["off"] = np.arange(n, dtype=np.uint64) * np.uint64(MSG)
    pkts["counter"] = np.arange(n, dtype=np.uint64) + np.uint64(1 << 32)
    pkts["len"] = PKT
    pkts["key"] = np.arange(n) % N_KEYS
    keys = np.zeros(N_KEYS, AEAD_KEY_DTYPE)
    keys["key"] = rng.integers(0, 256, (N_KEYS, 32), dtype=np.uint8)
    keys["remote_index"] = np.arange(N_KEYS) + 0x1000
    return arena, pkts, keys


class _Evp:
    """EVP_chacha20_poly1305 seal of the local OpenSSL (context and spot check only)."""

    def __init__(self):
        path = ctypes.util.find_library("crypto")
        if not path:
            raise OSError("no libcrypto")
        L = C.CDLL(path)
        vp, i = C.c_void_p, C.c_int
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        L.EVP_chacha20_poly1305.restype = vp
        L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, C.c_char_p, C.c_char_p]
        L.EVP_EncryptUpdate.argtypes = [vp, C.c_char_p, C.POINTER(i), C.c_char_p, i]
        L.EVP_EncryptFinal_ex.argtypes = [vp, C.c_char_p, C.POINTER(i)]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, i, i, vp]
        self.L, self.ctx = L, L.EVP_CIPHER_CTX_new()
        self.out, self.tag, self.n = C.create_string_buffer(65536 + 16), C.create_string_buffer(16), C.c_int(0)
        if L.EVP_EncryptInit_ex(self.ctx, L.EVP_chacha20_poly1305(), None, None, None) != 1:
            raise OSError("EVP_chacha20_poly1305 unavailable")

    def seal(self, key: bytes, counter: int, pt: bytes) -> bytes:
        L, n = self.L, self.n
        L.EVP_EncryptInit_ex(self.ctx, None, None, key, b"\0\0\0\0" + struct.pack("<Q", counter))
        L.EVP_EncryptUpdate(self.ctx, self.out, C.byref(n), pt, len(pt))
        L.EVP_EncryptFinal_ex(self.ctx, self.tag, C.byref(n))
        L.EVP_CIPHER_CTX_ctrl(self.ctx, 0x10, 16, self.tag)
        return self.out.raw[:len(pt)] + self.tag.raw


def libcrypto_context(arena, pkts, keys, count: int = 4096):
    """One core of OpenSSL sealing the first `count` packets: (plaintext GiB/s,
    the sealed messages of the first 4 for the spot check) or (None, None)."""
    try:
        evp = _Evp()
    except (OSError, AttributeError):
        return None, None
    count = min(count, len(pkts))
    a = arena.reshape(-1, MSG)
    pts = [a[i, 16:16 + PKT].tobytes() for i in range(count)]
    kb = [keys[k]["key"].tobytes() for k in range(N_KEYS)]
    ctr = [int(c) for c in pkts["counter"][:count]]
    t0 = time.perf_counter()
    out = [evp.seal(kb[i % N_KEYS], ctr[i], pts[i]) for i in range(count)]
    el = time.perf_counter() - t0
    msgs = [struct.pack("<IIQ", 4, int(keys[i % N_KEYS]["remote_index"]), ctr[i]) + out[i] for i in range(4)]
    return count * PKT / el / 2**30, msgs


def valu_ceiling(mode: str, slots: int | None):
    """(issue slots per 16 B per lane, ceiling in plaintext GiB/s, how counted)."""
    how = "given on the command line"
    if slots is None:
        path = os.path.join(ROOT, "scripts", "aead_valu_count.py")
        spec = importlib.util.spec_from_file_location("aead_valu_count", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        rec = mod.loop_cost(mod.census(mod.kernels(mod.assembly())[mode.upper()]))
        slots, how = rec["issue_slots"], f"scripts/aead_valu_count.py: {json.dumps(rec)}"
    # a lane turns 16 message bytes per `slots` issue slots; of a 1452-B message 1420 B are plaintext,
    # and the 91 chunks + length block take 6 trips of a 16-lane row (96 lane-trips for 92 blocks)
    lane_slots_per_s = N_CU * SIMDS * LANES_PER_CYCLE * CLOCK_HZ
    trips = -(-(-(-PKT // 16) + 1) // 16)
    bytes_per_s = lane_slots_per_s / (slots * trips * 16) * PKT
    return slots, bytes_per_s / 2**30, how


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("seal", "open"), required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--packets", type=int, default=65536)
    ap.add_argument("--copies", type=int, default=4, help="seal: arena copies the launches rotate over (>= 4)")
    ap.add_argument("--open-copies", type=int, default=32, help="open: freshly sealed copies per timed chunk")
    ap.add_argument("--valu-slots", type=int, default=None,
                    help="VALU issue slots per loop trip, if already counted (default: count now with hipcc)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.copies < 4 or args.steps < 1 or args.warmup < 0:
        ap.error("--copies >= 4, --steps >= 1, --warmup >= 0")

    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("aead_bench: no GPU (this measurement does not fall back)")
    torch.cuda.set_device(args.device)
    dev = Device(args.device)
    n = args.packets
    arena, pkts, keys = make_arena(n)
    cpu_gibs, cpu_msgs = libcrypto_context(arena, pkts, keys)
    d_plain = torch.from_numpy(arena).cuda()
    d_pkts = torch.from_numpy(pkts.view(np.uint8).reshape(-1)).cuda()
    opk = pkts.copy()
    opk["len"] = MSG
    d_opkts = torch.from_numpy(opk.view(np.uint8).reshape(-1)).cuda()
    d_keys = torch.from_numpy(keys.view(np.uint8).reshape(-1)).cuda()
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ctr = torch.zeros(n, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def seal(buf):
        transport.seal_batch(dev, buf, d_pkts, d_keys, MTU, d_len, stream=stream, n=n, n_keys=N_KEYS)

    def open_(buf):
        transport.open_batch(dev, buf, d_opkts, d_keys, d_len, d_ctr, stream=stream, n=n, n_keys=N_KEYS)

    d_sealed = d_plain.clone()
    seal(d_sealed)
    torch.cuda.synchronize()
    assert bool((d_len == MSG).all()), "seal status"
    if cpu_msgs is not None:  # the device agrees with OpenSSL on the first messages
        head = d_sealed[:4 * MSG].cpu().numpy().tobytes()
        assert [head[i * MSG:(i + 1) * MSG] for i in range(4)] == cpu_msgs, "device seal != OpenSSL"

    if args.mode == "seal":
        # sealing what is already sealed is the same work (the kernel's path does not depend on the bytes)
        copies = [d_plain] + [d_plain.clone() for _ in range(args.copies - 1)]
        for k in range(args.warmup):
            seal(copies[k % len(copies)])
        e0.record(stream)
        for k in range(args.steps):
            seal(copies[(args.warmup + k) % len(copies)])
        e1.record(stream)
        torch.cuda.synchronize()
        ms_total = e0.elapsed_time(e1)
        assert bool((d_len == MSG).all()), "seal status"
        nbuf = len(copies)
    else:
        nbuf = max(4, min(args.open_copies, max(args.steps, args.warmup)))
        copies = [d_sealed.clone() for _ in range(nbuf)]

        def restore():
            for c in copies:
                c.copy_(d_sealed)
            torch.cuda.synchronize()
        for k in range(min(args.warmup, nbuf)):
            open_(copies[k])
        torch.cuda.synchronize()
        assert bool((d_len == PKT).all()), "open status"
        assert torch.equal(copies[0][16:16 + PKT], d_plain[16:16 + PKT]) if args.warmup else True
        ms_total, done = 0.0, 0
        while done < args.steps:
            restore()
            chunk = min(nbuf, args.steps - done)
            e0.record(stream)
            for k in range(chunk):
                open_(copies[k])
            e1.record(stream)
            torch.cuda.synchronize()
            ms_total += e0.elapsed_time(e1)
            done += chunk
        assert bool((d_len == PKT).all()), "open status"
        assert bool((d_ctr == torch.from_numpy(pkts["counter"].astype(np.int64)).cuda()).all()), "open counters"

    ms = ms_total / args.steps
    plaintext = n * PKT
    moved = n * (PKT + MSG)  # seal reads the packet and writes the message; open the reverse
    gibs = plaintext / (ms * 1e-3) / 2**30
    slots, ceil_gibs, how = valu_ceiling(args.mode, args.valu_slots)
    res = {
        "metric": f"aead_{args.mode}_plaintext_gibs", "value": round(gibs, 2), "unit": "GiB/s",
        "us_per_launch": round(ms * 1e3, 2), "steps": args.steps, "warmup": args.warmup,
        "workload": {"packets": n, "packet_bytes": PKT, "message_bytes": MSG, "mtu": MTU, "keys": N_KEYS,
                     "arena_copies": nbuf, "arena_bytes": n * MSG},
        "kernel": f"aead_batch_kernel<{args.mode.upper()}>",
        "hbm": {"bytes_read_plus_written_per_launch": moved,
                "share_of_8tbs": round(moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
        "valu": {"issue_slots_per_trip": slots, "mad64_issue_slots": 4, "counted": how,
                 "ceiling_plaintext_gibs": round(ceil_gibs, 1), "measured_over_ceiling": round(gibs / ceil_gibs, 3),
                 "assumes": f"{N_CU} CUs x {SIMDS} SIMDs x {LANES_PER_CYCLE} lanes/cycle at {CLOCK_HZ / 1e9} GHz"},
        "libcrypto_one_core_gibs": None if cpu_gibs is None else round(cpu_gibs, 3),
    }
    print(json.dumps(res), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
