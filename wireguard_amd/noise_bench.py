"""X25519, handshake-consume and handshake-respond measurement (DESIGN.md
§4.14, §4.15): the device-resident wgcs_x25519_batch,
wgcs_handshake_consume_batch and wgcs_handshake_respond_batch on one MI355X,
beside the same scalar code on one host core.

  python -m wireguard_amd.noise_bench --mode x25519|consume|respond [--rows 65536 --peers 1024 --steps 20 --warmup 3]

Workload:
  respond  `rows` descriptors over `--distinct` consumed initiations made on the
           host and tiled, no gate, every row runs the whole function: a fresh
           ephemeral key and session index each, a cookie on every other one, a
           preshared key for every other peer, key rows 2q and 2q + 1.  The line
           also carries three wgcs_x25519_batch launches of the same `rows`
           timed in the same process: the three ladders and nothing else, the
           floor for this kernel.
  x25519   `rows` random scalars and points, one scalar multiplication each
  consume  `rows` initiations of 148 B at odd byte offsets of one arena (pitch
           150), every row of type 1 with no gate, against a sorted table of
           `peers` public keys.  A fraction `--valid` (default one half) are
           authentic and run the whole function; the rest have one byte of
           their static field flipped and stop at the first open, having paid
           the X25519 and almost nothing else.  `--distinct` authentic messages
           are made on the host and tiled over the batch (the kernel does the
           same work for a repeated message: nothing is cached between lanes).
One enqueue of K launches sits between a HIP event pair, after W warmup
launches; the kernels only read their inputs, so every launch does the same
work.  The device's outputs are checked against the host functions before
anything is timed.

Prints one JSON line: us per launch and rows per second, and in the same line
the host functions of the C ABI (wgcs_x25519 / wgcs_noise_consume_initiation /
wgcs_noise_create_response) on one CPU core over the first `--host-rows` rows, called through ctypes, and
-- as context only -- the X25519 line of `openssl speed -seconds 1 ecdhx25519`
where that binary exists.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import shutil
import subprocess
import time

import numpy as np

from . import _lib, noise
from .noise import HS_INIT_DTYPE
from .transport import AEAD_PKT_DTYPE

MSG, PITCH = 148, 150
INITIATORS = 16


def openssl_speed() -> str | None:
    exe = shutil.which("openssl")
    if exe is None:
        return None
    try:
        r = subprocess.run([exe, "speed", "-seconds", "1", "ecdhx25519"], capture_output=True, text=True, timeout=60)
    except (OSError, subprocess.TimeoutExpired):
        return None
    lines = [ln.strip() for ln in r.stdout.splitlines() if "X25519" in ln or "x25519" in ln]
    return lines[-1] if lines else None


def make_x25519(n: int, seed: int = 20261021):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, 32 * n, dtype=np.uint8), rng.integers(0, 256, 32 * n, dtype=np.uint8)


def make_consume(n: int, n_peers: int, valid: float, distinct: int, seed: int = 20261021):
    rng = np.random.default_rng(seed)
    responder, pub = noise.responder_init(rng.bytes(32))
    privs = [rng.bytes(32) for _ in range(min(INITIATORS, n_peers))]
    keys = [noise.x25519(k, (9).to_bytes(32, "little")) for k in privs]
    keys += [rng.bytes(32) for _ in range(n_peers - len(keys))]  # peers that never call: any 32 bytes are a key
    table = noise.peer_keys_build(responder, keys, np.arange(n_peers, dtype=np.uint32))
    good = [noise.create_initiation(privs[i % len(privs)], pub, rng.bytes(32), rng.bytes(12), i)[0]
            for i in range(min(distinct, n))]
    n_valid = int(round(n * valid))
    is_valid = np.zeros(n, bool)
    is_valid[rng.permutation(n)[:n_valid]] = True
    arena = np.zeros(n * PITCH + 64, np.uint8)
    msgs = []
    for q in range(n):
        m = good[q % len(good)]
        if not is_valid[q]:
            m = m[:40 + q % 48] + bytes([m[40 + q % 48] ^ 0x80]) + m[41 + q % 48:]
        msgs.append(m)
        arena[1 + q * PITCH:1 + q * PITCH + MSG] = np.frombuffer(m, np.uint8)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    pkts["off"] = 1 + np.arange(n, dtype=np.uint64) * np.uint64(PITCH)
    pkts["len"], pkts["key"] = MSG, 0xFFFFFFFF
    return responder, table, arena, pkts, msgs, is_valid


def make_respond(n: int, n_peers: int, distinct: int, seed: int = 20261022):
    """`distinct` consumed initiations made on the host (wgcs_hs_init rows), and n
    descriptors over them: a fresh ephemeral key and index each, key rows 2q and
    2q + 1, a cookie on every other one, a preshared key for every other peer."""
    rng = np.random.default_rng(seed)
    responder, pub = noise.responder_init(rng.bytes(32))
    privs = [rng.bytes(32) for _ in range(min(INITIATORS, n_peers))]
    keys = [noise.x25519(k, (9).to_bytes(32, "little")) for k in privs]
    keys += [noise.x25519(rng.bytes(32), (9).to_bytes(32, "little")) for _ in range(n_peers - len(keys))]
    table = noise.peer_keys_build(responder, keys, np.arange(n_peers, dtype=np.uint32))
    rows = []
    for i in range(min(distinct, n)):
        msg = noise.create_initiation(privs[i % len(privs)], pub, rng.bytes(32), rng.bytes(12), i)[0]
        verdict, row = noise.consume_initiation(responder, table, msg)
        assert verdict == noise.HS_CONSUMED
        rows.append(row)
    init = np.concatenate(rows)
    row_of_peer = np.zeros(n_peers, np.uint32)
    row_of_peer[table["peer"]] = np.arange(n_peers, dtype=np.uint32)
    psk = rng.integers(0, 256, (n_peers, 32), dtype=np.uint8)
    psk[::2] = 0
    resp = np.zeros(n, noise.HS_RESP_DTYPE)
    resp["init_row"] = np.arange(n, dtype=np.uint32) % len(init)
    resp["peer_row"] = row_of_peer[init["peer"][resp["init_row"]]]
    resp["local_index"] = rng.integers(0, 2**32, n, dtype=np.uint32)
    resp["send_key"], resp["recv_key"] = 2 * np.arange(n, dtype=np.uint32), 2 * np.arange(n, dtype=np.uint32) + 1
    resp["flags"] = np.arange(n, dtype=np.uint32) & 1
    resp["ephemeral_private"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    resp["cookie"] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    return table, init, psk, resp


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("x25519", "consume", "respond"), required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--peers", type=int, default=1024, help="rows of the peer table (consume)")
    ap.add_argument("--valid", type=float, default=0.5, help="fraction of authentic initiations (consume)")
    ap.add_argument("--distinct", type=int, default=1024, help="authentic messages made on the host and tiled")
    ap.add_argument("--host-rows", type=int, default=512, help="rows the one-core host path is timed over")
    ap.add_argument("--no-openssl", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0 or args.rows < 1 or args.peers < 1 or not 0 <= args.valid <= 1:
        ap.error("--steps >= 1, --warmup >= 0, --rows >= 1, --peers >= 1, 0 <= --valid <= 1")

    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("noise_bench: no GPU (this measurement does not fall back)")
    torch.cuda.set_device(args.device)
    dev = Device(args.device)
    L = _lib.load()
    n = args.rows
    host_n = min(args.host_rows, n)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    if args.mode == "x25519":
        scalars, points = make_x25519(n)
        out = C.create_string_buffer(32)
        ks = [scalars[32 * q:32 * q + 32].tobytes() for q in range(host_n)]
        us = [points[32 * q:32 * q + 32].tobytes() for q in range(host_n)]
        host_out = []
        t0 = time.perf_counter()
        for q in range(host_n):
            L.wgcs_x25519(out, ks[q], us[q])
            host_out.append(out.raw)
        host_us = (time.perf_counter() - t0) / host_n * 1e6
        d_k, d_u = up(scalars), up(points)
        d_out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        d_status = torch.full((n,), -99, dtype=torch.int32, device="cuda")

        def launch():
            noise.x25519_batch(dev, d_k, d_u, d_out, d_status, stream=stream, n=n)
        launch()
        torch.cuda.synchronize()
        assert d_out[:32 * host_n].cpu().numpy().tobytes() == b"".join(host_out), "device X25519 != host X25519"
        assert bool((d_status == 0).all()), "status"
        kernel, workload = "x25519_kernel", {"rows": n}
    elif args.mode == "respond":
        table, init, psk, resp = make_respond(n, args.peers, args.distinct)
        msg, send, recv = C.create_string_buffer(92), C.create_string_buffer(32), C.create_string_buffer(32)
        calls = [(init[int(r["init_row"]):int(r["init_row"]) + 1].ctypes.data,
                  table["public_key"][int(r["peer_row"])].tobytes(), psk[int(r["peer_row"])].tobytes(),
                  r["ephemeral_private"].tobytes(), int(r["local_index"]),
                  r["cookie"].tobytes() if r["flags"] & 1 else None) for r in resp[:host_n]]
        host_rows = []
        t0 = time.perf_counter()
        for a in calls:
            rc = L.wgcs_noise_create_response(*a, msg, send, recv)
            host_rows.append((rc, msg.raw, send.raw, recv.raw))
        host_us = (time.perf_counter() - t0) / host_n * 1e6
        d_resp, d_init, d_table, d_psk = up(resp), up(init), up(table), up(psk)
        d_keys = torch.zeros(48 * 2 * n, dtype=torch.uint8, device="cuda")
        d_msgs = torch.zeros(noise.RESPONSE_PITCH * n, dtype=torch.uint8, device="cuda")
        d_status = torch.full((n,), -99, dtype=torch.int32, device="cuda")

        def launch():
            noise.respond_batch(dev, d_resp, d_init, None, d_table, d_psk, d_keys, d_msgs, d_status, stream=stream, n=n,
                                n_init=len(init), n_peers=len(table), n_keys=2 * n)
        launch()
        torch.cuda.synchronize()
        assert bool((d_status == noise.HS_RESPONDED).all()), "status"
        got_msgs = d_msgs[:noise.RESPONSE_PITCH * host_n].cpu().numpy().reshape(host_n, noise.RESPONSE_PITCH)
        got_keys = d_keys[:96 * host_n].cpu().numpy().reshape(host_n, 2, 48)
        for q, (rc, m, s_key, r_key) in enumerate(host_rows):
            sender = init["sender"][int(resp["init_row"][q])].tobytes()
            assert rc == 0 and got_msgs[q].tobytes() == m + bytes(4), f"device response {q} != host response"
            assert got_keys[q, 0].tobytes() == s_key + sender + bytes(12), f"device send key {q} != host"
            assert got_keys[q, 1].tobytes() == r_key + bytes(16), f"device recv key {q} != host"
        kernel = "hs_respond_kernel"
        workload = {"rows": n, "peers": len(table), "distinct_initiations": len(init), "cookie_fraction": 0.5,
                    "psk_fraction": 0.5, "gate": None}
        # the floor: three wgcs_x25519_batch launches of the same n, the ladders and nothing else
        x_k, x_u = (up(a) for a in make_x25519(n))
        x_out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        x_status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def floor():
            for _ in range(3):
                noise.x25519_batch(dev, x_k, x_u, x_out, x_status, stream=stream, n=n)
    else:
        responder, table, arena, pkts, msgs, is_valid = make_consume(n, args.peers, args.valid, args.distinct)
        rp, tp, row = responder.ctypes.data, table.ctypes.data, np.zeros(1, HS_INIT_DTYPE)
        host_rows, host_verdict = [], []
        t0 = time.perf_counter()
        for q in range(host_n):
            host_verdict.append(L.wgcs_noise_consume_initiation(rp, tp, len(table), msgs[q], MSG, row.ctypes.data))
            host_rows.append(row.tobytes())
        host_us = (time.perf_counter() - t0) / host_n * 1e6
        d_arena, d_pkts, d_responder, d_table = up(arena), up(pkts), up(responder), up(table)
        d_type = torch.ones(n, dtype=torch.int32, device="cuda")
        d_verdict = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        d_out = torch.zeros(128 * n, dtype=torch.uint8, device="cuda")

        def launch():
            noise.consume_batch(dev, d_arena, d_pkts, d_type, None, d_responder, d_table, d_verdict, d_out,
                                stream=stream, n=n, n_peers=len(table))
        launch()
        torch.cuda.synchronize()
        verdict = d_verdict.cpu().numpy()
        assert np.array_equal(verdict == noise.HS_CONSUMED, is_valid) and (verdict[~is_valid] == noise.ERR_AUTH).all(), "verdicts"
        assert verdict[:host_n].tolist() == host_verdict, "device verdicts != host verdicts"
        assert d_out[:128 * host_n].cpu().numpy().tobytes() == b"".join(host_rows), "device rows != host rows"
        kernel = "hs_consume_kernel"
        workload = {"rows": n, "message_bytes": MSG, "pitch": PITCH, "peers": len(table),
                    "valid_fraction": round(float(is_valid.mean()), 4), "distinct_messages": min(args.distinct, n),
                    "invalid": "one byte of the static field flipped: stops at the first open"}

    for _ in range(args.warmup):
        launch()
    e0.record(stream)
    for _ in range(args.steps):
        launch()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    rate = n / (ms * 1e-3)
    floor_ms = None
    if args.mode == "respond":  # the same event pair around K times three X25519 launches, in the same process
        for _ in range(args.warmup):
            floor()
        e0.record(stream)
        for _ in range(args.steps):
            floor()
        e1.record(stream)
        torch.cuda.synchronize()
        floor_ms = e0.elapsed_time(e1) / args.steps
    res = {
        "metric": {"x25519": "x25519_per_s", "consume": "handshake_consume_initiations_per_s",
                   "respond": "handshake_responses_per_s"}[args.mode],
        "value": round(rate), "unit": "rows/s", "us_per_launch": round(ms * 1e3, 2), "steps": args.steps,
        "warmup": args.warmup, "workload": workload, "kernel": kernel,
        "host_one_core": {"us_per_row": round(host_us, 2), "rows_per_s": round(1e6 / host_us), "rows": host_n,
                          "path": "the C ABI's host function, one ctypes call per row",
                          "device_over_host": round(rate / (1e6 / host_us), 1)},
    }
    if floor_ms is not None:
        res["three_x25519_launches"] = {"us": round(floor_ms * 1e3, 2), "kernel": "x25519_kernel",
                                        "respond_over_floor": round(ms / floor_ms, 3)}
    if not args.no_openssl:
        res["openssl_speed_ecdhx25519"] = openssl_speed()
    print(json.dumps(res), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
