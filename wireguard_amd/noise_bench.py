"""X25519 and handshake measurement: the
device-resident wgcs_x25519_batch, wgcs_handshake_consume_batch,
wgcs_handshake_respond_batch, wgcs_handshake_initiate_batch,
wgcs_handshake_finish_batch and wgcs_handshake_accept_batch on one MI355X, beside the same scalar code on one
host core.

  python -m wireguard_amd.noise_bench --mode x25519|consume|respond|initiate|finish|accept
                                      [--rows 65536 --peers 1024 --steps 20 --warmup 3]

Workload:
  accept    the consume workload below, and behind it
           wgcs_handshake_accept_batch over consume's rows against a fresh table
           of peer rows, with `--tickets` tickets; one JSON line for `rows` and
           one for 1,024 rows.  The authentic messages come from 16 peers and
           are tiled, so a batch is a flood of replayed authentic initiations:
           16 winners, the rest replays and floods.  Timed: the accept call
           alone (HIP events; a device copy restores the peer rows before every
           call), the chain consume -> accept -> respond on one stream, and the
           way without the call: consume, synchronise, read d_out and the
           verdicts back, wgcs_handshake_accept_host on one core, upload the
           descriptors, respond.  The two chains are timed by a host clock
           around one call that ends in a synchronise, alternating; their
           outputs are compared before anything is timed.
  initiate `rows` descriptors, every one of which runs the whole function: state
           row q and key rows 2q and 2q + 1, the peers in turn, a fresh ephemeral
           key, timestamp and index each, a cookie on every other one.
  finish   `rows` responses of 92 B at odd byte offsets of one arena (pitch 97),
           every row of type 2 with no gate and authentic, each for a state row of
           its own.  `--distinct` handshakes are made on the host (initiation,
           the peer's consume and response) and tiled: a tiled row is its state
           and its response under another index, which the transcript does not
           cover, so every lane does the whole work and every row ends
           WGCS_HS_FINISHED.  The call zeroes the states it finishes, so a device
           copy restores the state table before every launch, inside the timed
           window (128 B per row, read and written once).
           Both lines also carry two wgcs_x25519_batch launches of the same
           `rows` timed in the same process, the floor for two ladders per lane.
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
wgcs_noise_create_response, one call per row; wgcs_handshake_initiate_host /
wgcs_handshake_finish_host, one call for all rows) on one CPU core over the first `--host-rows` rows, called through ctypes, and
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
from .transport import AEAD_KEY_DTYPE, AEAD_PKT_DTYPE

MSG, PITCH = 148, 150
RESP_PITCH = 97  # finish: responses at 1 + 97 q, every alignment of the dword loads
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


def _peers(rng, n_peers: int):
    """(private keys of the first INITIATORS peers, every peer's public key)"""
    privs = [rng.bytes(32) for _ in range(min(INITIATORS, n_peers))]
    keys = [noise.x25519(k, (9).to_bytes(32, "little")) for k in privs]
    keys += [noise.x25519(rng.bytes(32), (9).to_bytes(32, "little")) for _ in range(n_peers - len(keys))]
    return privs, keys


def make_initiate(n: int, n_peers: int, seed: int = 20261023, callers: int | None = None):
    """The initiator's responder row, public key and peer table, and n descriptors:
    state row q, key rows 2q and 2q + 1, the peers in turn (or only the first
    `callers` of them, whose private keys are returned), index 1 + q, a cookie on
    every other one."""
    rng = np.random.default_rng(seed)
    me, pub = noise.responder_init(rng.bytes(32))
    privs, keys = _peers(rng, n_peers)
    table = noise.peer_keys_build(me, keys, np.arange(n_peers, dtype=np.uint32))
    row_of_peer = np.zeros(n_peers, np.uint32)
    row_of_peer[table["peer"]] = np.arange(n_peers, dtype=np.uint32)
    q = np.arange(n, dtype=np.uint32)
    start = np.zeros(n, noise.HS_START_DTYPE)
    start["state_row"], start["send_key"], start["recv_key"] = q, 2 * q, 2 * q + 1
    start["peer_row"] = row_of_peer[q % (n_peers if callers is None else callers)]
    start["local_index"], start["flags"] = 1 + q, q & 1
    start["timestamp"] = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    start["ephemeral_private"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    start["cookie"] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    return me, pub, privs, table, start


def make_finish(n: int, n_peers: int, distinct: int, seed: int = 20261024):
    """`distinct` whole handshakes made on the host against the first INITIATORS
    peers, tiled over n rows: state row q and the response at 1 + 97 q carry the
    index 1 + q.  A preshared key for every other peer."""
    from .router import session_table

    rng = np.random.default_rng(seed)
    m = min(distinct, n)
    me, pub, privs, table, start = make_initiate(m, n_peers, seed, callers=min(INITIATORS, n_peers))
    psk = rng.integers(0, 256, (n_peers, 32), dtype=np.uint8)
    psk[::2] = 0
    states, msgs, status = np.zeros(m, noise.HS_STATE_DTYPE), np.zeros(m * noise.INITIATION_PITCH, np.uint8), np.zeros(m, np.int32)
    noise.initiate_host(start, pub, table, states, msgs, status, 2 * m)
    assert (status == noise.HS_INITIATED).all()
    sides = []
    for k in privs:
        r, _ = noise.responder_init(k)
        sides.append((r, noise.peer_keys_build(r, [pub], [0])))
    responses = np.zeros((m, 92), np.uint8)
    for h in range(m):
        r, t = sides[h % len(privs)]
        verdict, init = noise.consume_initiation(r, t, msgs[noise.INITIATION_PITCH * h:noise.INITIATION_PITCH * h + 148].tobytes())
        assert verdict == noise.HS_CONSUMED
        key = psk[int(start["peer_row"][h])]
        rc, msg, _, _ = noise.create_response(init, pub, rng.bytes(32), int(rng.integers(0, 2**32)),
                                              key.tobytes() if key.any() else None, rng.bytes(16) if h & 1 else None)
        assert rc == 0
        responses[h] = np.frombuffer(msg, np.uint8)
    q = np.arange(n, dtype=np.uint32)
    all_states = states[q % m].copy()
    all_states["local_index"], all_states["send_key"], all_states["recv_key"] = 1 + q, 2 * q, 2 * q + 1
    tiled = responses[q % m].copy()
    tiled[:, 8:12] = (1 + q).astype("<u4").view(np.uint8).reshape(n, 4)
    arena = np.zeros(1 + RESP_PITCH * n + 64, np.uint8)
    at = 1 + RESP_PITCH * q.astype(np.int64)
    arena[(at[:, None] + np.arange(92)[None, :]).reshape(-1)] = tiled.reshape(-1)
    pkts = np.zeros(n, AEAD_PKT_DTYPE)
    pkts["off"], pkts["len"], pkts["key"] = at, 92, 0xFFFFFFFF
    slots = session_table(1 + q, q)
    return me, table, psk, all_states, arena, pkts, slots


def run_accept(args, dev, torch) -> None:
    """--mode accept: one JSON line per batch size (see the module docstring)."""
    L = _lib.load()
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    def pinned(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    now, nt = 1_700_000_000_000_000_000, args.tickets
    for n in dict.fromkeys((args.rows, min(args.rows, 1024))):
        responder, table, arena, pkts, msgs, is_valid = make_consume(n, args.peers, args.valid, args.distinct)
        n_peers = len(table)
        peer_rows = noise.peer_rows_build(table, n_peers)
        peers0 = np.zeros(n_peers, noise.HS_PEER_DTYPE)
        peers0["claim"] = noise.HS_CLAIM_NONE
        rng = np.random.default_rng(20261025)
        tickets = np.zeros(nt, noise.HS_TICKET_DTYPE)
        tickets["local_index"] = rng.integers(0, 2**32, nt, dtype=np.uint32)
        tickets["send_key"], tickets["recv_key"] = 2 * np.arange(nt, dtype=np.uint32), 2 * np.arange(nt, dtype=np.uint32) + 1
        tickets["ephemeral_private"] = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        d_arena, d_pkts, d_responder, d_table = up(arena), up(pkts), up(responder), up(table)
        d_rows, d_peers0, d_tickets = up(peer_rows), up(peers0), up(tickets)
        d_peers = d_peers0.clone()
        d_type = torch.ones(n, dtype=torch.int32, device="cuda")
        d_consumed = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        d_verdict = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        d_init = torch.zeros(128 * n, dtype=torch.uint8, device="cuda")
        d_resp = torch.zeros(80 * nt, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_keys = torch.zeros(48 * 2 * nt, dtype=torch.uint8, device="cuda")
        d_msgs = torch.zeros(noise.RESPONSE_PITCH * nt, dtype=torch.uint8, device="cuda")
        d_status = torch.full((nt,), -99, dtype=torch.int32, device="cuda")

        def consume():
            noise.consume_batch(dev, d_arena, d_pkts, d_type, None, d_responder, d_table, d_consumed, d_init,
                                stream=stream, n=n, n_peers=n_peers)

        def accept():
            d_peers.copy_(d_peers0)  # the call commits what it accepts: every launch starts from the same table
            noise.accept_batch(dev, d_init, d_consumed, now, d_table, d_rows, d_peers, d_tickets, d_resp, d_count,
                               d_verdict, stream=stream, n=n, n_ids=n_peers, n_peers=n_peers, n_tickets=nt)

        def respond(m=nt):
            noise.respond_batch(dev, d_resp, d_init, None, d_table, None, d_keys, d_msgs, d_status, stream=stream, n=m,
                                n_init=n, n_peers=n_peers, n_keys=2 * nt)

        def device_chain():
            consume(), accept(), respond()

        # the parent's way: consume, synchronise, read the rows back, the tail on one host core, upload, respond
        h_init, h_consumed, h_resp = pinned(128 * n), pinned(4 * n), pinned(80 * nt)
        np_init, np_consumed = h_init.numpy().view(HS_INIT_DTYPE), h_consumed.numpy().view(np.int32)
        np_resp = h_resp.numpy().view(noise.HS_RESP_DTYPE)
        h_peers, h_count, h_verdict = peers0.copy(), np.zeros(1, np.uint32), np.zeros(n, np.int32)
        tail_s = []

        def host_tail():
            h_peers[:] = peers0
            t0 = time.perf_counter()
            rc = L.wgcs_handshake_accept_host(np_init.ctypes.data, np_consumed.ctypes.data, n, now, table.ctypes.data,
                                              peer_rows.ctypes.data, n_peers, h_peers.ctypes.data, n_peers,
                                              tickets.ctypes.data, nt, np_resp.ctypes.data, h_count.ctypes.data,
                                              h_verdict.ctypes.data)
            tail_s.append(time.perf_counter() - t0)
            assert rc == 0

        def host_chain():
            consume()
            h_init.copy_(d_init, non_blocking=True)
            h_consumed.copy_(d_consumed.view(torch.uint8), non_blocking=True)
            stream.synchronize()
            host_tail()
            m = int(h_count[0])
            if m:
                d_resp[:80 * m].copy_(h_resp[:80 * m], non_blocking=True)
                respond(m)

        # both ways give the same bytes, and they are the host form's
        device_chain()
        torch.cuda.synchronize()
        got = (d_verdict.cpu().numpy(), d_peers.cpu().numpy(), d_resp.cpu().numpy(), int(d_count.item()),
               d_msgs.cpu().numpy(), d_keys.cpu().numpy(), d_status.cpu().numpy())
        d_msgs.zero_(), d_keys.zero_(), d_status.fill_(-99)
        host_chain()
        torch.cuda.synchronize()
        m = int(h_count[0])
        assert np.array_equal(got[0], h_verdict), "device verdicts != host form"
        assert got[1].tobytes() == h_peers.tobytes() and got[3] == m, "device peer rows / count != host form"
        assert got[2].tobytes() == np_resp.tobytes(), "device descriptors != host form"
        assert got[4][:noise.RESPONSE_PITCH * m].tobytes() == d_msgs.cpu().numpy()[:noise.RESPONSE_PITCH * m].tobytes(), "responses"
        assert got[5].tobytes() == d_keys.cpu().numpy().tobytes(), "keys"
        assert (got[6][:m] == noise.HS_RESPONDED).all() and (got[6][m:] == _lib.ERR_INVALID_ARG).all(), "status"
        assert m == int((h_verdict == noise.HS_ACCEPTED).sum()) and m > 0

        def events(fn):
            for _ in range(args.warmup):
                fn()
            e0.record(stream)
            for _ in range(args.steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.steps * 1e3

        def wall(fn):
            """us per call, each call ending in a synchronise: (median, min)"""
            out = []
            for k in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    out.append((time.perf_counter() - t0) * 1e6)
            return round(float(np.median(out)), 2), round(min(out), 2)

        accept_us = events(accept)
        restore_us = events(lambda: d_peers.copy_(d_peers0))
        chain_events_us = events(device_chain)
        consume_us = events(consume)
        rounds = [(wall(device_chain), wall(host_chain)) for _ in range(3)]  # alternating, in one process
        del tail_s[:]
        for _ in range(5):
            host_tail()
        tail_us = float(np.median(tail_s)) * 1e6
        verdicts = {str(k): int(v) for k, v in zip(*np.unique(h_verdict, return_counts=True))}
        res = {
            "metric": "handshake_accept_rows_per_s", "value": round(n / (accept_us * 1e-6)), "unit": "rows/s",
            "us_per_launch": round(accept_us, 2), "steps": args.steps, "warmup": args.warmup,
            "kernel": "hs_accept_claim_kernel + hs_accept_verdict_kernel + compact_scan_kernel + hs_accept_commit_kernel",
            "timing": "HIP events around K calls; each call is a device copy that restores the peer rows, then the four launches",
            "peer_row_restore_us": round(restore_us, 2),
            "workload": {"rows": n, "peers": n_peers, "calling_peers": min(INITIATORS, n_peers), "tickets": nt,
                         "valid_fraction": round(float(is_valid.mean()), 4), "distinct_messages": min(args.distinct, n),
                         "verdicts": verdicts, "now": "one value; every peer row starts fresh"},
            "chain_consume_accept_respond": {
                "device_events_us": round(chain_events_us, 2), "consume_alone_events_us": round(consume_us, 2),
                "respond": f"{nt} descriptors, NULL gate, count not read",
                "device_wall_us_median_min": [r[0] for r in rounds],
                "parent_way_wall_us_median_min": [r[1] for r in rounds],
                "parent_way": "consume, stream synchronise, d_out and verdicts to pinned memory, wgcs_handshake_accept_host on "
                              "one core, upload of the descriptors written, respond over them",
                "wall": "host clock around one call ending in a device synchronise; three rounds, the two ways alternating"},
            "host_one_core": {"us_per_batch": round(tail_us, 2), "ns_per_row": round(tail_us * 1e3 / n, 2), "rows": n,
                              "path": "wgcs_handshake_accept_host, one ctypes call for all rows"},
        }
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("x25519", "consume", "respond", "initiate", "finish", "accept"), required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--peers", type=int, default=1024, help="rows of the peer table (consume)")
    ap.add_argument("--valid", type=float, default=0.5, help="fraction of authentic initiations (consume)")
    ap.add_argument("--distinct", type=int, default=1024, help="authentic messages made on the host and tiled")
    ap.add_argument("--host-rows", type=int, default=512, help="rows the one-core host path is timed over")
    ap.add_argument("--tickets", type=int, default=64, help="responses the caller is ready to pay for (accept)")
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
    if args.mode == "accept":
        run_accept(args, dev, torch)
        dev.close()
        return
    L = _lib.load()
    n = args.rows
    host_n = min(args.host_rows, n)
    host_path = "the C ABI's host function, one ctypes call per row"

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

        floor_launches = 3
    elif args.mode == "initiate":
        me, pub, _, table, start = make_initiate(n, args.peers)
        h_states = np.zeros(host_n, noise.HS_STATE_DTYPE)
        h_msgs, h_status = np.zeros(noise.INITIATION_PITCH * host_n, np.uint8), np.zeros(host_n, np.int32)
        t0 = time.perf_counter()
        rc = L.wgcs_handshake_initiate_host(start.ctypes.data, host_n, pub, table.ctypes.data, len(table), 2 * n,
                                            h_states.ctypes.data, host_n, h_msgs.ctypes.data, h_status.ctypes.data)
        host_us = (time.perf_counter() - t0) / host_n * 1e6
        assert rc == 0 and (h_status == noise.HS_INITIATED).all(), "host status"
        d_start, d_pub, d_table = up(start), up(np.frombuffer(pub, np.uint8)), up(table)
        d_states = torch.zeros(128 * n, dtype=torch.uint8, device="cuda")
        d_msgs = torch.zeros(noise.INITIATION_PITCH * n, dtype=torch.uint8, device="cuda")
        d_status = torch.full((n,), -99, dtype=torch.int32, device="cuda")

        def launch():
            noise.initiate_batch(dev, d_start, d_pub, d_table, d_states, d_msgs, d_status, 2 * n, stream=stream, n=n,
                                 n_peers=len(table), n_states=n)
        launch()
        torch.cuda.synchronize()
        assert bool((d_status == noise.HS_INITIATED).all()), "status"
        assert d_msgs[:noise.INITIATION_PITCH * host_n].cpu().numpy().tobytes() == h_msgs.tobytes(), "device initiations != host"
        assert d_states[:128 * host_n].cpu().numpy().tobytes() == h_states.tobytes(), "device states != host states"
        kernel = "hs_initiate_kernel"
        workload = {"rows": n, "peers": len(table), "cookie_fraction": 0.5}
        floor_launches, host_path = 2, "wgcs_handshake_initiate_host, one ctypes call for all rows"
    elif args.mode == "finish":
        me, table, psk, states, arena, pkts, slots = make_finish(n, args.peers, args.distinct)
        h_states, h_keys = states[:host_n].copy(), np.zeros(2 * host_n, AEAD_KEY_DTYPE)
        h_work, h_verdict = np.zeros(noise.FINISH_WORK_BYTES * host_n, np.uint8), np.zeros(host_n, np.int32)
        h_type = np.full(n, 2, np.int32)
        t0 = time.perf_counter()
        rc = L.wgcs_handshake_finish_host(arena.ctypes.data, pkts.ctypes.data, h_type.ctypes.data, None, host_n,
                                          me.ctypes.data, slots.ctypes.data, len(slots), h_states.ctypes.data, host_n,
                                          psk.ctypes.data, len(psk), h_keys.ctypes.data, 2 * host_n, h_work.ctypes.data,
                                          h_verdict.ctypes.data)
        host_us = (time.perf_counter() - t0) / host_n * 1e6
        assert rc == 0 and (h_verdict == noise.HS_FINISHED).all(), "host verdicts"
        d_arena, d_pkts, d_me, d_slots, d_psk = up(arena), up(pkts), up(me), up(slots), up(psk)
        d_states0 = up(states)
        d_states = d_states0.clone()
        d_type = torch.full((n,), 2, dtype=torch.int32, device="cuda")
        d_keys = torch.zeros(48 * 2 * n, dtype=torch.uint8, device="cuda")
        d_work = torch.zeros(noise.FINISH_WORK_BYTES * n, dtype=torch.uint8, device="cuda")
        d_verdict = torch.full((n,), -99, dtype=torch.int32, device="cuda")

        def launch():
            d_states.copy_(d_states0)  # the call zeroes what it finishes: every launch starts from the same table
            noise.finish_batch(dev, d_arena, d_pkts, d_type, None, d_me, d_slots, d_states, d_psk, d_keys, d_work,
                               d_verdict, stream=stream, n=n, n_slots=len(slots), n_states=n, n_peers=len(psk),
                               n_keys=2 * n)
        launch()
        torch.cuda.synchronize()
        assert bool((d_verdict == noise.HS_FINISHED).all()), "verdicts"
        assert d_keys[:96 * host_n].cpu().numpy().tobytes() == h_keys.tobytes(), "device keys != host keys"
        assert d_states[:128 * host_n].cpu().numpy().tobytes() == h_states.tobytes(), "device states != host states"
        assert not bool(d_work.any()), "d_work"
        kernel = "hs_finish_kernel + hs_finish_commit_kernel"
        workload = {"rows": n, "message_bytes": 92, "pitch": RESP_PITCH, "peers": len(table),
                    "distinct_handshakes": min(args.distinct, n), "psk_fraction": 0.5, "gate": None,
                    "state_restore": "a device copy of the state table before every launch, inside the timed window"}
        floor_launches, host_path = 2, "wgcs_handshake_finish_host, one ctypes call for all rows"
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
    if args.mode in ("respond", "initiate", "finish"):  # the same event pair around K times the bare X25519 launches
        if args.mode != "respond":
            x_k, x_u = (up(a) for a in make_x25519(n))
            x_out = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
            x_status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def floor():
            for _ in range(floor_launches):
                noise.x25519_batch(dev, x_k, x_u, x_out, x_status, stream=stream, n=n)
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
                   "respond": "handshake_responses_per_s", "initiate": "handshake_initiations_per_s",
                   "finish": "handshake_finishes_per_s"}[args.mode],
        "value": round(rate), "unit": "rows/s", "us_per_launch": round(ms * 1e3, 2), "steps": args.steps,
        "warmup": args.warmup, "workload": workload, "kernel": kernel,
        "host_one_core": {"us_per_row": round(host_us, 2), "rows_per_s": round(1e6 / host_us), "rows": host_n,
                          "path": host_path,
                          "device_over_host": round(rate / (1e6 / host_us), 1)},
    }
    if floor_ms is not None:
        res[{3: "three", 2: "two"}[floor_launches] + "_x25519_launches"] = {
            "us": round(floor_ms * 1e3, 2), "kernel": "x25519_kernel", f"{args.mode}_over_floor": round(ms / floor_ms, 3)}
    if not args.no_openssl:
        res["openssl_speed_ecdhx25519"] = openssl_speed()
    print(json.dumps(res), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
