"""Per-keypair state measurement: the device-resident
wgcs_replay_batch / wgcs_send_assign_batch on one MI355X, and the host path
each replaces.

  python -m wireguard_amd.keystate_bench --mode replay|assign [--steps 200 --warmup 20]

Workload: 65,536 rows per launch (replay: messages; assign: Tun.Read jobs of 1
to 4 segments in 4 slots each) over 1, 16, 1,024 and 16,384 keys, dealt round
robin over the slots with a jitter of up to 3 places.  Replay counters ascend
per key; about 1 % of the rows are displaced by up to 64 places within their
key and 0.1 % repeat an earlier counter of their key.  The filters are zeroed
on the launches' stream before every launch, inside the timed region (its cost
alone is reported as zero_fill_us).  One enqueue of K launches sits between a HIP event
pair, after W warmup launches; every output of the first launch is compared
with the host loop first.

Per key count the JSON line carries: us per launch; keyorder_us, the same
launch with no row taking part (every pkt_len an error / every status
non-zero), which leaves the key pass, the sort and the heads and an empty
per-key kernel; and the host path measured in this process: D2H of what the
host step reads, one core running wgcs_replay_validate per row (a C loop built
here with the system compiler that calls the library's entry point; the send
step is the same loop shape over jobs), and H2D of what it produces.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import tempfile
import time

import numpy as np

from . import _lib, keystate
from .keystate import REPLAY_FILTER_DTYPE
from .transport import AEAD_PKT_DTYPE

MAX_SEGS, STRIDE = 4, 1440
LIMIT = _lib.REJECT_AFTER_MESSAGES

HOST_LOOP_C = r"""
#include <stdint.h>
typedef int (*validate_fn)(void *, uint64_t, uint64_t);
typedef struct { uint64_t off, counter; uint32_t len, key; } pkt;
void replay_loop(validate_fn f, char *filters, const pkt *pk, const int32_t *len, const uint64_t *ctr, uint32_t n,
                 uint32_t n_keys, uint64_t limit, int32_t *verdict) {
  for (uint32_t i = 0; i < n; ++i) {
    int32_t v = len[i];
    if (pk[i].key < n_keys && (v >= 0 || v == -8) && f(filters + 1032ull * pk[i].key, ctr[i], limit) != 1) v = -20;
    verdict[i] = v;
  }
}
/* the peer id is the key row in this bench */
void assign_loop(const int32_t *sizes, const uint32_t *peer, const int32_t *count, const int32_t *status, uint32_t nj,
                 uint32_t max_segs, uint64_t stride, uint64_t *nonce, uint8_t *dead, uint32_t n_keys, uint64_t limit,
                 pkt *pk, int32_t *nbufs, uint32_t *job_key) {
  for (uint32_t j = 0; j < nj; ++j) {
    uint32_t k = peer[(uint64_t)j * max_segs], c = (uint32_t)count[j];
    int keep = status[j] == 0 && count[j] >= 1 && c <= max_segs && k < n_keys && !dead[k];
    if (keep && (nonce[k] > limit || limit - nonce[k] < c)) { dead[k] = 1; nonce[k] = limit; keep = 0; }
    nbufs[j] = keep ? (int32_t)c : 0;
    job_key[j] = keep ? k : 0xFFFFFFFFu;
    for (uint32_t s = 0; s < max_segs; ++s) {
      uint64_t q = (uint64_t)j * max_segs + s;
      pk[q].off = q * stride;
      if (keep && s < c) { pk[q].counter = nonce[k]++; pk[q].len = (uint32_t)sizes[q]; pk[q].key = k; }
      else { pk[q].counter = 0; pk[q].len = 0; pk[q].key = 0xFFFFFFFFu; }
    }
  }
}
"""


def host_loop(td: str):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        raise SystemExit("keystate_bench: no C compiler for the host loop")
    src, so = os.path.join(td, "host_loop.c"), os.path.join(td, "host_loop.so")
    with open(src, "w") as f:
        f.write(HOST_LOOP_C)
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, src], check=True)
    return C.CDLL(so)


def deal_keys(n, n_keys, rng):
    return ((np.arange(n) + rng.integers(0, 4, n)) % n_keys).astype(np.uint32)


def replay_counters(keys, n_keys, rng):
    n = len(keys)
    counter = np.zeros(n, np.uint64)
    first = rng.integers(0, 1 << 40, n_keys).astype(np.uint64)
    displaced = repeated = 0
    order = np.argsort(keys, kind="stable")
    ends = np.searchsorted(keys[order], np.arange(n_keys + 1))
    for k in range(n_keys):
        rows = order[ends[k]:ends[k + 1]]  # the key's rows in slot order
        c = first[k] + np.arange(len(rows), dtype=np.uint64)
        for i in np.flatnonzero(rng.random(len(rows)) < 0.01):
            j = min(len(rows) - 1, i + int(rng.integers(1, 65)))
            c[i], c[j] = c[j], c[i]
            displaced += 1
        for i in np.flatnonzero(rng.random(len(rows)) < 0.001):
            if i:
                c[i] = c[int(rng.integers(0, i))]
                repeated += 1
        counter[rows] = c
    return counter, displaced, repeated


def timed(stream, e0, e1, warmup, steps, fn):
    import torch

    for _ in range(warmup):
        fn()
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("replay", "assign"), required=True)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 16, 1024, 16384])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0 or not 1 <= args.rows <= 1 << 24 or min(args.keys) < 1:
        ap.error("--steps >= 1, --warmup >= 0, 1 <= --rows <= 2^24, --keys >= 1")

    import torch  # before the library: one HIP runtime per process (_lib.load)

    from .tun import Device

    if not torch.cuda.is_available():
        raise SystemExit("keystate_bench: no GPU (this measurement does not fall back)")
    torch.cuda.set_device(args.device)
    dev = Device(args.device)
    n = args.rows
    # a stream of this bench's own for the launches and torch's fills alike: on the
    # default stream the library would use its context's stream, and each fill
    # would join the two
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    work = torch.empty(keystate.work_bytes(n), dtype=torch.uint8, device="cuda")
    results = []
    with tempfile.TemporaryDirectory() as td:
        hl = host_loop(td)
        validate = C.cast(dev.lib.wgcs_replay_validate, C.c_void_p)
        for n_keys in args.keys:
            rng = np.random.default_rng(20261020 + n_keys)
            keys = deal_keys(n, n_keys, rng)
            rec = {"keys": n_keys}
            if args.mode == "replay":
                counter, displaced, repeated = replay_counters(keys, n_keys, rng)
                pk = np.zeros(n, AEAD_PKT_DTYPE)
                pk["off"], pk["len"], pk["key"] = np.arange(n, dtype=np.uint64) * 1456, 1452, keys
                pkt_len = np.full(n, 1420, np.int32)
                d_pk, d_ctr = torch.from_numpy(pk.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counter.view(np.int64)).cuda()
                d_len, d_none = torch.from_numpy(pkt_len).cuda(), torch.full((n,), _lib.ERR_AUTH, dtype=torch.int32, device="cuda")
                d_f = torch.zeros(n_keys * REPLAY_FILTER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                d_v = torch.zeros(n, dtype=torch.int32, device="cuda")

                def launch(lens=d_len):
                    d_f.zero_()
                    keystate.replay_batch(dev, d_pk, lens, d_ctr, d_f, d_v, work, stream=stream, n=n, n_keys=n_keys)

                # the host path: D2H of what the filter reads, one core, H2D of the verdicts
                t0 = time.perf_counter()
                h_pk, h_len, h_ctr = d_pk.cpu().numpy(), d_len.cpu().numpy(), d_ctr.cpu().numpy()
                t1 = time.perf_counter()
                h_f, h_v = np.zeros(n_keys, REPLAY_FILTER_DTYPE), np.zeros(n, np.int32)
                h_f.view(np.uint8).fill(0)  # touch the pages: the host's filters are resident memory
                h_v.fill(0)
                t2 = time.perf_counter()
                hl.replay_loop(validate, C.c_void_p(h_f.ctypes.data), C.c_void_p(h_pk.ctypes.data),
                               C.c_void_p(h_len.ctypes.data), C.c_void_p(h_ctr.ctypes.data), C.c_uint32(n),
                               C.c_uint32(n_keys), C.c_uint64(LIMIT), C.c_void_p(h_v.ctypes.data))
                t3 = time.perf_counter()
                torch.from_numpy(h_v).cuda()
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                launch()
                torch.cuda.synchronize()
                assert np.array_equal(d_v.cpu().numpy(), h_v), "replay verdicts != wgcs_replay_validate"
                assert d_f.cpu().numpy().tobytes() == h_f.tobytes(), "filters != wgcs_replay_validate"
                rec.update(displaced=displaced, repeated=repeated, rejected=int((h_v == _lib.ERR_REPLAY).sum()))
                us = timed(stream, e0, e1, args.warmup, args.steps, launch)
                order_us = timed(stream, e0, e1, args.warmup, args.steps, lambda: launch(d_none))
                zero_us = timed(stream, e0, e1, args.warmup, args.steps, lambda: d_f.zero_())
                launch()
                torch.cuda.synchronize()
                assert np.array_equal(d_v.cpu().numpy(), h_v), "replay verdicts after the timed launches"
            else:
                count = rng.integers(1, MAX_SEGS + 1, n).astype(np.int32)
                status = np.where(rng.random(n) < 0.01, -3, 0).astype(np.int32)
                peer = np.repeat(keys, MAX_SEGS)  # the peer id is the key row
                sizes = rng.integers(1, 1421, n * MAX_SEGS).astype(np.int32)
                first = rng.integers(0, 1 << 40, n_keys).astype(np.uint64)
                from . import router

                slots = router.session_table(np.arange(n_keys, dtype=np.uint32), np.arange(n_keys, dtype=np.uint32))
                d_sizes, d_peer, d_count, d_status = (torch.from_numpy(x.view(np.int32)).cuda()
                                                      for x in (sizes, peer, count, status))
                d_bad = torch.full((n,), -3, dtype=torch.int32, device="cuda")
                d_slots = torch.from_numpy(slots.view(np.uint8).reshape(-1)).cuda()
                d_nonce = torch.from_numpy(first.view(np.int64).copy()).cuda()
                d_pk = torch.zeros(n * MAX_SEGS * AEAD_PKT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                d_nbufs, d_key = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))

                def launch(st=d_status):
                    keystate.send_assign_batch(dev, d_sizes, d_peer, d_count, st, MAX_SEGS, STRIDE, d_slots, d_nonce, d_pk,
                                               d_nbufs, d_key, work, stream=stream, n_jobs=n, n_slots=len(slots),
                                               n_keys=n_keys)

                t0 = time.perf_counter()
                h_sizes, h_peer, h_count, h_status = (x.cpu().numpy() for x in (d_sizes, d_peer, d_count, d_status))
                t1 = time.perf_counter()
                h_pk, h_nbufs, h_key = np.zeros(n * MAX_SEGS, AEAD_PKT_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.uint32)
                h_nonce, dead = first.copy(), np.zeros(n_keys, np.uint8)
                for a in (h_pk.view(np.uint8), h_nbufs, h_key, dead):
                    a.fill(0)  # touch the pages
                t2 = time.perf_counter()
                hl.assign_loop(*(C.c_void_p(x.ctypes.data) for x in (h_sizes, h_peer, h_count, h_status)), C.c_uint32(n),
                               C.c_uint32(MAX_SEGS), C.c_uint64(STRIDE), C.c_void_p(h_nonce.ctypes.data),
                               C.c_void_p(dead.ctypes.data), C.c_uint32(n_keys), C.c_uint64(LIMIT),
                               C.c_void_p(h_pk.ctypes.data), C.c_void_p(h_nbufs.ctypes.data), C.c_void_p(h_key.ctypes.data))
                t3 = time.perf_counter()
                torch.from_numpy(h_pk.view(np.uint8).reshape(-1)).cuda()
                torch.from_numpy(h_nbufs).cuda()
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                launch()
                torch.cuda.synchronize()
                assert d_pk.cpu().numpy().tobytes() == h_pk.tobytes(), "seal descriptors != the host loop"
                assert np.array_equal(d_nbufs.cpu().numpy(), h_nbufs), "d_nbufs != the host loop"
                assert np.array_equal(d_key.cpu().numpy().view(np.uint32), h_key), "d_job_key != the host loop"
                assert np.array_equal(d_nonce.cpu().numpy().view(np.uint64), h_nonce), "d_send_nonce != the host loop"
                rec.update(max_segs=MAX_SEGS, kept_jobs=int((h_nbufs > 0).sum()))
                us = timed(stream, e0, e1, args.warmup, args.steps, launch)
                order_us = timed(stream, e0, e1, args.warmup, args.steps, lambda: launch(d_bad))
                zero_us = None
            rec.update(us_per_launch=round(us, 2), mrows_per_s=round(n / us, 1), keyorder_us=round(order_us, 2),
                       host_d2h_us=round((t1 - t0) * 1e6, 1), host_one_core_us=round((t3 - t2) * 1e6, 1),
                       host_h2d_us=round((t4 - t3) * 1e6, 1),
                       host_path_us=round((t1 - t0 + t3 - t2 + t4 - t3) * 1e6, 1))
            if zero_us is not None:
                rec.update(zero_fill_us=round(zero_us, 2))
            results.append(rec)
    print(json.dumps({"metric": f"keystate_{args.mode}_us", "unit": "us/launch", "steps": args.steps,
                      "warmup": args.warmup, "workload": {"rows": n}, "keys": results}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
