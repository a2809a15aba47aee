#!/usr/bin/env python3
"""Interleaved bench.py runs of several builds / settings on one box (NOT
product code): each leg is a label, environment overrides and bench arguments;
the legs run round after round, each run a fresh child process under its own
time limit, and one record per run (value, roofline.kernel_ms,
timing.wall_minus_span_us) is appended to OUT.jsonl.  Stops at the first run
that fails or runs out of time.

usage: python scripts/ab_bench.py OUT.jsonl ROUNDS LABEL=KEY~VALUE,KEY~VALUE:BENCH_ARGS ...
e.g.   python scripts/ab_bench.py ab.jsonl 5 "parent=WGCS_LIB~/path/to/parent/libwgcsum.so:--gpus 1 --steps 20 --warmup 5" \\
           "new=:--gpus 1 --steps 20 --warmup 5" "fuse0=WGCS_FUSE~0:--gpus 1 --steps 20 --warmup 5"
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out, rounds = sys.argv[1], int(sys.argv[2])
    legs = []
    for spec in sys.argv[3:]:
        label, rest = spec.split("=", 1)
        envs, _, args = rest.partition(":")
        env = dict(kv.split("~", 1) for kv in filter(None, envs.split(",")))
        legs.append((label, env, args.split()))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        for r in range(rounds):
            for label, env, args in legs:
                cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
                t0 = time.time()
                try:
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, **env))
                except subprocess.TimeoutExpired:
                    print(f"TIMEOUT {label}: stopping", flush=True)
                    sys.exit(124)
                if p.returncode != 0 or "illegal memory access" in p.stderr:
                    print(f"FAIL {label} rc={p.returncode}\n{p.stderr[-3000:]}", flush=True)
                    sys.exit(1)
                line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                rec = {"label": label, "round": r, "args": " ".join(args),
                       "env": {k: os.path.basename(v) for k, v in env.items()},
                       "value": line["value"], "ms_per_step": line["ms_per_step"],
                       "kernel_ms": line.get("roofline", {}).get("kernel_ms"),
                       "frac": line.get("roofline", {}).get("frac"),
                       "wall_minus_span_us": line.get("timing", {}).get("wall_minus_span_us"),
                       "wall_us": line.get("timing", {}).get("wall_us")}
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(f"{label:10s} r{r} value={rec['value']} kernel_ms={rec['kernel_ms']} "
                      f"wms={rec['wall_minus_span_us']} ({time.time() - t0:.1f}s)", flush=True)


if __name__ == "__main__":
    main()
