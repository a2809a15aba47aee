"""Per-basic-block instruction census of aead_batch_kernel<SEAL|OPEN>, from the
compiler's own assembly (a count, for the VALU ceiling of DESIGN.md §4.9).

usage: python scripts/aead_valu_count.py [--json]

Compiles wireguard_amd/csrc/aead_kernels.hip for gfx950 with -S, splits each
kernel into basic blocks at its labels and prints, per block, the number of
VALU instructions (v_*), of those the 64-bit multiply-adds (v_mad_u64_u32,
which issue at a quarter of the plain rate), the DPP moves, the vector memory
instructions, and the branch targets.  A block whose branch goes to itself or
to an earlier label closes a loop.  The per-iteration cost of the main loop is
the sum over its blocks with the inner ChaCha loop (10 double rounds, unrolled
by 2: five trips) weighted by its trip count; wireguard_amd/aead_bench.py
does that sum from the blocks this script reports (loop_cost below).
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "wireguard_amd", "csrc", "aead_kernels.hip")
MAD64_ISSUE = 4  # v_mad_u64_u32 against a plain VALU instruction


def assembly() -> str:
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "aead.s")
        subprocess.run([hipcc, "--offload-arch=" + os.environ.get("WGCS_OFFLOAD_ARCH", "gfx950"), "-O3", "-std=c++17",
                        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", out, SRC],
                       check=True, capture_output=True)
        with open(out) as f:
            return f.read()


def kernels(asm: str) -> dict:
    """{SEAL|OPEN: [(label, [instructions])]} in program order."""
    res = {}
    for m in re.finditer(r"^(_ZN\S*aead_batch_kernelILi(\d)E\S*):.*?\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        blocks = [("entry", [])]
        for line in m.group(3).split("\n"):
            lm = re.match(r"^(\.LBB\d+_\d+):", line)
            if lm:
                blocks.append((lm.group(1), []))
                continue
            t = line.split(";")[0].strip()
            if t and not t.startswith("."):
                blocks[-1][1].append(t)
                if t.startswith(("s_cbranch", "s_branch")) :  # a branch ends the block; the fall-through is its own
                    nxt = blocks[-1][0].rstrip("+") + "+"
                    blocks.append((nxt if nxt != blocks[-1][0] else nxt + "+", []))
        res["OPEN" if m.group(2) == "1" else "SEAL"] = blocks
    return res


def census(blocks) -> list:
    order = {lbl: k for k, (lbl, _) in enumerate(blocks)}
    rows = []
    for k, (lbl, ins) in enumerate(blocks):
        valu = [i for i in ins if i.startswith("v_")]
        targets = [i.split()[-1] for i in ins if i.startswith("s_cbranch") or i.startswith("s_branch")]
        rows.append({"label": lbl, "n": len(ins), "valu": len(valu),
                     "mad64": sum(i.startswith("v_mad_u64_u32") for i in valu),
                     "dpp": sum("quad_perm" in i or "row_" in i for i in valu),
                     "rot": sum(i.startswith("v_alignbit") for i in valu),
                     "vmem": sum(i.startswith(("global_", "flat_", "buffer_")) for i in ins),
                     "targets": targets, "back": [t for t in targets if order.get(t, 1 << 30) <= k]})
    return rows


def loop_cost(rows) -> dict:
    """VALU issue slots of one trip of the main loop: the outermost loop that
    holds vector memory instructions; inner loops (the ChaCha rounds) count
    trips x body, with the trip count read off the unroll (10 double rounds)."""
    rows = [r for r in rows if r["n"]]
    order = {r["label"]: k for k, r in enumerate(rows)}
    loops = sorted({(order[t], k) for k, r in enumerate(rows) for t in r["back"]})
    # the main loop: the narrowest loop that holds loads, 64-bit multiplies and a
    # DPP round loop.  Every block of its body counts once, the byte-wise paths
    # of the ragged last chunk and the length block included, so the figure is
    # a little above what a trip over 16 whole chunks issues.
    def has(a, b, key):
        return sum(r[key] for r in rows[a:b + 1]) > 0
    cands = [(a, b) for a, b in loops if has(a, b, "vmem") and has(a, b, "mad64") and
             any(a <= x and y <= b and (x, y) != (a, b) and has(x, y, "dpp") and not has(x, y, "vmem") for x, y in loops)]
    if not cands:
        raise RuntimeError("main loop not found")
    a, b = min(cands, key=lambda ab: ab[1] - ab[0])
    inner = [(x, y) for x, y in loops if a <= x and y <= b and (x, y) != (a, b)]
    trips = {}
    for x, y in inner:  # a round loop: DPP, no memory; a double round has 8 rotations (v_alignbit)
        body = rows[x:y + 1]
        if sum(r["vmem"] for r in body) == 0 and sum(r["dpp"] for r in body):
            trips[(x, y)] = 10 // max(1, sum(r["rot"] for r in body) // 8)
    plain = mad = 0
    for k in range(a, b + 1):
        w = 1
        for (x, y), t in trips.items():
            if x <= k <= y:
                w = t
        plain += w * (rows[k]["valu"] - rows[k]["mad64"])
        mad += w * rows[k]["mad64"]
    return {"loop": [rows[a]["label"], rows[b]["label"]], "round_loops": {rows[x]["label"]: t for (x, y), t in trips.items()},
            "valu_plain": plain, "valu_mad64": mad, "issue_slots": plain + MAD64_ISSUE * mad}


def main():
    ks = kernels(assembly())
    out = {}
    for name, blocks in ks.items():
        rows = census(blocks)
        out[name] = {"blocks": rows, "main_loop": loop_cost(rows)}
    if "--json" in sys.argv:
        print(json.dumps(out))
        return
    for name, rec in out.items():
        print("==", name)
        for r in rec["blocks"]:
            print(f"{r['label']:10s} n={r['n']:4d} valu={r['valu']:4d} mad64={r['mad64']:3d} dpp={r['dpp']:3d} "
                  f"vmem={r['vmem']:2d} -> {','.join(r['targets'])}" + ("   (loop back)" if r["back"] else ""))
        print("main loop:", json.dumps(rec["main_loop"]))


if __name__ == "__main__":
    main()
