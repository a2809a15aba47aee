"""The Poly1305 limb arithmetic of the AEAD kernel (wireguard_amd/csrc/
wgcs_poly1305.h) as host code under AddressSanitizer + UBSan, against Python
ints (CPU only).

tests/aead_host/poly1305_host.cpp is a stand-alone program that includes the
header the kernel includes.  The edges below cannot be reached through the AEAD
interface, where r comes out of ChaCha20: the clamp's extremes, accumulators
that sit at p - 1, p, p + 1 and 2^130 - 1 before the final reduction, and the
row-parallel schedule at every block count that changes which lane holds the
last block."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import aead_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "aead_host", "poly1305_host.cpp")
P = aead_ref.P1305
MASK26 = (1 << 26) - 1

RFC_KEY = bytes.fromhex("85d6be7857556d337f4452fe42d506a8" "0103808afb0db2fd4abff6af4149f51b")  # §2.5.2
RFC_MSG = b"Cryptographic Forum Research Group"
RFC_TAG = "a8061dc1305136c6c22b8baf0c0127a9"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("poly1305") / "poly1305_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "wireguard_amd", "csrc"),
                    "-o", str(exe), SRC], check=True, timeout=300)
    return str(exe)


def run(prog, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    out = p.stdout.split()
    assert out[-2:] == ["poly1305_host:", "ok"]
    tags = out[:-2]
    assert len(tags) == len(lines)
    return tags


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def test_rfc_8439_vector(prog):
    assert aead_ref.poly1305(RFC_KEY, RFC_MSG).hex() == RFC_TAG
    assert run(prog, [f"mac {RFC_KEY.hex()} {RFC_MSG.hex()}", f"row {RFC_KEY.hex()} {RFC_MSG.hex()}"]) == [RFC_TAG] * 2


def test_clamp_extremes_and_ff_blocks(prog):
    """r and s all ones (the clamp leaves r = 0x0ffffffc0ffffffc0ffffffc0fffffff,
    its largest value) and all zero, with messages of all-0xFF blocks."""
    lines, want = [], []
    for r in (b"\xff" * 16, b"\0" * 16, b"\x01" + b"\0" * 15, b"\xfc\xff\xff\x0f" * 4):
        for s in (b"\xff" * 16, b"\0" * 16):
            for n in (0, 1, 15, 16, 17, 32, 33, 256, 257, 1024):
                key, msg = r + s, b"\xff" * n
                for op in ("mac", "row"):
                    lines.append(f"{op} {key.hex()} {hx(msg)}")
                    want.append(aead_ref.poly1305(key, msg).hex())
    assert run(prog, lines) == want


def limbs(v: int, spread: int = 0):
    """v as five 26-bit limbs; spread > 0 moves value into higher-than-26-bit
    limbs the way a sum of `spread` carried numbers looks (same value)."""
    l = [(v >> (26 * i)) & MASK26 for i in range(4)] + [v >> 104]
    for i in range(4):  # borrow from limb i + 1 into limb i: value unchanged
        k = min(spread, l[i + 1])
        l[i + 1] -= k
        l[i] += k << 26
    return l


def test_final_reduction_edges(prog):
    """p1305_finish on accumulators at and around p, canonical and as un-carried
    sums (limbs up to 2^31), with s = 0 and s = all ones (the carry out of 2^128
    is dropped)."""
    values = [0, 1, 4, 5, 6, P - 6, P - 5, P - 1, P, P + 1, P + 4, P + 5, (1 << 130) - 1, 1 << 130, (1 << 130) + 5,
              2 * P - 1, 2 * P, (1 << 128) - 1, 1 << 128, (1 << 104) - 1]
    lines, want = [], []
    for v in values:
        for spread in (0, 1, 15, 30):
            l = limbs(v, spread)
            assert sum(x << (26 * i) for i, x in enumerate(l)) == v and all(x < (1 << 31) for x in l)
            for s in (0, (1 << 128) - 1, 0x0123456789ABCDEF0FEDCBA987654321):
                lines.append("fin " + " ".join(f"{x:x}" for x in l) + " " + s.to_bytes(16, "little").hex())
                want.append((((v % P) + s) & ((1 << 128) - 1)).to_bytes(16, "little").hex())
    assert run(prog, lines) == want


def test_accumulator_at_p_through_real_inputs(prog):
    """r = 1 makes the accumulator the plain sum of the blocks (each block is
    its 16 bytes + 2^128), so these messages leave exactly p - 1, p, p + 1 and
    2^130 - 1 in the limbs before the final reduction."""
    key = b"\x01" + b"\0" * 15 + bytes(range(16))

    def blk(v):
        return v.to_bytes(16, "little")
    cases = {
        P - 1: blk((1 << 128) - 1) + blk((1 << 128) - 5),
        P: blk((1 << 128) - 1) + blk((1 << 128) - 4),
        P + 1: blk((1 << 128) - 1) + blk((1 << 128) - 3),
        (1 << 130) - 1: blk((1 << 128) - 1) + blk(0) + blk(0),
    }
    lines, want = [], []
    for total, msg in cases.items():
        assert sum(int.from_bytes(msg[i:i + 16], "little") + (1 << 128) for i in range(0, len(msg), 16)) == total
        for op in ("mac", "row"):
            lines.append(f"{op} {key.hex()} {msg.hex()}")
            want.append(aead_ref.poly1305(key, msg).hex())
    assert run(prog, lines) == want


def test_row_parallel_matches_serial_for_every_block_count(prog):
    """16 interleaved accumulators with powers of r against serial Horner and
    Python ints: 0..40 whole blocks, and each with a ragged last block."""
    rng = np.random.default_rng(8439)
    lines, want = [], []
    for nblk in range(0, 41):
        for tail in (0, 1, 15):
            if nblk == 0 and tail == 0:
                msg = b""
            else:
                msg = rng.bytes(16 * nblk + tail) if tail else rng.bytes(16 * nblk)
            key = rng.bytes(32)
            for op in ("mac", "row"):
                lines.append(f"{op} {key.hex()} {hx(msg)}")
                want.append(aead_ref.poly1305(key, msg).hex())
    assert run(prog, lines) == want
