"""Generate tests/golden/aead_vectors.json -- committed vectors for the
transport AEAD (wgcs_aead_seal / wgcs_aead_open and their batch forms).

The sealed messages come from a third-party implementation, the local
OpenSSL's EVP_chacha20_poly1305 (tests/aead_ref.py: Libcrypto), and every one
is cross-checked here against the pure-Python restatement of RFC 8439.  They
are WireGuard-shaped: nonce = 4 zero bytes | LE64 counter, no additional data,
the packet zero-padded as device/send.go:529-560 says.  The file lets the GPU
tests check the product on a machine that has no libcrypto.

Packets of up to 300 bytes are stored in full.  Larger ones are the stated
pattern  byte i = (i * mul + add) & 0xFF  and the file keeps the message's
length, tag, first and last 16 ciphertext bytes and SHA-256.

usage: python tests/golden/make_aead_golden.py   (rewrites aead_vectors.json)
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import aead_ref  # noqa: E402

SEED = 8439
OUT = os.path.join(HERE, "aead_vectors.json")
SMALL = 300


def pattern(n: int, mul: int, add: int) -> bytes:
    return ((np.arange(n, dtype=np.uint64) * np.uint64(mul) + np.uint64(add)) & np.uint64(0xFF)).astype(np.uint8).tobytes()


def generate(lc) -> dict:
    rng = np.random.default_rng(SEED)
    counters = [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
    cases = []
    small = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 239, 240, 241, 255, 256, 257, 300]
    large = [1023, 1024, 1025, 1419, 1420, 1424, 1500, 3000, 4095, 4096, 4097, 65487]
    for k, n in enumerate(small + large):
        key = rng.bytes(32)
        remote_index = int(rng.integers(0, 2**32))
        counter = counters[k % len(counters)] if k % 3 else int(rng.integers(0, 2**64, dtype=np.uint64))
        mtu = 0 if n == 65487 else (0, 1420, 1500)[k % 3]
        rec = {"key": key.hex(), "remote_index": remote_index, "counter": counter, "mtu": mtu, "len": n}
        if n <= SMALL:
            packet = rng.bytes(n)
            rec["packet_hex"] = packet.hex()
        else:
            rec["pattern"] = [int(rng.integers(1, 256)) | 1, int(rng.integers(0, 256))]
            packet = pattern(n, *rec["pattern"])
        msg = aead_ref.wg_seal(key, remote_index, counter, packet, mtu, seal=lc.seal)
        assert msg == aead_ref.wg_seal(key, remote_index, counter, packet, mtu), "libcrypto != RFC 8439 restatement"
        assert len(msg) == 32 + n + aead_ref.padding(n, mtu)
        if n <= SMALL:
            rec["msg_hex"] = msg.hex()
        else:
            rec.update(msg_len=len(msg), tag=msg[-16:].hex(), ct_first=msg[16:32].hex(), ct_last=msg[-32:-16].hex(),
                       msg_sha256=hashlib.sha256(msg).hexdigest())
        cases.append(rec)
    rfc = {  # RFC 8439 §2.8.2, the AEAD's own vector (not WireGuard-shaped: 12-byte AAD)
        "key": bytes(range(0x80, 0xA0)).hex(), "nonce": "070000004041424344454647", "aad": "50515253c0c1c2c3c4c5c6c7",
        "plaintext": ("Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
                      "sunscreen would be it."),
        "tag": "1ae10b594f09e26a7e902ecbd0600691",
    }
    sealed = lc.seal(bytes.fromhex(rfc["key"]), bytes.fromhex(rfc["nonce"]), rfc["plaintext"].encode(),
                     bytes.fromhex(rfc["aad"]))
    assert sealed[-16:].hex() == rfc["tag"]
    rfc["ciphertext"] = sealed[:-16].hex()
    return {"generator": "tests/golden/make_aead_golden.py", "seed": SEED, "source": "OpenSSL EVP_chacha20_poly1305",
            "rfc8439_2_8_2": rfc, "cases": cases}


def dumps(g: dict) -> str:
    return json.dumps(g, separators=(",", ":"))


def expand(rec: dict) -> tuple[bytes, bytes | None]:
    """(packet, message or None) of a case; large cases carry no full message."""
    if "packet_hex" in rec:
        return bytes.fromhex(rec["packet_hex"]), bytes.fromhex(rec["msg_hex"])
    return pattern(rec["len"], *rec["pattern"]), None


def main():
    lc = aead_ref.libcrypto()
    if lc is None:
        raise SystemExit("no libcrypto with EVP_chacha20_poly1305 on this machine")
    with open(OUT, "w") as f:
        f.write(dumps(generate(lc)))
    print(os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
