"""Generate tests/golden/x25519_vectors.json -- committed vectors for X25519
(wgcs_x25519 and wgcs_x25519_batch).

The shared secrets come from a third-party implementation, the local OpenSSL
(`openssl pkeyutl -derive`), which takes the raw 32-byte keys wrapped in their
fixed DER headers (RFC 8410: PKCS#8 for the private key, SubjectPublicKeyInfo
for the peer's).  Every one is cross-checked here against the pure-Python
ladder of tests/noise_ref.py.  The scalars are random bytes, unclamped, and
every other u has bit 255 set: both sides must clamp and mask on their own.
The file lets the tests check the product on a machine that has no openssl;
the tests read the JSON and never call openssl.

usage: python tests/golden/make_x25519_golden.py   (rewrites x25519_vectors.json)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import noise_ref  # noqa: E402

SEED = 7748
COUNT = 300
OUT = os.path.join(HERE, "x25519_vectors.json")
PKCS8_X25519 = bytes.fromhex("302e020100300506032b656e04220420")  # PrivateKeyInfo { v0, id-X25519, OCTET STRING { OCTET STRING
SPKI_X25519 = bytes.fromhex("302a300506032b656e032100")           # SubjectPublicKeyInfo { id-X25519, BIT STRING


def derive(openssl: str, td: str, scalar: bytes, u: bytes) -> bytes:
    priv, pub, out = (os.path.join(td, name) for name in ("priv.der", "pub.der", "secret.bin"))
    with open(priv, "wb") as f:
        f.write(PKCS8_X25519 + scalar)
    with open(pub, "wb") as f:
        f.write(SPKI_X25519 + u)
    subprocess.run([openssl, "pkeyutl", "-derive", "-keyform", "DER", "-inkey", priv, "-peerform", "DER", "-peerkey",
                    pub, "-out", out], check=True, capture_output=True)
    with open(out, "rb") as f:
        return f.read()


def generate(openssl: str) -> dict:
    rng = np.random.default_rng(SEED)
    cases = []
    with tempfile.TemporaryDirectory() as td:
        for i in range(COUNT):
            scalar, u = rng.bytes(32), bytearray(rng.bytes(32))
            u[31] = (u[31] | 0x80) if i % 2 else (u[31] & 0x7F)
            u = bytes(u)
            secret = derive(openssl, td, scalar, u)
            assert secret == noise_ref.x25519_raw(scalar, u), "openssl != RFC 7748 restatement"
            cases.append({"scalar": scalar.hex(), "u": u.hex(), "out": secret.hex()})
    version = subprocess.run([openssl, "version"], capture_output=True, text=True, check=True).stdout.strip()
    return {"generator": "tests/golden/make_x25519_golden.py", "seed": SEED, "source": f"{version}: pkeyutl -derive",
            "cases": cases}


def main():
    openssl = shutil.which("openssl")
    if openssl is None:
        raise SystemExit("no openssl on this machine")
    with open(OUT, "w") as f:
        f.write(json.dumps(generate(openssl), separators=(",", ":")))
    print(os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
