"""Writes tests/golden/comb_edge_vectors.json: valid signatures whose
fixed-base comb scalar has a chosen digit at a chosen position, so that the
verify kernels' comb reads the table entries a random signature practically
never does: entry 32768 (digit -32768), entry 0 (digit 0) and entry 32767.

The key and the nonce are fixed (seeded below), so A and R are fixed and one
point multiplication each is all the curve work; only the message varies
(a counter), and with it k = SHA-512(R || A || M) mod L and S = r + k a.
  path "full"  the comb's scalar is S (the engine's full_path=True)
  path "half"  the comb's scalar is w = v S mod L, v from the half-size split
               of k (csrc/fdgpu_lattice.h, built for the host from
               tests/native/lattice_host.cpp); a k whose split fails is passed over
Targets, per path: digits -32768, 0 and 32767 at each of the positions 0..14
and digit 0 at position 15 (the only one of the three a scalar below L can
have there).  The first message that meets a target is kept.

    python tests/golden/make_comb_golden.py

Deterministic; CPU only.  Measured run time: 6.6 s on one x86-64 core
(301,882 messages tried for the 92 vectors).
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import pyref_ed25519 as ref          # noqa: E402
import pyref_group as pg             # noqa: E402

OUT = os.path.join(HERE, "comb_edge_vectors.json")
SEED = b"fdgpu comb edge vectors v1"
W, NDIG = 16, 16
L = ref.L


def host_split_lib(tmpdir):
    so = os.path.join(tmpdir, "liblattice.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    os.path.join(REPO, "tests", "native", "lattice_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.hs_split_host.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int]
    return lib


class HostSplit:
    """hs_split of the host build: k -> signed v, or None where the split fails."""

    def __init__(self, lib):
        self.lib = lib
        self.k = (ctypes.c_uint32 * 8)()
        self.u, self.v, self.f = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 4)()

    def v_of(self, k):
        ctypes.memmove(self.k, k.to_bytes(32, "little"), 32)
        self.lib.hs_split_host(self.k, self.u, self.v, self.f, 0)
        if not self.f[0]:
            return None
        v = int.from_bytes(bytes(self.v), "little")
        return -v if self.f[2] else v


def comb_scalar(split, k, S, path):
    """The scalar the comb recodes for this signature on this path (None: the
    half-size split fails and the lane takes the full-length chain)."""
    if path == "full":
        return S
    v = split.v_of(k)
    return None if v is None else v * S % L


def main():
    t0 = time.time()
    a = int.from_bytes(hashlib.sha512(SEED + b" key").digest(), "little") % L
    r = int.from_bytes(hashlib.sha512(SEED + b" nonce").digest(), "little") % L
    pub, r_enc = pg.encode(ref._mul(a, ref.B)), pg.encode(ref._mul(r, ref.B))
    want = {}
    for path in ("full", "half"):
        for pos in range(NDIG - 1):
            for digit in (-32768, 0, 32767):
                want[(path, pos, digit)] = None
        want[(path, NDIG - 1, 0)] = None
    # offset form of the recoding (pyref_group.signed_digits): the plain digits of x + OFF are the signed ones + 2^15
    OFF = sum(0x8000 << (W * i) for i in range(NDIG))
    slot = {0x0000: -32768, 0x8000: 0, 0xffff: 32767}
    left, tries = len(want), 0
    with tempfile.TemporaryDirectory() as tmp:
        split = HostSplit(host_split_lib(tmp))
        while left:
            msg = SEED + tries.to_bytes(8, "little")
            tries += 1
            k = pg.hram(r_enc, pub, msg)
            S = (r + k * a) % L
            for path in ("full", "half"):
                x = comb_scalar(split, k, S, path)
                if x is None:
                    continue
                y = x + OFF
                for pos in range(NDIG):
                    d = slot.get((y >> (W * pos)) & 0xffff)
                    key = (path, pos, d)
                    if d is not None and key in want and want[key] is None:
                        assert pg.signed_digits(x, W, NDIG)[pos] == d
                        want[key] = {"path": path, "pos": pos, "digit": d, "msg": msg.hex(),
                                     "sig": (r_enc + S.to_bytes(32, "little")).hex(), "pub": pub.hex()}
                        left -= 1
    vectors = [want[k] for k in sorted(want)]
    for v in vectors:
        assert ref.verify(bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["pub"])) == 0
    with open(OUT, "w") as f:
        json.dump({"seed": SEED.decode(), "w": W, "ndig": NDIG, "sha256": pg.vectors_digest(vectors),
                   "vectors": vectors}, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(vectors)} vectors, {tries} messages tried, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
