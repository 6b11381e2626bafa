"""Exact models of the verify chain's scalar side (csrc/fdgpu_verify.hip:
recode16_160, hs_wscalar, the half / full routing) and the builder of
signatures at a chosen k, for tests/test_chain_model.py (CPU) and
tests/test_gpu_chain.py (the prehashed verify kernels on the GPU).

TEST INFRASTRUCTURE ONLY.  A hash gives uniformly random k: over 20,000 of
them the split yields window counts 31..34 and never fails.  Here k is chosen
(the kernel is handed the SHA-512 state words of a number congruent to k), so
a wave can run 1 window or 40, lanes can fall to the full-length path beside
half-size neighbours, and A can carry a torsion point at every k mod 8.

The split is the product's own (csrc/fdgpu_lattice.h compiled for the host,
tests/native/lattice_host.cpp; tests/test_lattice.py checks it against Python
integers and tests/test_gpu_lattice.py the device against it).  Everything
after it is Python integers, and every expected code is the evaluation of
[S]B == R + [k]A with tests/pyref_ed25519.py's point arithmetic.
"""
import ctypes
import os
import random
import subprocess
import tempfile

import numpy as np

import pyref_ed25519 as ref
import pyref_group as grp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = ref.P, ref.L
N = 8 * L
MAX_WIN = 40                                  # HS_MAX_WIN

SMALL_KS = [0, 1, 2, 7, 8, 9, 15, 16, 2**127, 2**128 - 1]
FAIL_KS = [2**128, 2**128 + 1, L - 1, L - 2, L // 2, 2**252]      # the host split reports ok = 0 for each


# ------------------------------------------------------------ the models
def recode16_160(m):
    """Signed radix-16 digits of 0 <= m < 2^160 -> (40 digits in [-8, 7], nd):
    nd counts the digits up to the highest nonzero one, 41 if a carry is left."""
    assert 0 <= m < 1 << 160
    digits, carry, nd = [], 0, 0
    for i in range(40):
        e = ((m >> (4 * i)) & 15) + carry
        carry = 1 if e >= 8 else 0
        e -= 16 * carry
        digits.append(e)
        if e:
            nd = i + 1
    return digits, (41 if carry else nd)


def wscalar(v, S):
    """hs_wscalar: w = v S mod L for the signed v."""
    return v * S % L


_SPLIT = None


def host_split():
    """k -> (u, v, ok) with signed u, v: hs_split of csrc/fdgpu_lattice.h, built for the host once a process."""
    global _SPLIT
    if _SPLIT is None:
        so = os.path.join(tempfile.mkdtemp(prefix="chainlat"), "liblattice.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                        os.path.join(REPO, "tests", "native", "lattice_host.cpp"), "-o", so], check=True)
        lib = ctypes.CDLL(so)
        lib.hs_split_host.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int]

        def split(k):
            kb = (ctypes.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
            u, v, f = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 4)()
            lib.hs_split_host(kb, u, v, f, 0)
            uu = sum(int(x) << (32 * i) for i, x in enumerate(u))
            vv = sum(int(x) << (32 * i) for i, x in enumerate(v))
            return (-uu if f[1] else uu), (-vv if f[2] else vv), bool(f[0])
        _SPLIT = split
    return _SPLIT


class Route:
    """Where the verify kernel sends a lane with this k: kind "half" with its
    window count nd (1..40) and the split (u, v), or "full" (the split failed,
    or a recoding left a carry: nd = 41)."""

    def __init__(self, k):
        self.k = k
        self.u, self.v, self.ok = host_split()(k)
        self.nd = max(recode16_160(abs(self.u))[1], recode16_160(abs(self.v))[1], 1) if self.ok else 0
        self.kind = "half" if self.ok and self.nd <= MAX_WIN else "full"

    def __repr__(self):
        return f"Route(k={self.k:#x}, {self.kind}, nd={self.nd}, u={self.u:#x}, v={self.v:#x})"


def route(k):
    return Route(k)


# ------------------------------------------------- k of every route class
def find_classes(seed=0xC4A1):
    """{class: k}: ("half", nd, v < 0) for nd = 1..40 (nd = 1 has v = 1 only),
    ("carry",) for nd = 41, ("fail", j) for some split failures beyond
    FAIL_KS, and ("u_neg",) if the search meets a negative u.  k near the
    rationals 8L m / n (n of every size up to 2^131) have partial quotients
    as large as wanted, which is what moves the stop of Euclid and with it
    the sizes of u and v."""
    rnd = random.Random(seed)
    found = {}
    want = {("half", 1, False), ("carry",)} | {("half", nd, s) for nd in range(2, 41) for s in (False, True)}
    want |= {("fail", j) for j in range(4)}

    def note(k):
        r = Route(k)
        if r.ok and r.u < 0:
            found.setdefault(("u_neg",), k)
        if not r.ok:
            j = sum(1 for c in found if c[0] == "fail")
            if j < 4 and k not in FAIL_KS and k not in found.values():
                found[("fail", j)] = k
        elif r.nd == 41:
            found.setdefault(("carry",), k)
        else:
            found.setdefault(("half", r.nd, r.v < 0), k)

    for k in range(1, 8):
        note(k)
    for rounds in range(40):
        for bits in range(1, 132):
            n = rnd.randrange(1 << (bits - 1), 1 << bits)
            m = rnd.randrange(1, n + 1)
            for off in (0, 1, -1, rnd.randrange(-1000, 1000), rnd.randrange(-2**40, 2**40), rnd.randrange(-2**100, 2**100)):
                note((N * m // n + off) % L)
        if want <= set(found):
            break
    return found


# ------------------------------------------------------- record builder
_MUL = {}


def mul(s, pt):
    """[s]pt by pyref_ed25519._mul, remembered (the variants of one k share their products)."""
    key = (s, pt)
    if key not in _MUL:
        _MUL[key] = ref._mul(s, pt)
    return _MUL[key]


def state_bytes(x):
    """The 64 arena bytes of the SHA-512 state whose digest is LE(x): eight
    big-endian 64-bit words, each stored as the device's native uint64."""
    d = x.to_bytes(64, "little")
    return b"".join(d[8 * j:8 * j + 8][::-1] for j in range(8))


def state_value(b):
    """The kernel's reading of 64 state bytes: the digest as a little-endian integer."""
    return int.from_bytes(b"".join(b[8 * j:8 * j + 8][::-1] for j in range(8)), "little")


def lift(k, which):
    """x = k (mod L) below 2^512: k itself, k + L, or the largest such."""
    return (k, k + L, k + L * ((2**512 - 1 - k) // L))[which % 3]


def expected_code(A, R, S, k):
    """The reference's verdict on decoded points: pass 1 in pyref_ed25519._pass1's order (S < L; a decode failure
    cannot occur, the points are encoded here), then [S]B == R + [k]A, evaluated."""
    if S >= L:
        return ref.ERR_SIG
    if ref._small_order(A):
        return ref.ERR_PUBKEY
    if ref._small_order(R):
        return ref.ERR_SIG
    return ref.SUCCESS if ref._eq(mul(S, ref.B), ref._add(R, mul(k, A))) else ref.ERR_MSG


class Record:
    __slots__ = ("k", "kind", "a", "r", "S", "A", "R", "pub", "sig", "state", "code", "tors")

    def __init__(self, k, kind, a, r, S, A, R, x_choice, tors=None):
        self.k, self.kind, self.a, self.r, self.S, self.A, self.R, self.tors = k, kind, a, r, S, A, R, tors
        self.pub = grp.encode(A)
        self.sig = grp.encode(R) + S.to_bytes(32, "little")
        self.state = state_bytes(lift(k, x_choice))
        self.code = expected_code(A, R, S, k)


class RecordSet:
    """Records at chosen k, seeded.  Per k: a, r random in [1, L), A = aB,
    R = rB, S = r + k a mod L ("valid"); S + 1 ("bad"); S = 0 with r = -k a
    ("szero").  tors[k mod 8]: A + T for the 8 torsion points T, each with S
    and S + 1."""

    def __init__(self, seed=0xC4A1):
        self.rnd = random.Random(seed)
        self.classes = find_classes(seed)
        self.records = []
        self.by_k = {}            # k -> indices of its records
        self.tors = {}            # k mod 8 -> indices
        ks = list(SMALL_KS) + list(FAIL_KS) + [self.classes[c] for c in sorted(self.classes)]
        self.ks = list(dict.fromkeys(ks))
        self.routes = {k: route(k) for k in self.ks}
        for k in self.ks:
            self._add_k(k)
        # a half-size k of every residue mod 8 for the torsion set: 9 .. 16 are
        # one or two windows, so these take count-33 scalars as a hash would give
        for res in range(8):
            while True:
                k = self.rnd.randrange(L) & ~7 | res
                rt = route(k)
                if rt.kind == "half":
                    break
            self.routes[k] = rt
            self._add_tors(k)
        self.expected = np.array([r.code for r in self.records], dtype=np.int8)

    def _new(self, *a, **kw):
        rec = Record(*a, x_choice=len(self.records), **kw)
        self.records.append(rec)
        self.by_k.setdefault(rec.k, []).append(len(self.records) - 1)
        return len(self.records) - 1

    def _add_k(self, k):
        a, r = self.rnd.randrange(1, L), self.rnd.randrange(1, L)
        A, R, S = mul(a, ref.B), mul(r, ref.B), (r + k * a) % L
        self._new(k, "valid", a, r, S, A, R)
        self._new(k, "bad", a, r, (S + 1) % L, A, R)
        r0 = -k * a % L
        self._new(k, "szero", a, r0, 0, A, mul(r0, ref.B))

    def _add_tors(self, k):
        a, r = self.rnd.randrange(1, L), self.rnd.randrange(1, L)
        A, R, S = mul(a, ref.B), mul(r, ref.B), (r + k * a) % L
        idx = []
        for t, T in enumerate(grp.torsion_points()):
            At = grp.affine(ref._add(A, T))
            idx.append(self._new(k, "tors", a, r, S, At, R, tors=t))
            idx.append(self._new(k, "tors_bad", a, r, (S + 1) % L, At, R, tors=t))
        self.tors[k % 8] = idx

    # ---- selections
    def route_of(self, i):
        return self.routes[self.records[i].k]

    def half_at(self, nd):
        """indices of the records whose lane runs nd windows"""
        return [i for i, rec in enumerate(self.records)
                if self.route_of(i).kind == "half" and self.route_of(i).nd == nd and rec.tors is None]

    def full(self):
        return [i for i in range(len(self.records)) if self.route_of(i).kind == "full"]

    def n_full(self, idx):
        """the fallback queue's count for these lanes: full routes among the lanes that passed pass 1"""
        return sum(1 for i in idx if self.route_of(i).kind == "full" and self.records[i].code in (0, ref.ERR_MSG))

    def n_pass1(self, idx):
        return sum(1 for i in idx if self.records[i].code in (0, ref.ERR_MSG))

    # ---- the arena of the prehashed launch
    def arena(self):
        """(uint8 arena, per-record (state_off, sig_off, pub_off)): record j's 64 state bytes (8-B aligned), its
        signature and its key, 160 B a record."""
        buf = bytearray()
        offs = []
        for rec in self.records:
            o = len(buf)
            buf += rec.state + rec.sig + rec.pub
            offs.append((o, o + 64, o + 128))
        return np.frombuffer(bytes(buf), dtype=np.uint8), offs

    def descs(self, idx, offs, dtype):
        """descriptors of the lanes idx (lane i = record idx[i]; a record may serve many lanes)"""
        d = np.zeros(len(idx), dtype=dtype)
        for lane, i in enumerate(idx):
            d[lane] = (offs[i][0], 0, offs[i][1], offs[i][2])
        return d
