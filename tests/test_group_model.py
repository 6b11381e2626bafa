"""The models of tests/pyref_group.py against plain integer arithmetic, and
the comb edge fixture (tests/golden/comb_edge_vectors.json), on the CPU: what
tests/test_gpu_group.py compares the kernels with must itself be right."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import pyref_ed25519 as ref
import pyref_group as pg
from conftest import load_json
from pyref_ed25519 import L, P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, NDIG, ENT, CHUNK = 16, 16, 32769, 64      # the comb's shape (csrc/fdgpu_internal.h); the GPU test reads the library's


def test_limb_value_model_equals_int_arithmetic():
    rnd = random.Random(1)
    for x in [0, 1, 19, P - 1, P, P + 18, 2**255 - 1] + [rnd.randrange(2**255) for _ in range(200)]:
        lim = pg.limbs_of(x)
        assert all(v < 1 << w for v, w in zip(lim, pg.WIDTH))
        assert sum(v << p for v, p in zip(lim, pg.POS)) == x and pg.limbs_value(lim) == x % P
        assert pg.canonical_limbs_to_ints(np.array([lim], dtype=np.uint32)) == [x]
    # loose limbs: the weights alone decide the value
    for _ in range(200):
        lim = [rnd.randrange(1 << 31) for _ in range(10)]
        assert pg.limbs_value(lim) == sum(v * 2**(25 * i + (i + 1) // 2) for i, v in enumerate(lim)) % P
    assert pg.limbs_value(pg.P2) == pg.limbs_value(pg.P4) == pg.limbs_value(pg.limbs_of_kp(1)) == 0
    assert sum(v << p for v, p in zip(pg.P2, pg.POS)) == 2 * P and sum(v << p for v, p in zip(pg.P4, pg.POS)) == 4 * P


def test_fe_raw_records_stay_inside_the_contract():
    """The all-maximum inputs of every admitted pair sit at the header's
    limits and not beyond, and every record has at least its plain results
    expected; each conditional operation is expected somewhere."""
    for a, b in pg.MUL_PAIRS:
        assert pg.mul_conditions(pg.CLASS_LIMIT[a], pg.CLASS_LIMIT[b]) == (True, True, True), (a, b)
        assert pg.mul_in_contract(pg.CLASS_MAX[a], pg.CLASS_MAX[b])
    assert not pg.mul_in_contract(pg.CLASS_MAX["S4"], pg.CLASS_MAX["S"])
    assert not pg.mul_in_contract(pg.CLASS_MAX["S"], pg.CLASS_MAX["S4"])
    recs = pg.fe_raw_records()
    assert len(recs) % 64 == 1
    seen = dict.fromkeys(pg.FE_RAW_OPS, 0)
    for r in recs:
        exp = pg.fe_raw_expected(r[:10], r[10:])
        assert exp["canon"] is not None and exp["add"] is not None
        for k, v in exp.items():
            seen[k] += v is not None
    assert all(n >= 100 for n in seen.values()), seen


@pytest.mark.parametrize("w,n,top", [(4, 64, 2**253 - 1), (16, 16, L - 1)])
def test_recoding_model_round_trip(w, n, top):
    rnd = random.Random(2)
    half = 1 << (w - 1)
    for x in [0, 1, half - 1, half, L - 1, 2**252, 2**252 - 1, top] + [rnd.randrange(L) for _ in range(500)]:
        d = pg.signed_digits(x, w, n)
        assert all(-half <= v < half for v in d) and sum(v << (w * i) for i, v in enumerate(d)) == x
        # the carry form of the same recoding
        c, e = 0, []
        for i in range(n):
            t = ((x >> (w * i)) & ((1 << w) - 1)) + c
            c = 1 if t >= half else 0
            e.append(t - (c << w))
        assert e == d and c == 0
    assert pg.signed_digits(half << (w * (n - 1)), w, n) is None      # past the top digit's range
    packed = [0x8000ffff, 0x00017fff]
    assert pg.unpack_digits(packed, 16, 4) == [-1, -32768, 32767, 1]


def test_torsion_points_have_their_orders():
    pts = pg.torsion_points()
    assert len({pg.encode(p) for p in pts}) == 8 and all(pg.on_curve(p) for p in pts)
    order = lambda p: next(k for k in (1, 2, 4, 8) if ref._eq(ref._mul(k, p), pg.O))   # noqa: E731
    assert [order(p) for p in pts] == [1, 2, 4, 4, 8, 8, 8, 8]


def test_table_model_first_and_last_entries():
    bases = pg.comb_bases(W, NDIG)
    for i in (0, 1, NDIG - 1):
        assert ref._eq(bases[i], ref._mul(1 << (W * i), ref.B))
    for i in (0, NDIG - 1):
        pts = list(pg.table_points(bases[i], ENT))
        for j in (0, 1, 2, CHUNK - 1, CHUNK, ENT - 2, ENT - 1):
            assert ref._eq(pts[j], ref._mul(j << (W * i), ref.B)) and pg.on_curve(pts[j]), (i, j)


def test_table_check_accepts_the_model_and_names_a_bad_entry():
    """A small comb of the same layout: the check passes on the model's own
    table and reports position and kind of a planted error."""
    w, ndig, ent, chunk = 4, 3, 9, 4
    tab = pg.model_table(w, ndig, ent)
    assert pg.check_table(tab, w, chunk) is None
    for (i, j), kind in (((1, 8), "alone in its chunk"), ((2, 4), "a chunk's first"), ((0, 3), "a chunk's last")):
        bad = tab.copy()
        bad[i, j, 20] ^= 1
        msg = pg.check_table(bad, w, chunk)
        assert msg and f"table {i} entry {j} " in msg and kind in msg, msg
    bad = tab.copy()
    bad[1, 2, 31] = 1
    assert "canonical" in pg.check_table(bad, w, chunk)
    bad = tab.copy()
    bad[1, 2, 3] |= 1 << 25                       # an odd limb past its 25 bits
    assert "canonical" in pg.check_table(bad, w, chunk)
    sel = pg.subset_select(NDIG, ENT, CHUNK)
    assert sel(0, 5000) and sel(7, 129) and not sel(7, 130) and sel(7, 64 * 9) and sel(7, 64 * 9 + 63) and sel(7, 32640)


@pytest.fixture(scope="module")
def host_v(tmp_path_factory):
    """v of the host build of the half-size split (signed), None where it fails."""
    so = str(tmp_path_factory.mktemp("latgrp") / "liblattice.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    os.path.join(REPO, "tests", "native", "lattice_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.hs_split_host.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int]

    def v_of(k):
        kb = (ctypes.c_uint32 * 8)(*[(k >> (32 * i)) & 0xffffffff for i in range(8)])
        u, v, f = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 4)()
        lib.hs_split_host(kb, u, v, f, 0)
        if not f[0]:
            return None
        val = sum(int(x) << (32 * i) for i, x in enumerate(v))
        return -val if f[2] else val
    return v_of


def test_comb_edge_vectors(host_v):
    """Every vector is a valid signature, its comb scalar (S on the full
    path, v S mod L on the half-size one) has the digit it claims where it
    claims it, every target is present, and the file is the recorded one."""
    g = load_json("comb_edge_vectors.json")
    vec = g["vectors"]
    assert pg.vectors_digest(vec) == g["sha256"] and (g["w"], g["ndig"]) == (W, NDIG)
    want = {(p, i, d) for p in ("full", "half") for i in range(NDIG - 1) for d in (-32768, 0, 32767)}
    want |= {(p, NDIG - 1, 0) for p in ("full", "half")}
    assert {(v["path"], v["pos"], v["digit"]) for v in vec} == want and len(vec) == len(want)
    for v in vec:
        msg, sig, pub = (bytes.fromhex(v[k]) for k in ("msg", "sig", "pub"))
        assert ref.verify(msg, sig, pub) == ref.SUCCESS
        S = int.from_bytes(sig[32:], "little")
        x = S
        if v["path"] == "half":
            hv = host_v(pg.hram(sig[:32], pub, msg))
            assert hv is not None
            x = hv * S % L
        assert pg.signed_digits(x, W, NDIG)[v["pos"]] == v["digit"], v
