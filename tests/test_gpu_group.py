"""The layer between the field and the verify chain on the MI355X, each piece
against an exact Python-integer model (tests/pyref_group.py): loose-limb field
products at the bounds of fdgpu_fe.h's classes, every group operation of
fdgpu_ge.h against textbook addition on the points where formulas go wrong,
the two scalar recodings of fdgpu_sc.h, the fixed-base comb table entry by
entry, and signatures that drive the product comb to its edge entries.  All
comparisons are exact."""
import random
import time

import numpy as np
import pytest

import pyref_ed25519 as ref
import pyref_group as pg
from conftest import load_json
from firedancer_amd import VerifyEngine, ed25519 as ed, workload
from pyref_ed25519 import L, P

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ 1. raw limbs
def test_fe_raw_ops_at_the_class_bounds(engine):
    # the all-maximum inputs sit at the header's limits, not beyond them
    for a, b in pg.MUL_PAIRS:
        fm, gm = pg.CLASS_LIMIT[a], pg.CLASS_LIMIT[b]
        print(a, b, "267 max f max g = 2^%.3f" % np.log2(267.0 * max(fm) * max(gm)), "2 f = 2^%.3f" % np.log2(2.0 * max(fm)),
              "19 g = 2^%.3f" % np.log2(19.0 * max(gm)))
        assert 267 * max(fm) * max(gm) < 1 << 64 and 2 * max(fm) < 1 << 32 and 19 * max(gm) < 1 << 32
    recs = pg.fe_raw_records()
    assert len(recs) % 64 == 1 and len(recs) > 64
    out = engine.debug_fe_raw(recs)
    bad, checked = [], dict.fromkeys(pg.FE_RAW_OPS, 0)
    for i, r in enumerate(recs):
        exp = pg.fe_raw_expected(r[:10], r[10:])
        for k, name in enumerate(pg.FE_RAW_OPS):
            if exp[name] is None:
                continue
            checked[name] += 1
            if pg.words_value(out[i, k]) != exp[name]:
                bad.append((i, name, [int(v) for v in r[:10]], [int(v) for v in r[10:]]))
    print("records", len(recs), "checked", checked)
    assert all(n >= 100 for n in checked.values()), checked
    assert not bad, f"{len(bad)} results differ, first: {bad[0]}"


# ------------------------------------------------------- 2. group operations
# result index -> what it must equal, and whether it is a p2 result (T = 0)
GE_EXPECT = ["2P", "2P", "P+Q", "P-Q", "P+Q", "P-Q", "P+Q", "P-Q", "P+Q", "P-Q", "P+Q", "P-Q", "P+Q", "P-Q",
             "Q", "-Q", "Q", "-Q", "-P", "16P+2Q", "16P"]
GE_P2 = {1, 14, 15}
GE_NAMES = ["dbl->p3", "dbl->p2", "add_cached", "add_cached neg", "add_cached_ld", "add_cached_ld neg",
            "add_cached_regs", "add_cached_regs neg", "add_cached_regs_swapped", "add_cached_regs_swapped neg",
            "add_niels", "add_niels neg", "add_niels_regs", "add_niels_regs neg", "cached_regs_to_p2",
            "cached_regs_to_p2 neg", "niels_regs_to_p3", "niels_regs_to_p3 neg", "p3_neg", "window +Q +Q", "window +Q -Q"]
KINDS = [(c, k) for c in range(4) for k in ("one", "minus_one", "noncanon")]


def _points(rnd):
    tors = pg.torsion_points()
    named = tors + [ref.B, pg.neg(ref.B), pg.affine(ref._mul(2, ref.B)), pg.affine(ref._mul(L - 1, ref.B))]
    rand = [pg.affine(ref._mul(rnd.randrange(1, L), ref.B)) for _ in range(24)]
    rand += [pg.affine(ref._add(ref._mul(rnd.randrange(1, L), ref.B), tors[1 + i % 7])) for i in range(16)]
    assert all(pg.on_curve(p) for p in named + rand)
    return named, rand


def _representative(pt, kind, rnd):
    """pt scaled so that coordinate c becomes 1, p - 1 or a small residue; the
    small residues of the last kind are then written as residue + p."""
    if kind is None:
        return pt, False
    c, how = kind
    target = {"one": 1, "minus_one": P - 1, "noncanon": rnd.randint(1, 18)}[how]
    lam = target * ref._inv(pt[c]) % P if pt[c] % P else rnd.randrange(1, P)
    return pg.rescale(pt, lam), how == "noncanon"


def _coord_words(v, noncanon):
    return pg.value_words(v + P if noncanon and v < 19 else v)       # v + p < 2^255 only for v < 19


def _ge_case(Pt, Qt, kind, rnd):
    Pr, nc = _representative(Pt, kind, rnd)
    Qr, _ = _representative(Qt, kind, rnd)
    words = [_coord_words(v, nc) for v in Pr + Qr] + [pg.value_words(v) for v in pg.niels(Qt)]
    return np.concatenate(words)


def test_ge_ops_equal_textbook_addition(engine):
    rnd = random.Random(0x6E0)
    named, rand = _points(rnd)
    pairs = [(a, b) for a in named for b in named]
    n_named = len(pairs)
    every = named + rand
    pairs += [(rnd.choice(every), rnd.choice(every)) for _ in range(300)]
    cases = []                                   # (pair index, kind)
    for pi in range(len(pairs)):
        kinds = [None] + (KINDS if pi < n_named else rnd.sample(KINDS, 2))
        cases += [(pi, k) for k in kinds]
    w_in, n_res = ed.ge_ops_shape()
    assert (w_in, n_res) == (88, len(GE_EXPECT))
    while len(cases) % 64 != 1:                  # a partial wave at the end
        cases.append((rnd.randrange(len(pairs)), rnd.choice(KINDS)))
    rec = np.stack([_ge_case(*pairs[pi], k, rnd) for pi, k in cases])
    # the noncanonical representatives really are in [p, 2^255)
    assert any(pg.words_value(rec[i, 8 * c:8 * c + 8]) >= P for i in range(len(rec)) for c in range(8))
    out = engine.debug_ge_ops(rec)
    flat = out.reshape(len(rec), n_res, 4, 8)
    expected = {}
    bad = []
    for i, (pi, kind) in enumerate(cases):
        if pi not in expected:
            Pt, Qt = pairs[pi]
            p16 = ref._mul(16, Pt)
            expected[pi] = {"2P": ref._add(Pt, Pt), "P+Q": ref._add(Pt, Qt), "P-Q": ref._add(Pt, pg.neg(Qt)), "Q": Qt,
                            "-Q": pg.neg(Qt), "-P": pg.neg(Pt), "16P+2Q": ref._add(p16, ref._add(Qt, Qt)), "16P": p16}
        for r in range(n_res):
            X, Y, Z, T = (pg.words_value(flat[i, r, c]) for c in range(4))
            Xe, Ye, Ze, _ = expected[pi][GE_EXPECT[r]]
            ok = max(X, Y, Z, T) < P and Z != 0 and (X * Ze - Xe * Z) % P == 0 and (Y * Ze - Ye * Z) % P == 0
            ok = ok and (T == 0 if r in GE_P2 else (T * Z - X * Y) % P == 0)
            if not ok:
                bad.append((GE_NAMES[r], "pair", pi, "named" if pi < n_named else "random", "representative", kind))
    print("records", len(rec), "pairs", len(pairs), "results compared", len(rec) * n_res)
    assert not bad, f"{len(bad)} results differ, first: {bad[:5]}"


# ------------------------------------------------------------- 3. recodings
def _recode_scalars():
    rnd = random.Random(0x5C)
    trunc = lambda x: x & ((1 << 252) - 1)                          # noqa: E731  below 2^252 < L
    slots = lambda v, w: sum(v << (w * i) for i in range(256 // w))  # noqa: E731
    xs = [0, 1, L - 1, 2**252, 2**252 - 1, 2**253 - 1]
    for pat in (slots(0x7fff, 16), slots(0x8000, 16), slots(7, 4), slots(8, 4)):
        xs += [pat, trunc(pat)]
    for i in range(16):
        xs += [trunc(0x8000 << (16 * i)), trunc(0xffffffff << (16 * i)), trunc(0xffff << (16 * i))]
    xs += [rnd.randrange(L) for _ in range(1000)]
    while len(xs) % 64 != 1:
        xs.append(rnd.randrange(L))
    return xs


def test_sc_recodings_equal_the_signed_digit_model(engine):
    d = ed.bcomb_dims()
    w, ndig = d["w"], d["ndig"]
    slot = 16 if w <= 16 else 32
    xs = _recode_scalars()
    sb = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype=np.uint8).reshape(-1, 32)
    out = engine.debug_sc_recode(sb)
    n16 = ncomb = 0
    for i, x in enumerate(xs):
        # each function on its stated domain: sc_recode16 k < 2^253, the comb S < 2^(W NDIG - 1)
        if x < 1 << 253:
            got = pg.unpack_digits(out[i, :8], 4, 64)
            assert all(-8 <= v < 8 for v in got) and sum(v << (4 * j) for j, v in enumerate(got)) == x, hex(x)
            assert got == pg.signed_digits(x, 4, 64), hex(x)
            n16 += 1
        if x < 1 << (w * ndig - 1):
            got = pg.unpack_digits(out[i, 8:8 + (ndig * slot + 31) // 32], slot, ndig)
            half = 1 << (w - 1)
            assert all(-half <= v < half for v in got) and sum(v << (w * j) for j, v in enumerate(got)) == x, hex(x)
            assert got == pg.signed_digits(x, w, ndig), hex(x)
            ncomb += 1
    assert n16 >= 1000 and ncomb >= 1000 and L - 1 in xs and 2**253 - 1 in xs


# ------------------------------------------------------------ 4. comb table
def test_comb_table_every_entry(engine):
    d = ed.bcomb_dims()
    assert (d["w"], d["ndig"], d["entries"], d["stride"]) == (16, 16, 32769, 32)
    tab = engine.debug_btab()
    assert tab.shape == (d["ndig"], d["entries"], d["stride"])
    t0 = time.time()
    msg = pg.check_table(tab, d["w"], d["chunk"])      # all 16 x 32,769 entries
    print("table model walk and compare: %.1f s" % (time.time() - t0))
    assert msg is None, msg


# ------------------------------------------- 5. the product comb's edge entries
LANES = (0, 63, 64)
BATCH = 130                                        # two waves and a partial one


@pytest.fixture(scope="module")
def edge_vectors():
    g = load_json("comb_edge_vectors.json")
    assert pg.vectors_digest(g["vectors"]) == g["sha256"]
    return [(v["path"], bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["pub"])) for v in g["vectors"]]


@pytest.fixture(scope="module")
def padding():
    arena, txns, modes = workload.cfg1(BATCH, seed=0xC03B)
    a = arena.tobytes()
    recs = [(a[t["msg_off"]:t["msg_off"] + t["msg_sz"]], a[t["sig_off"]:t["sig_off"] + 64], a[t["pub_off"]:t["pub_off"] + 32])
            for t in txns]
    return recs, modes == 0


def _run_edge(eng, vecs, padding, flip):
    recs0, pad_ok = padding
    for g0 in range(0, len(vecs), len(LANES)):
        group = vecs[g0:g0 + len(LANES)]
        recs = list(recs0)
        for lane, (_, msg, sig, pub) in zip(LANES, group):
            recs[lane] = ((msg[:-1] + bytes([msg[-1] ^ 1])) if flip else msg, sig, pub)
        arena, txns = workload.pack_single(recs)
        got = eng.verify_txns(arena, txns)
        lanes = list(LANES[:len(group)])
        want = ed.ERR_MSG if flip else ed.SUCCESS
        assert got[lanes].tolist() == [want] * len(lanes), (g0, got[lanes].tolist())
        rest = np.ones(BATCH, dtype=bool)
        rest[lanes] = False
        assert ((got == 0) == pad_ok)[rest].all(), g0


@pytest.mark.parametrize("name,flags", [("default", {}), ("key_cache", {"key_cache": True}), ("pair", {"pair": True}),
                                        ("full_path", {"full_path": True})])
def test_comb_edge_signatures(name, flags, edge_vectors, padding):
    vecs = [v for v in edge_vectors if name != "full_path" or v[0] == "full"]
    assert len(vecs) == (46 if name == "full_path" else 92)
    eng = VerifyEngine(0, max_txn=1 << 10, **flags)
    try:
        _run_edge(eng, vecs, padding, flip=False)
        _run_edge(eng, vecs, padding, flip=True)
    finally:
        eng.close()
