"""tests/pyref_chain.py on the CPU: the scalar models against plain integers,
every class of k that tests/test_gpu_chain.py relies on populated, and every
record's verdict and state words reproducible."""
import random

import pytest

import pyref_chain as pc
import pyref_ed25519 as ref
import pyref_group as grp

L, N = pc.L, pc.N
# the recoding adds 8 to every nibble: a carry is left from 2^160 - 0x88..8 on
CARRY_FROM = 0x7777777777777777777777777777777777777778


@pytest.fixture(scope="module")
def rs():
    return pc.RecordSet()


def test_recode16_160_reconstructs():
    rnd = random.Random(0x16)
    ms = [0, 1, 7, 8, 15, 16, 2**159 - 1, 2**159, 2**160 - 1, 0x8888888888888888888888888888888888888888,
          0x7777777777777777777777777777777777777777, 0x7777777777777777777777777777777777777778]
    ms += [rnd.randrange(1 << b) for b in range(1, 161) for _ in range(4)]
    for m in ms:
        d, nd = pc.recode16_160(m)
        assert len(d) == 40 and all(-8 <= x <= 7 for x in d)
        val = sum(x << (4 * i) for i, x in enumerate(d))
        if nd == 41:
            assert val + (1 << 160) == m and m >= CARRY_FROM
        else:
            assert val == m and m < CARRY_FROM
            assert nd == max((i + 1 for i, x in enumerate(d) if x), default=0)
            assert all(x == 0 for x in d[nd:])
    assert pc.recode16_160(7)[1] == 1 and pc.recode16_160(8)[1] == 2 and pc.recode16_160(0)[1] == 0
    assert pc.recode16_160(CARRY_FROM)[1] == 41 and pc.recode16_160(CARRY_FROM - 1)[1] == 40


def test_wscalar_and_split_relation(rs):
    rnd = random.Random(0x77)
    for k, rt in rs.routes.items():
        if not rt.ok:
            continue
        assert (rt.u - rt.v * k) % N == 0 and rt.v % 2 == 1 and 0 < abs(rt.v) < L, rt
        S = rnd.randrange(L)
        w = pc.wscalar(rt.v, S)
        assert 0 <= w < L and (w - rt.v * S) % L == 0
        assert pc.wscalar(rt.v, 0) == 0
    # k < 2^128: the split is (k, 1)
    for k in (1, 2, 7, 8, 9, 15, 16, 2**127, 2**128 - 1):
        assert (rs.routes[k].u, rs.routes[k].v, rs.routes[k].kind) == (k, 1, "half")


def test_every_class_is_populated(rs):
    for k in pc.SMALL_KS:
        assert rs.routes[k].kind == "half", k
    assert rs.routes[0].u == 0 and rs.routes[0].nd == 1            # the A chain all zeros
    for k in pc.FAIL_KS:
        assert not rs.routes[k].ok, hex(k)
    c = rs.classes
    assert rs.routes[c[("half", 1, False)]].nd == 1
    for nd in range(2, 41):
        for neg in (False, True):
            rt = rs.routes[c[("half", nd, neg)]]
            assert rt.kind == "half" and rt.nd == nd and (rt.v < 0) == neg, (nd, neg, rt)
        assert rs.half_at(nd)
    rt = rs.routes[c[("carry",)]]
    assert rt.ok and rt.nd == 41 and rt.kind == "full"
    for j in range(4):
        assert not rs.routes[c[("fail", j)]].ok
    # hs_take leaves u >= 0 for every candidate: the search meets no negative u
    assert ("u_neg",) not in c and all(rt.u >= 0 for rt in rs.routes.values())
    # k >= 2^128 with v of either sign, S = 0 with v negative (w = 0 and the sign flip)
    assert any(r.kind == "szero" and rs.route_of(i).kind == "half" and rs.route_of(i).v < 0 and r.code == 0
               for i, r in enumerate(rs.records))
    # the torsion set: a half-size k of every residue, eight points, both S
    assert sorted(rs.tors) == list(range(8))
    for res, idx in rs.tors.items():
        assert len(idx) == 16 and all(rs.records[i].k % 8 == res and rs.route_of(i).kind == "half" for i in idx)
        assert sorted(rs.records[i].tors for i in idx) == sorted(list(range(8)) * 2)
    assert len(rs.records) <= 650


def test_state_words_reduce_to_k(rs):
    seen = set()
    for j, rec in enumerate(rs.records):
        x = pc.state_value(rec.state)
        assert x % L == rec.k and x < 2**512
        seen.add(0 if x == rec.k else 1 if x == rec.k + L else 2)
        assert x in (rec.k, rec.k + L) or x + L >= 2**512
    assert seen == {0, 1, 2}
    arena, offs = rs.arena()
    assert all(o[0] % 8 == 0 for o in offs)
    j = len(rs.records) // 2
    assert bytes(arena[offs[j][0]:offs[j][0] + 64]) == rs.records[j].state
    assert bytes(arena[offs[j][1]:offs[j][1] + 64]) == rs.records[j].sig
    assert bytes(arena[offs[j][2]:offs[j][2] + 32]) == rs.records[j].pub


def test_verdicts_are_reproducible(rs):
    """Each record's code again from its encodings alone, by pyref_ed25519's decode and point arithmetic with no
    remembered product; and what each variant must give."""
    tors = grp.torsion_points()
    for i, rec in enumerate(rs.records):
        A, R = ref.decode(rec.pub), ref.decode(rec.sig[:32])
        S = int.from_bytes(rec.sig[32:], "little")
        assert A is not None and R is not None and S < L
        assert ref._eq(A, rec.A) and ref._eq(R, rec.R)
        if i % 7 == 0 or rec.kind.startswith("tors"):
            negA = grp.neg(A)
            if ref._small_order(A):
                code = ref.ERR_PUBKEY
            elif ref._small_order(R):
                code = ref.ERR_SIG
            else:
                code = 0 if ref._eq(ref._add(ref._mul(S, ref.B), ref._mul(rec.k, negA)), R) else ref.ERR_MSG
            assert code == rec.code, (i, rec.kind)
        if rec.kind == "valid":
            assert rec.code == 0
        elif rec.kind == "bad":
            assert rec.code == ref.ERR_MSG
        elif rec.kind == "szero":
            assert rec.code == (ref.ERR_SIG if rec.k == 0 else 0)       # k = 0: R = O, small order
        else:
            # A + T: [k]T = O decides; no a B + T is of small order
            assert not ref._small_order(A)
            good = ref._eq(ref._mul(rec.k % 8, tors[rec.tors]), grp.O)
            assert rec.code == (0 if good and rec.kind == "tors" else ref.ERR_MSG)
    # every residue sees both verdicts among the valid-S torsion records, except k = 0 (mod 8): all accepted
    for res, idx in rs.tors.items():
        codes = {int(rs.records[i].code) for i in idx if rs.records[i].kind == "tors"}
        assert codes == ({0} if res == 0 else {0, ref.ERR_MSG}), (res, codes)
