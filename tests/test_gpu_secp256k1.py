"""The secp256k1 precompile path on the GPU against the Python model
(tests/pyref_secp256k1.py), every comparison exact: the field, scalar and
group operations, the recover at chosen inputs, the Keccak, the ingest's walk,
whole batches through the ring, the block callers, and the Ed25519 batch's
unchanged behaviour on a block that mixes both programs."""
import numpy as np
import pytest

import pyref_precompile as pp
import pyref_secp256k1 as k1
from firedancer_amd import tile, workload
from firedancer_amd import ed25519 as ed

pytestmark = pytest.mark.gpu

NONE = k1.NONE
P, N, G = k1.P, k1.N, k1.G
M256 = (1 << 256) - 1


def info_tuple(r):
    return (int(r["instr_idx"]), int(r["rec_idx"]), int(r["ed_instr_cnt"]), int(r["sig_cnt"]), int(r["ed_code"]))


def place(payloads, gaps=None, caps=None, tail=0, bound=k1.sig_bound):
    """payloads into one arena, payload i after gaps[i] bytes of filler ->
    (arena, PRECOMPILE_DTYPE records with sig_cap the size bound, or caps)"""
    gaps = gaps or [0] * len(payloads)
    buf, recs = bytearray(), np.zeros(len(payloads), dtype=ed.PRECOMPILE_DTYPE)
    for i, (p, g) in enumerate(zip(payloads, gaps)):
        buf += b"\xa5" * g
        recs[i] = (len(buf), len(p), bound(len(p)) if caps is None else caps[i])
        buf += p
    buf += b"\x5a" * tail
    return np.frombuffer(bytes(buf), dtype=np.uint8), recs


@pytest.fixture(scope="module")
def cases():
    return k1.cases()


@pytest.fixture(scope="module")
def want(cases):
    return k1.expected(cases)


def check(got, want_codes, want_infos):
    codes, info = got
    assert codes.tolist() == [int(c) for c in want_codes]
    assert [info_tuple(r) for r in info] == list(want_infos)
    assert not np.asarray(info["_pad"]).any()


# 1 ------------------------------------------------- field and scalar operations

def test_field_and_scalar_operations(engine):
    """mul, sqr, inversion and square root mod p; mul, inversion and reduction
    mod n: the edges of each modulus, operands above it where the operation
    takes them, products that need the reduction's later folds, and 200
    seeded random operands."""
    rng = k1.Rng("ops")
    rnd = [int.from_bytes(rng.bytes(32), "big") for _ in range(200)]
    c_p = (1 << 32) + 977
    edge = [0, 1, 2, P - 1, P - 2, N - 1, N, N + 1, P, P + 1, M256, M256 - 1, c_p, c_p - 1, c_p + 1, 1 << 255, (1 << 256) - c_p - 1,
            1 << 128, (1 << 128) - 1, M256 ^ ((1 << 64) - 1), (1 << 224) + 1, M256 // 3, (P + 1) // 2, (N + 1) // 2, 7, P - 7]
    items, exp = [], []
    pairs = [(a, b) for a in edge for b in edge[:14]] + list(zip(rnd, rnd[1:] + rnd[:1]))
    for a, b in pairs:
        items.append((0, a, b)); exp.append((0, a * b % P, 0))
        items.append((4, a, b)); exp.append((0, a * b % N, 0))
    for a in edge + rnd:
        items.append((1, a)); exp.append((0, a * a % P, 0))
        items.append((6, a)); exp.append((0, a % N, 0))
    for a in edge + rnd[:60]:
        items.append((2, a)); exp.append((0, pow(a % P, P - 2, P), 0))
        r = pow(a % P, (P + 1) // 4, P)
        items.append((3, a)); exp.append((1 if r * r % P == a % P else 0, r, 0))
        if a < N:
            items.append((5, a)); exp.append((0, pow(a, N - 2, N), 0))
    # squares and non-squares both occur, and the inverses are inverses
    assert {e[0] for it, e in zip(items, exp) if it[0] == 3} == {0, 1}
    got = engine.debug_secp256k1_ops(items)
    bad = [(it[0], hex(it[1])) for it, g, e in zip(items, got, exp) if g != e]
    assert not bad, bad[:5]
    assert len(items) > 1000


# 2 ------------------------------------------------------------ group operations

def _aff(pt):
    return (1, 0, 0) if pt is k1.INF else (0, pt[0], pt[1])


def test_group_operations(engine):
    """P + Q, P + P through the addition, P + (-P), infinity on either side,
    and the doubling, each under several Jacobian scalings of its operands."""
    rng = k1.Rng("group")
    pts = [G, k1.mul(2, G), k1.mul(3, G), k1.mul(N - 1, G), k1.mul(N - 2, G)]
    pts += [k1.mul(int.from_bytes(rng.bytes(32), "big"), G) for _ in range(6)]
    x = 1
    while k1.lift_x(x, 0) is None:
        x += 1
    pts += [k1.lift_x(x, 0), k1.lift_x(x, 1)]                  # y chosen by the model, either parity
    zs = [1, 2, P - 1, int.from_bytes(rng.bytes(32), "big") % P, (1 << 32) + 977]
    items, exp = [], []
    for i, a in enumerate(pts):
        for j, b in enumerate(pts):
            z1, z2 = zs[(i + j) % len(zs)], zs[(2 * i + j + 1) % len(zs)]
            items.append((7, a[0], a[1], z1, b[0], b[1], z2)); exp.append(_aff(k1.add(a, b)))
        for z in zs:
            items.append((7, a[0], a[1], z, a[0], a[1], zs[0])); exp.append(_aff(k1.add(a, a)))            # equal points
            items.append((7, a[0], a[1], z, a[0], P - a[1], z)); exp.append((1, 0, 0))                      # opposite points
            items.append((7, a[0], a[1], 0, a[0], a[1], z)); exp.append(_aff(a))                            # infinity + P
            items.append((7, a[0], a[1], z, a[0], a[1], 0)); exp.append(_aff(a))                            # P + infinity
            items.append((8, a[0], a[1], z)); exp.append(_aff(k1.add(a, a)))
    items.append((7, G[0], G[1], 0, G[0], G[1], 0)); exp.append((1, 0, 0))
    items.append((8, G[0], G[1], 0)); exp.append((1, 0, 0))
    got = engine.debug_secp256k1_ops(items)
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, (bad[:5], [items[i][0] for i in bad[:5]])
    assert sum(e[0] for e in exp) > 50


# 3 ------------------------------------------------------ recover at chosen inputs

def test_recover_at_chosen_inputs(engine):
    edges = k1.recover_edges()
    rng = k1.Rng("gpu-recover")
    extra = [(f"random_{i}", rng.bytes(32), bytes(1) + rng.bytes(31) + bytes(1) + rng.bytes(31), rng.below(4)) for i in range(24)]
    allc = edges + extra
    codes, keys = engine.debug_secp256k1_recover([(h, s, r) for _, h, s, r in allc])
    seen = set()
    for (name, h, s, r), c, key in zip(allc, codes, keys):
        exp = k1.recover(h, s, r)
        assert (int(c), bytes(key)) == exp, name
        seen.add(exp[0])
    assert seen == {0, -1, -2, -3, -4}
    # one record alone in its wave, and 65 copies across a wave boundary
    name, h, s, r = edges[0]
    codes, keys = engine.debug_secp256k1_recover([(h, s, r)] * 65)
    assert codes.tolist() == [0] * 65 and all(bytes(k) == k1.recover(h, s, r)[1] for k in keys)


# 4 ---------------------------------------------------------------------- Keccak

def test_keccak_lengths_mixed_in_a_wave(engine):
    data = k1.Rng("gpu-keccak").bytes(1400)
    lens = [0, 1, 135, 136, 137, 271, 272, 998, 1062, 1232, 2, 134, 138, 270, 273, 407, 408, 409, 543, 544, 680, 816, 952, 1088,
            1087, 1223, 1224, 1225]
    msgs = [data[(7 * i) % 23:(7 * i) % 23 + n] for i, n in enumerate(lens * 3)]       # 84 messages: two waves
    got = engine.debug_keccak256(msgs)
    for m, g in zip(msgs, got):
        assert bytes(g) == k1.keccak256(m), len(m)
    # one ten-block lane among empty messages, at either end of the wave and in its middle
    for at in (0, 31, 63):
        msgs = [b""] * 64
        msgs[at] = data[:1232]
        got = engine.debug_keccak256(msgs)
        assert [bytes(g) for g in got] == [k1.keccak256(m) for m in msgs]


# 5 ------------------------------------------------------------------------ walk

def _check_walk(cases, recs, walk, descs, pos, flags=0):
    used = np.zeros(len(descs), dtype=bool)
    for c, r, w in zip(cases, recs, walk):
        got = (int(w["code"]), int(w["sig_cnt"]), int(w["instr_idx"]), int(w["rec_idx"]), int(w["ed_instr_cnt"]))
        if c.model is None:
            assert got == (k1.CODE_PARSE_FAIL, 0, NONE, NONE, 0), c.name
            continue
        code, fi, fr, cnt, rr = k1.walk(*c.model, flags=flags)
        if len(rr) > int(r["sig_cap"]):
            assert got == (k1.CODE_CAP, 0, NONE, NONE, 0), c.name
            continue
        assert got == (code, len(rr), fi, fr, cnt), c.name
        s0, off = int(w["sig0"]), int(r["off"])
        assert s0 + len(rr) <= len(descs)
        for k, (j, i, s, a, m, ms) in enumerate(rr):
            d = descs[s0 + k]
            assert (int(d["msg_off"]), int(d["msg_sz"]), int(d["sig_off"]), int(d["pub_off"])) == (off + m, ms, off + s, off + a), c.name
            assert int(pos[s0 + k]) == (j << 16) | i, c.name
            assert not used[s0 + k]
            used[s0 + k] = True
    assert used.all()                         # the slots taken are exactly the records, each once


def test_walk_matches_python(engine, cases):
    for flags in (0, k1.FAIL_ON_BAD_COUNT):
        arena, recs = place([c.payload for c in cases], gaps=[(7 * i) % 16 for i in range(len(cases))])
        walk, descs, pos = engine.debug_secp256k1_walk(arena, recs, flags)
        _check_walk(cases, recs, walk, descs, pos, flags)


def test_walk_caps_and_wave_boundaries(engine, cases):
    """sig_cap exact, one short (CAP) and 0; batches of 1, 63, 64 and 65
    transactions (n - 1 is the lane the inactive lanes clamp to)."""
    exact = [len(k1.walk(*c.model)[4]) if c.model is not None else 0 for c in cases]
    for caps in (exact, [max(e - 1, 0) for e in exact], [0] * len(cases)):
        arena, recs = place([c.payload for c in cases], caps=caps)
        walk, descs, pos = engine.debug_secp256k1_walk(arena, recs)
        _check_walk(cases, recs, walk, descs, pos)
        assert len(descs) == sum(e for e, c in zip(exact, caps) if e <= c)
    assert any(e > 1 for e in exact)
    for n in (1, 63, 64, 65):
        sub = [cases[(3 * i) % len(cases)] for i in range(n)]
        arena, recs = place([c.payload for c in sub], gaps=[i % 5 for i in range(n)])
        walk, descs, pos = engine.debug_secp256k1_walk(arena, recs)
        _check_walk(sub, recs, walk, descs, pos)


# 6 --------------------------------------------------------------- whole batches

def test_batches_match_python(engine, cases, want):
    codes, infos, _ = want
    arena, recs = place([c.payload for c in cases], gaps=[(5 * i) % 16 for i in range(len(cases))])
    check(engine.verify_secp256k1(arena, recs), codes, infos)
    fc, fi, _ = k1.expected(cases, k1.FAIL_ON_BAD_COUNT)
    assert fc.tolist() != codes.tolist()
    check(engine.verify_secp256k1(arena, recs, k1.FAIL_ON_BAD_COUNT), fc, fi)
    by = {c.name: i for i, c in enumerate(cases)}
    for name in ("cnt0_sz12", "cnt0_sz40"):
        assert (int(codes[by[name]]), int(fc[by[name]])) == (0, k1.CODE_DATA_SIZE)
    for name, exp in (("order_recfail_then_badidx", (k1.CODE_SIGNATURE, -5)), ("order_badidx_then_recfail", (k1.CODE_DATA_OFFSET, 0))):
        assert (int(codes[by[name]]), infos[by[name]][4]) == exp
    # every record code occurs
    assert {i[4] for i in infos} >= {0, -1, -2, -3, -4, -5}


def test_empty_capped_and_foreign_batches(engine, cases, want):
    codes, infos, _ = want
    got = engine.verify_secp256k1(np.zeros(1, np.uint8)[:0], np.zeros(0, dtype=ed.PRECOMPILE_DTYPE))
    assert len(got[0]) == 0 and len(got[1]) == 0
    # no secp256k1 instruction at all: the Ed25519 case set
    ed_cases = [c for c in pp.cpu_cases(workload.sign) if c.model is not None and not any(
        c.model[0][p] == k1.SECP256K1_ID for p, _, _ in c.model[1])][:40]
    arena, recs = place([c.payload for c in ed_cases])
    c2, i2 = engine.verify_secp256k1(arena, recs)
    assert c2.tolist() == [0] * len(ed_cases) and all(info_tuple(r) == (NONE, NONE, 0, 0, 0) for r in i2)
    # one slot short: CAP, nothing run, no position
    exact = [len(k1.walk(*c.model)[4]) if c.model is not None else 0 for c in cases]
    arena, recs = place([c.payload for c in cases], caps=[max(e - 1, 0) for e in exact])
    c3, i3 = engine.verify_secp256k1(arena, recs)
    for c, e, g, r, wc, wi in zip(cases, exact, c3, i3, codes, infos):
        if e:
            assert (int(g), info_tuple(r)) == (k1.CODE_CAP, (NONE, NONE, 0, 0, 0)), c.name
        else:
            assert (int(g), info_tuple(r)) == (int(wc), wi), c.name
    with pytest.raises(RuntimeError):
        engine.submit_secp256k1(arena, recs, 2)                 # an unknown flag
    bad = recs.copy()
    bad["off"][3] = len(arena)
    with pytest.raises(RuntimeError):
        engine.submit_secp256k1(arena, bad)


def test_two_slots_in_flight(engine, cases, want):
    codes, infos, _ = want
    half = len(cases) // 2
    a1, r1 = place([c.payload for c in cases[:half]])
    a2, r2 = place([c.payload for c in cases[half:]], gaps=[3] * (len(cases) - half))
    t1 = engine.submit_secp256k1(a1, r1)
    t2 = engine.submit_secp256k1(a2, r2)
    check(engine.poll_secp256k1(t2), codes[half:], infos[half:])
    check(engine.poll_secp256k1(t1), codes[:half], infos[:half])
    # a slot that carried this kind carries an Ed25519 batch next, and the reverse
    e_cases = pp.cpu_cases(workload.sign)[:30]
    ea, er = place([c.payload for c in e_cases], bound=pp.sig_bound)
    engine.verify_precompiles(ea, er)
    check(engine.verify_secp256k1(a1, r1), codes[:half], infos[:half])


def test_block_callers_on_a_mixed_block(engine, oracle):
    """fdgpu_block_secp256k1_verify and fdgpu_block_precompile_verify_all over
    a block mixing both programs, small batches so that several are in
    flight; and fdgpu_submit_precompiles over the same block still returns
    what the Ed25519 reference gives: it skips the secp256k1 instructions."""
    block = k1.mixed_block(workload.sign) + k1.cases()[:30]
    payloads = [c.payload for c in block]
    e_codes, e_infos, _ = pp.expected(block, oracle.verify)
    k_codes, k_infos, _ = k1.expected(block)
    none = (NONE, NONE, 0, 0, 0)
    got, gi = tile.block_secp256k1_verify(engine, payloads, batch_txn_max=7)
    for c, g, r, kc, ki in zip(block, got, gi, k_codes, k_infos):
        assert (int(g), info_tuple(r)) == (int(kc), ki if ki[2] else none), c.name
    got, gi = tile.block_precompile_verify_all(engine, payloads, batch_txn_max=7)
    which = set()
    for c, g, r, ec, ei, kc, ki in zip(block, got, gi, e_codes, e_infos, k_codes, k_infos):
        exp = k1.merge((int(ec), ei if ei[2] else none), (int(kc), ki if ki[2] else none))
        assert (int(g), info_tuple(r) + (int(r["_pad"][0]),)) == exp, c.name
        which.add((c.name, exp[1][5]))
    assert ("ed_fails_first", 1) in which and ("k1_fails_first", 2) in which
    # the old behaviour
    arena, recs = place(payloads, bound=pp.sig_bound)
    c0, i0 = engine.verify_precompiles(arena, recs)
    assert c0.tolist() == e_codes.tolist()
    assert [info_tuple(r) for r in i0] == e_infos
