"""The Ed25519 precompile path on the GPU against the Python reference
(tests/pyref_precompile.py, verdicts by the oracle): the ingest's walk, the
ring batch with every engine path, batch sizes around the wave, message
lengths at every arena alignment, the end of the arena, the ring's semantics
and the block caller."""
import numpy as np
import pytest

import pyref_precompile as pp
from firedancer_amd import VerifyEngine, tile, workload
from firedancer_amd import ed25519 as ed

pytestmark = pytest.mark.gpu

NONE = pp.NONE


def info_tuple(r):
    return (int(r["instr_idx"]), int(r["rec_idx"]), int(r["ed_instr_cnt"]), int(r["sig_cnt"]), int(r["ed_code"]))


def place(payloads, gaps=None, caps=None, tail=0):
    """payloads into one arena, payload i after gaps[i] bytes of filler ->
    (arena, PRECOMPILE_DTYPE records with sig_cap the size bound, or caps)"""
    gaps = gaps or [0] * len(payloads)
    buf, recs = bytearray(), np.zeros(len(payloads), dtype=ed.PRECOMPILE_DTYPE)
    for i, (p, g) in enumerate(zip(payloads, gaps)):
        buf += b"\xa5" * g
        recs[i] = (len(buf), len(p), pp.sig_bound(len(p)) if caps is None else caps[i])
        buf += p
    buf += b"\x5a" * tail
    return np.frombuffer(bytes(buf), dtype=np.uint8), recs


@pytest.fixture(scope="module")
def cases():
    return pp.cpu_cases(workload.sign)


@pytest.fixture(scope="module")
def want(cases, oracle):
    return pp.expected(cases, oracle.verify)


def check(got, want_codes, want_infos):
    codes, info = got
    assert codes.tolist() == [int(c) for c in want_codes]
    assert [info_tuple(r) for r in info] == list(want_infos)
    assert not np.asarray(info["_pad"]).any()


def test_walk_matches_python(engine, cases):
    """debug_precompile_walk on the whole CPU case set as one batch: codes,
    positions, counts, and each transaction's descriptors in order."""
    arena, recs = place([c.payload for c in cases], gaps=[(7 * i) % 16 for i in range(len(cases))])
    walk, descs, pos = engine.debug_precompile_walk(arena, recs)
    used = np.zeros(len(descs), dtype=bool)
    for c, r, w in zip(cases, recs, walk):
        if c.model is None:
            assert (int(w["code"]), int(w["sig_cnt"]), int(w["instr_idx"]), int(w["rec_idx"]), int(w["ed_instr_cnt"])) == \
                (pp.CODE_PARSE_FAIL, 0, NONE, NONE, 0), c.name
            continue
        code, fi, fr, ed_cnt, rr = pp.walk(*c.model)
        assert (int(w["code"]), int(w["sig_cnt"]), int(w["instr_idx"]), int(w["rec_idx"]), int(w["ed_instr_cnt"])) == \
            (code, len(rr), fi, fr, ed_cnt), c.name
        s0, off = int(w["sig0"]), int(r["off"])
        assert s0 + len(rr) <= len(descs)
        for k, (j, i, s, p, m, ms) in enumerate(rr):
            d = descs[s0 + k]
            assert (int(d["msg_off"]), int(d["msg_sz"]), int(d["sig_off"]), int(d["pub_off"])) == (off + m, ms, off + s, off + p), c.name
            assert int(pos[s0 + k]) == (j << 16) | i, c.name
            assert not used[s0 + k]
            used[s0 + k] = True
    assert used.all()                         # the slots taken are exactly the records, each once


@pytest.mark.parametrize("flags", [{}, {"key_cache": True}, {"full_path": True}, {"pair": True}])
def test_verify_matches_python(engine, cases, want, flags):
    codes, infos, _ = want
    arena, recs = place([c.payload for c in cases], gaps=[(5 * i) % 16 for i in range(len(cases))])
    if not flags:
        check(engine.verify_precompiles(arena, recs), codes, infos)
        return
    e = VerifyEngine(0, max_txn=256, max_sig=8192, max_arena=1 << 18, **flags)
    try:
        check(e.verify_precompiles(arena, recs), codes, infos)
    finally:
        e.close()


@pytest.fixture(scope="module")
def pool(oracle):
    """Transactions of 0, 1, 2, 17, 64 and 75 records, some with a failing
    record, and their verdicts: the batches below draw from it."""
    g = pp.Gen(workload.sign, "pool")
    txs = []
    for n in (0, 1, 2, 17, 64):
        txs.append(pp.random_txn(g, n))
        if n:
            txs.append(pp.random_txn(g, n, bad_at=n - 1))
    txs.append(pp.max_records(g, pp.MTU))                       # 75 records, the first of which fails
    codes, infos, recs = pp.expected(txs, oracle.verify)
    assert sorted(set(len(r) for r in recs)) == [0, 1, 2, 17, 64, 75]
    return txs, codes, infos, [len(r) for r in recs]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_batch_sizes(engine, pool, n):
    """A wave's claim exceeds 64 and 256 signatures, several waves contend for
    the counter; sig_cap is the exact count."""
    txs, codes, infos, cnts = pool
    rng = pp.Rng("batch %d" % n)
    pick = [rng.below(len(txs)) for _ in range(n)]
    if n >= 64:
        pick[:4] = [len(txs) - 1, len(txs) - 2, len(txs) - 3, 0]      # 75 + 64 + 64 in one wave, beside a 0
    arena, recs = place([txs[k].payload for k in pick], caps=[cnts[k] for k in pick])
    check(engine.verify_precompiles(arena, recs), [codes[k] for k in pick], [infos[k] for k in pick])


@pytest.fixture(scope="module")
def small():
    """One small engine for the tests of the limits: 64 transactions, 300
    signature slots, a 128 KiB arena, two ring slots."""
    e = VerifyEngine(0, max_txn=64, max_sig=300, max_arena=1 << 17, ring_depth=2)
    yield e
    e.close()


def test_caps_and_limits(small, pool, cases, want):
    txs, codes, infos, cnts = pool
    e = small
    big = [k for k, c in enumerate(cnts) if c >= 64]
    pick = big[:3]
    assert len(pick) == 3
    total = sum(cnts[k] for k in pick)
    one = next(k for k, c in enumerate(cnts) if c == 1)
    while total + 17 <= 300:
        k17 = next(k for k, c in enumerate(cnts) if c == 17)
        pick.append(k17)
        total += 17
    pick += [one] * (300 - total)
    arena, recs = place([txs[k].payload for k in pick], caps=[cnts[k] for k in pick])
    assert int(recs["sig_cap"].sum()) == 300                 # exactly max_sig: accepted
    check(e.verify_precompiles(arena, recs), [codes[k] for k in pick], [infos[k] for k in pick])
    recs2 = recs.copy()
    recs2["sig_cap"][0] += 1                                 # one above: FDGPU_ERR_INVAL
    with pytest.raises(RuntimeError, match=r"\(-10\)"):
        e.submit_precompiles(arena, recs2)
    # one short of what resolves: CAP, nothing run; the neighbours keep their verdicts
    recs3 = recs.copy()
    recs3["sig_cap"][0] -= 1
    recs3["sig_cap"][2] = 0
    c3, i3 = e.verify_precompiles(arena, recs3)
    for k in (0, 2):
        assert c3[k] == pp.CODE_CAP and info_tuple(i3[k]) == (NONE, NONE, 0, 0, 0)
    keep = [k for k in range(len(pick)) if k not in (0, 2)]
    assert c3[keep].tolist() == [int(codes[pick[k]]) for k in keep]
    assert [info_tuple(i3[k]) for k in keep] == [infos[pick[k]] for k in keep]
    # all CAP, all PARSE_FAIL, empty
    capped = [k for k in pick[:40] if cnts[k]]
    a4, r4 = place([txs[k].payload for k in capped], caps=[0] * len(capped))
    c4, i4 = e.verify_precompiles(a4, r4)
    assert (c4 == pp.CODE_CAP).all() and all(info_tuple(r) == (NONE, NONE, 0, 0, 0) for r in i4)
    bad = [c.payload for c in cases if c.model is None] * 5
    c5, i5 = e.verify_precompiles(*place(bad))
    assert (c5 == pp.CODE_PARSE_FAIL).all() and all(info_tuple(r) == (NONE, NONE, 0, 0, 0) for r in i5)
    c6, i6 = e.verify_precompiles(np.zeros(0, np.uint8), np.zeros(0, ed.PRECOMPILE_DTYPE))
    assert len(c6) == 0 and len(i6) == 0
    # at the size bound: every transaction's cap the bound of its size
    a7, r7 = place([txs[k].payload for k in (len(txs) - 1, 0, 1)])
    assert r7["sig_cap"].tolist()[0] == 75
    check(e.verify_precompiles(a7, r7), [codes[k] for k in (len(txs) - 1, 0, 1)], [infos[k] for k in (len(txs) - 1, 0, 1)])


def longest(g, bad):
    """The longest message a transaction can carry, 998 bytes: a 1,232-byte
    transaction of two accounts whose one instruction's data is the table, the
    key, filler and then the signature over everything before it."""
    prv = g.rng.bytes(32)
    pub = workload.sign(prv, b"")[0]
    n = 1062 - 64
    body = pp.table([pp.record(n, 0xFFFF, 16, 0xFFFF, 0, n, 0xFFFF)]) + pub + g.rng.bytes(n - 48)
    sig = workload.sign(prv, body)[1]
    if bad:
        sig = bytes([sig[0] ^ 4]) + sig[1:]
    c = g.case("longest_bad" if bad else "longest", [(1, b"", body + sig)], accts=[g.payer, pp.ED25519_ID])
    assert len(c.payload) == pp.MTU
    return c


@pytest.fixture(scope="module")
def by_len(oracle):
    g = pp.Gen(workload.sign, "lens")
    txs = []
    for ln in (0, 1, 111, 112, 127, 128, 129):
        txs.append(g.case("len%d" % ln, [(pp.ED, b"", g.self_ix([ln]))]))
        txs.append(g.case("len%d_bad" % ln, [(pp.ED, b"", g.self_ix([ln], ["R"]))]))
    txs += [longest(g, False), longest(g, True)]
    codes, infos, _ = pp.expected(txs, oracle.verify)
    assert codes.tolist() == [0, pp.CODE_SIGNATURE] * 8
    return txs, codes, infos


def test_message_lengths_at_every_alignment(engine, by_len):
    """Messages of 0 .. 998 bytes (SHA-512 block boundaries at 111/112 and
    127/128/129 behind R and A) in one batch, each transaction at every arena
    offset mod 16."""
    txs, codes, infos = by_len
    payloads, gaps, wc, wi = [], [], [], []
    at = 0
    for a in range(16):
        for k, t in enumerate(txs):
            g = (a - at) % 16
            payloads.append(t.payload); gaps.append(g); wc.append(codes[k]); wi.append(infos[k])
            at += g + len(t.payload)
    arena, recs = place(payloads, gaps=gaps)
    assert sorted(set((recs["off"] % 16).tolist())) == list(range(16))
    check(engine.verify_precompiles(arena, recs), wc, wi)


def test_transaction_that_ends_with_the_arena(engine, by_len, cases, want):
    """The last transaction's last byte is the arena's last byte, staged and
    registered; a larger batch through the same ring slots first leaves stale
    bytes where the slack will lie."""
    txs, codes, infos = by_len
    order = [3, 14, 0, 15]                     # ends with the 998-byte message whose signature fails
    arena, recs = place([txs[k].payload for k in order], gaps=[3, 5, 9, 1])
    assert int(recs[-1]["off"]) + int(recs[-1]["sz"]) == len(arena)
    wc, wi = [codes[k] for k in order], [infos[k] for k in order]
    big_arena, big_recs = place([c.payload for c in cases], tail=4096)
    assert len(big_arena) > len(arena) + 4096 and big_arena[len(arena):len(arena) + 4096].any()
    check(engine.verify_precompiles(arena, recs), wc, wi)                        # staged
    reg = np.zeros(len(arena) + 8192, dtype=np.uint8)
    base = (-reg.ctypes.data) % 4096
    pinned = reg[base:base + len(arena)]
    pinned[:] = arena
    engine.host_register(pinned)
    try:
        for _ in range(2):                                                       # both ring slots
            check(engine.verify_precompiles(big_arena, big_recs), want[0], want[1])
        check(engine.verify_precompiles(pinned, recs), wc, wi)                   # uploaded in place
        check(engine.verify_precompiles(big_arena, big_recs), want[0], want[1])
        check(engine.verify_precompiles(arena, recs), wc, wi)
    finally:
        engine.host_unregister(pinned)


def test_ring_semantics(small, pool, cases, want):
    txs, codes, infos, cnts = pool
    e = small
    sub = slice(0, 60)                                                       # within the small engine's limits
    a1, r1 = place([c.payload for c in cases[sub]], caps=[len(r) for r in want[2][sub]])
    w1 = (want[0][sub], want[1][sub])
    assert int(r1["sig_cap"].sum()) + sum(cnts) <= 300 and len(a1) <= 1 << 17
    a2, r2 = place([t.payload for t in txs], caps=cnts)
    t1 = e.submit_precompiles(a1, r1)
    t2 = e.submit_precompiles(a2, r2)
    with pytest.raises(RuntimeError, match=r"\(-12\)"):                      # FDGPU_ERR_FULL at ring depth
        e.submit_precompiles(a2, r2)
    check(e.poll_precompiles(t2), codes, infos)                              # out of order
    check(e.poll_precompiles(t1), *w1)
    L = ed._lib.lib()

    def rc(arena, recs, n=None, arena_sz=None):
        return L.fdgpu_submit_precompiles(e._h, arena.ctypes.data if arena is not None else None,
                                          len(arena) if arena_sz is None else arena_sz,
                                          recs.ctypes.data if recs is not None else None, len(recs) if n is None else n)
    INVAL = -10
    assert rc(None, r2, arena_sz=len(a2)) == INVAL                           # null arena
    assert rc(a2, None, n=3) == INVAL                                        # null records
    assert L.fdgpu_submit_precompiles(None, a2.ctypes.data, len(a2), r2.ctypes.data, len(r2)) == INVAL
    many = np.zeros(65, dtype=ed.PRECOMPILE_DTYPE)
    assert rc(a2, many) == INVAL                                             # n > max_txn
    over = r2.copy(); over["sig_cap"][0] = 301
    assert rc(a2, over) == INVAL                                             # sum(sig_cap) > max_sig
    out = r2.copy(); out["off"][3] = len(a2) - int(out["sz"][3]) + 1
    assert rc(a2, out) == INVAL                                              # outside the arena
    fat = np.zeros(1, dtype=ed.PRECOMPILE_DTYPE); fat[0] = (0, 1233, 0)
    assert rc(np.zeros(2000, np.uint8), fat) == INVAL                        # larger than FD_TXN_MTU
    assert rc(np.zeros((1 << 17) + 1, np.uint8), r2[:0]) == INVAL            # arena beyond max_arena
    # the engine still works, and no slot leaked
    check(e.verify_precompiles(a2, r2), codes, infos)
    check(e.verify_precompiles(a1, r1), *w1)
    ing, ver = e.debug_precompile_time(a2, r2, iters=2)
    assert ing > 0 and ver > 0


def test_block_precompile_verify(engine, oracle, pool, cases):
    """A synthetic block of 2,000 transactions, one in eight with Ed25519
    instructions, some corrupted: the engine path equals its own e = NULL run
    and the Python reference."""
    txs, _, _, _ = pool
    g = pp.Gen(workload.sign, "block")
    with_ed = [c for c in cases if c.model is not None] + txs
    rng = pp.Rng("block pick")
    block = []
    for i in range(2000):
        if i % 8 == 3:
            block.append(with_ed[rng.below(len(with_ed))])
        elif i % 97 == 5:
            block.append(pp.Case("junk", rng.bytes(50 + rng.below(300)), None))
        else:
            block.append(pp.random_txn(g, 0))
    codes, infos, recs = pp.expected(block, oracle.verify)
    payloads = [c.payload for c in block]

    def fn(a, t):
        return [oracle.verify(bytes(a[int(x["msg_off"]):int(x["msg_off"]) + int(x["msg_sz"])]),
                              bytes(a[int(x["sig_off"]):int(x["sig_off"]) + 64]),
                              bytes(a[int(x["pub_off"]):int(x["pub_off"]) + 32])) for x in t]
    hc, hi = tile.block_precompile_verify(None, payloads, batch_txn_max=512, host_verifier=tile.PyVerifier(fn))
    gc, gi = tile.block_precompile_verify(engine, payloads, batch_txn_max=100)           # several ring batches
    assert gc.tolist() == hc.tolist() == codes.tolist()
    assert [info_tuple(r) for r in gi] == [info_tuple(r) for r in hi]
    assert [info_tuple(r) for r in gi] == [i if i[2] else (NONE, NONE, 0, 0, 0) for i in infos]
    assert (codes != 0).sum() > 50 and pp.CODE_PARSE_FAIL in codes.tolist()
