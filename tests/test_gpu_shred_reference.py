"""The shred path on the GPU against the reference's recorded verdicts
(tests/golden/shred_reference.json, see test_shred_reference.py): the whole
corpus as one batch through the default, the key-cache and the full-path
engine; the prefixed leaf hash and the proof-node loads at every (leaf length,
address mod 16); and shreds that end where the arena ends."""
import numpy as np
import pytest

import pyref_shred as ps
from conftest import load_json
from firedancer_amd import VerifyEngine, workload
from firedancer_amd.ed25519 import CODE_SHRED_REJECT, SHRED_DTYPE

pytestmark = pytest.mark.gpu

VERSION = ps.CORPUS_VERSION
PUB = workload.sign(ps.CORPUS_PRV, b"")[0]


def _roots(shreds):
    """-> (roots uint8[n, 32] by pyref_shred, all zero where the checks drop the shred; passed bool[n])"""
    roots = np.zeros((len(shreds), 32), dtype=np.uint8)
    passed = np.zeros(len(shreds), dtype=bool)
    for i, b in enumerate(shreds):
        r = ps.shred_root(b, VERSION)
        if r is not None:
            roots[i], passed[i] = np.frombuffer(r, dtype=np.uint8), True
    return roots, passed


@pytest.fixture(scope="module")
def judged():
    """-> (cases, arena, records, roots, passed): the corpus as one batch, the key behind the shreds"""
    cases = ps.judged_corpus(load_json("shred_reference.json"), workload.sign)
    arena, recs = ps.pack([c["buf"] for c in cases], [PUB])
    roots, passed = _roots([c["buf"] for c in cases])
    # what pyref_shred decides is what the reference decided (test_shred_reference.py asserts it case by case)
    assert passed.tolist() == [c["want"] != "reject" for c in cases]
    return cases, arena, recs, roots, passed


def _check_codes(cases, codes):
    assert len(codes) == len(cases)
    for i, c in enumerate(cases):
        assert ps.code_as_wanted(int(codes[i]), c["want"]), (i, c["family"], int(codes[i]), c["want"])


def test_corpus_matches_the_reference(engine, judged):
    cases, arena, recs, want_roots, passed = judged
    ok, roots = engine.debug_shred_roots(arena, recs, VERSION)
    assert ok.tolist() == np.where(passed, 0, CODE_SHRED_REJECT).tolist()
    assert not roots[~passed].any()
    assert (roots == want_roots).all()          # on the accepted cases the reference has vouched for this root
    codes, roots = engine.verify_shreds(arena, recs, VERSION)
    _check_codes(cases, codes)
    assert ((codes == CODE_SHRED_REJECT) == ~passed).all()
    assert not roots[~passed].any()
    assert (roots == want_roots).all()


def test_corpus_on_the_key_cache_and_full_path_engines(engine, judged):
    cases, arena, recs, want_roots, _ = judged
    codes, roots = engine.verify_shreds(arena, recs, VERSION)
    for kw in ({"key_cache": True}, {"full_path": True}):
        e = VerifyEngine(0, max_txn=1 << 12, max_sig=1 << 12, max_arena=1 << 23, **kw)
        try:
            c2, r2 = e.verify_shreds(arena, recs, VERSION)
        finally:
            e.close()
        _check_codes(cases, c2)
        assert c2.tolist() == codes.tolist(), kw
        assert (r2 == roots).all() and (r2 == want_roots).all(), kw


def _place(shreds, offsets_mod16, key_first=False):
    """Shreds at chosen arena offsets mod 16, explicit padding between them;
    the leader's key in front (then the last shred's last byte is the arena's
    last) or behind.  -> (arena, records)"""
    blob = bytearray(PUB if key_first else b"")
    recs = np.zeros(len(shreds), dtype=SHRED_DTYPE)
    for i, (b, m) in enumerate(zip(shreds, offsets_mod16)):
        blob += b"\xa5" * ((m - len(blob)) % 16)
        recs[i]["off"], recs[i]["sz"] = len(blob), len(b)
        blob += bytes(b)
    if not key_first:
        recs["pub_off"] = len(blob)
        blob += PUB
    return np.frombuffer(bytes(blob), dtype=np.uint8).copy(), recs


# one type per leaf length class: the leaf of a data shred is 1139 - 20 depth bytes (chained or not), 64 less when
# resigned, that of a code shred 1164 - 20 depth, 64 less when resigned -- 40 distinct lengths over depth 0..9
CLASSES = (ps.T_DATA_CH, ps.T_DATA_RS, ps.T_CODE, ps.T_CODE_RS)


def _class_shred(t, depth, rng):
    """A sealed shred of the class with the largest leaf index the depth admits (so the walk takes both sides).  A
    code shred's index is at least 1 (data_cnt 1, code.idx 0): at depth 0 the depth rule drops every code shred, so
    nothing ever hashes that leaf length -- the checks' verdict is what is compared there."""
    idx = min((1 << depth) - 1, 66) if ps.is_data(t) else max(1, min((1 << depth) - 1, 133))
    dc = min(67, idx)
    b = ps.blank_shred(t, depth, rng, VERSION, idx, data_cnt=dc, code_cnt=67)
    ps.seal(b, ps.CORPUS_PRV, VERSION, workload.sign)
    return b


def test_prefixed_hash_and_node_loads_at_every_alignment(engine):
    rng = ps.CounterRng("alignment sweep")
    shreds, mods = [], []
    for t in CLASSES:
        for depth in range(10):
            for m in range(16):
                shreds.append(_class_shred(t, depth, rng))
                mods.append(m)
    arena, recs = _place(shreds, mods)
    want_roots, passed = _roots(shreds)
    pairs = {(ps.proof_off(b[0x40] & 0xF0, b[0x40] & 0xF) - 64, int(r["off"]) % 16) for b, r in zip(shreds, recs)}
    assert len(pairs) == 640 and len({p[0] for p in pairs}) == 40
    assert passed.sum() == 640 - 2 * 16                  # all but the two code classes at depth 0
    ok, roots = engine.debug_shred_roots(arena, recs, VERSION)
    assert ok.tolist() == np.where(passed, 0, CODE_SHRED_REJECT).tolist()
    assert (roots == want_roots).all()
    codes, roots = engine.verify_shreds(arena, recs, VERSION)
    assert codes.tolist() == np.where(passed, 0, CODE_SHRED_REJECT).tolist()
    assert (roots == want_roots).all()


def _tail_batch(last, rng):
    """A few shreds behind the key, `last` the final one: (type, depth, flip the last protected byte after sealing)"""
    shreds = [_class_shred(t, d, rng) for t, d in ((ps.T_CODE_CH, 5), (ps.T_DATA, 0), (ps.T_DATA_RS, 9), (ps.T_CODE, 2))]
    t, depth, tampered = last
    b = _class_shred(t, depth, rng)
    if tampered:
        b[(ps.MIN_SZ if ps.is_data(t) else ps.MAX_SZ) - (64 if ps.resigned(t) else 0) - 1] ^= 0x80
    shreds.append(b)
    return shreds


@pytest.mark.parametrize("last", [(ps.T_DATA, 0, False), (ps.T_DATA_CH, 3, False), (ps.T_DATA, 9, True),
                                  (ps.T_CODE, 2, False), (ps.T_CODE_CH, 9, True), (ps.T_DATA_RS, 4, False)],
                         ids=lambda x: "%02x-d%d%s" % (x[0], x[1], "-tampered" if x[2] else ""))
def test_shreds_that_end_with_the_arena(engine, oracle, judged, last):
    """The loads of the last shred's leaf and proof run into the arena's slack (allocated on every path: the ring
    slot's arena, the diagnostics' own buffers) and the roots region behind it; what lies there -- zeros, or the
    bytes of an earlier, larger batch in the same ring slot -- must never reach a digest."""
    rng = ps.CounterRng("end of arena %r" % (last,))
    shreds = _tail_batch(last, rng)
    arena, recs = _place(shreds, [int(rng.integers(0, 16)) for _ in shreds], key_first=True)
    assert int(recs[-1]["off"]) + int(recs[-1]["sz"]) == len(arena) and int(recs["pub_off"][0]) == 0
    want_roots, passed = _roots(shreds)
    assert passed.all()
    want = [oracle.verify(want_roots[i].tobytes(), bytes(b[:64]), PUB) for i, b in enumerate(shreds)]
    assert want[:-1] == [0] * (len(shreds) - 1) and (want[-1] != 0) == last[2]

    def same(got):
        codes, roots = got
        assert codes.tolist() == want
        assert (roots == want_roots).all()

    ok, roots = engine.debug_shred_roots(arena, recs, VERSION)
    assert not ok.any() and (roots == want_roots).all()
    same(engine.verify_shreds(arena, recs, VERSION))                       # staged
    reg = np.zeros(len(arena) + 8192, dtype=np.uint8)
    base = (-reg.ctypes.data) % 4096
    pinned = reg[base:base + len(arena)]
    pinned[:] = arena
    engine.host_register(pinned)
    try:
        same(engine.verify_shreds(pinned, recs, VERSION))                  # uploaded in place
        # a larger batch through the same ring slot leaves its bytes where this arena's slack and roots will lie
        _, big_arena, big_recs, big_roots, _ = judged
        assert len(big_arena) > 4 * len(arena) and big_arena[len(arena):len(arena) + 4096].any()
        assert (engine.verify_shreds(big_arena, big_recs, VERSION)[1] == big_roots).all()
        same(engine.verify_shreds(pinned, recs, VERSION))
        assert (engine.verify_shreds(big_arena, big_recs, VERSION)[1] == big_roots).all()
        same(engine.verify_shreds(arena, recs, VERSION))
    finally:
        engine.host_unregister(pinned)
