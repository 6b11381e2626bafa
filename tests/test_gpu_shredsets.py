"""Set batches on the GPU (fdgpu_submit_shred_sets): codes, roots,
representatives and the lane count against the Python model over the oracle
and against fdgpu_submit_shreds on the same shreds.

Where a test asserts lanes == the number of distinct keys, it does so on a
batch of at most 1,024 shreds whose keys do not collide on purpose: the dedup
table holds at least twice as many slots as shreds (load <= 0.5), and under a
random seed a run of 32 occupied slots in front of a key -- the one way a
shred that has an equal in the table ends up representing itself -- does not
occur at that load.  That is a condition of these assertions, not a property
of the interface, which promises only distinct <= lanes <= n."""
import numpy as np
import pytest

import pyref_shred as ps
import pyref_shredsets as pss
from firedancer_amd import VerifyEngine, workload
from firedancer_amd.ed25519 import SET_SHRED_DTYPE

pytestmark = pytest.mark.gpu

VERSION = 0x1234


@pytest.fixture(scope="module")
def mixed():
    shreds, key_of, keys, _ = pss.mixed(VERSION, np.random.default_rng(31), workload.sign)
    return pss.pack(shreds, keys, key_of)


@pytest.fixture(scope="module")
def known():
    return pss.known_mix(VERSION, np.random.default_rng(32), workload.sign)


@pytest.fixture(scope="module")
def stream():
    shreds, key_of, keys = pss.stream(VERSION, np.random.default_rng(33), workload.sign, 257)
    return pss.pack(shreds, keys, key_of)


def run(eng, oracle, arena, recs, exact=True):
    """the batch on eng held to the model and to fdgpu_submit_shreds -> (codes, roots, rep, lanes, distinct)"""
    want_codes, want_roots, groups = pss.model(arena, recs, VERSION, oracle.verify)
    codes, roots, rep, lanes = eng.verify_shred_sets(arena, recs, VERSION)
    n = len(recs)
    assert len(codes) == n and roots.shape == (n, 32) and len(rep) == n
    assert codes.tolist() == want_codes.tolist()
    assert (roots == want_roots).all()
    distinct = pss.check_reps(rep, lanes, groups, n)
    assert distinct <= lanes <= n
    if exact:
        assert n <= 1024 and lanes == distinct
    nk = recs["known_off"] == pss.NO_ROOT
    c1, r1 = eng.verify_shreds(arena, pss.drop_known(recs[nk]), VERSION)
    assert c1.tolist() == codes[nk].tolist() and (r1 == roots[nk]).all()
    return codes, roots, rep, lanes, distinct


def test_whole_sets_mixed(engine, oracle, mixed):
    arena, recs = mixed
    assert len(recs) == 110
    codes, roots, rep, lanes, distinct = run(engine, oracle, arena, recs)
    assert (codes == 0).all()
    assert lanes == distinct == len(pss.MIXED_SETS)
    assert lanes < len(recs)                     # one verify lane per set, not per shred


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(engine, oracle, stream, n):
    """cut from a stream of 32:32 sets shifted by 32: one set spans the wave
    boundary at 64, one the dedup workgroup's at 256"""
    arena, recs = stream
    codes, roots, rep, lanes, distinct = run(engine, oracle, arena, recs[:n])
    assert (codes == 0).all()
    assert lanes == (0 if n == 0 else 1 + (n + 31) // 64)
    if n > 64:
        assert rep[63] == rep[64]
    if n > 256:
        assert rep[255] == rep[256]


def test_same_signature_different_keys(engine, oracle, mixed):
    arena, recs = mixed
    arena = arena.copy()
    a, b, c = 5, 17, 40
    arena[int(recs["off"][a]) + 200] ^= 0x40                     # its own root under the set's signature
    recs = np.concatenate([recs, recs[c:c + 1]])                 # the same shred twice: one key
    other = sorted(set(recs["pub_off"].tolist()) - {int(recs["pub_off"][b])})[0]
    recs["pub_off"][b] = other                                   # the wrong leader: its own key
    codes, roots, rep, lanes, distinct = run(engine, oracle, arena, recs)
    assert distinct == len(pss.MIXED_SETS) + 2
    assert codes[a] != 0 and codes[b] != 0 and (np.delete(codes, [a, b]) == 0).all()
    assert rep[a] == a and rep[b] == b and rep[len(recs) - 1] == rep[c]


def test_known_roots(engine, oracle, known, mixed):
    arena, recs = known
    codes, roots, rep, lanes, distinct = run(engine, oracle, arena, recs)
    kn = recs["known_off"] != pss.NO_ROOT
    assert (codes[kn] == 0).sum() >= 30 and (codes == pss.CODE_SHRED_ROOT_MISMATCH).sum() >= 8
    assert (codes == pss.CODE_SHRED_REJECT).sum() == 6 and (codes[kn] == pss.CODE_SHRED_REJECT).sum() == 3
    assert roots[codes == pss.CODE_SHRED_ROOT_MISMATCH].any(axis=1).all()     # the derived root, still reported
    assert (rep[kn] == pss.NO_REP).all()
    # the known roots take no lane: the same shreds without them need as many
    bare = recs.copy()
    bare["known_off"] = pss.NO_ROOT
    assert run(engine, oracle, arena, bare)[3] == lanes == len(pss.MIXED_SETS)
    # every shred with a known root, and every shred rejected: no verify lane at all
    allk = recs.copy()
    allk["known_off"] = np.where(kn, recs["known_off"], recs["known_off"][0])
    c2, r2, rep2, lanes2, _ = run(engine, oracle, arena, allk)
    assert lanes2 == 0 and (rep2 == pss.NO_REP).all() and set(c2.tolist()) == {0, pss.CODE_SHRED_ROOT_MISMATCH, pss.CODE_SHRED_REJECT}
    c3, r3, rep3, lanes3, _ = run(engine, oracle, arena, recs[codes == pss.CODE_SHRED_REJECT])
    assert lanes3 == 0 and (c3 == pss.CODE_SHRED_REJECT).all() and not r3.any()


def _same_r(rng):
    """40 shreds with one root and one R, distinct S (the codes need not be 0)"""
    s, _ = ps.fec_set(1, 1, ps.T_DATA, ps.T_CODE, pss.PRVS[0], VERSION, rng, workload.sign)
    out = []
    for k in range(40):
        b = bytearray(s[0])
        b[32:36] = (int.from_bytes(b[32:36], "little") ^ (k + 1)).to_bytes(4, "little")
        out.append(b)
    return out, [workload.sign(pss.PRVS[0], b"")[0]]


def test_probe_bound(engine, oracle):
    """The hash sees only R and the root, so these 40 keys start at one slot
    and fill a run of 32; the other 8 find no room and represent themselves.

    As the issue words it -- 40 copies of the last shred appended -- the lane
    count depends on which lanes win the slots: if a copy of the last key
    claims one, all 41 share it and lanes == distinct.  That batch is held to
    the codes and to distinct <= lanes <= n.  Appending one copy of each of
    the 40 makes the count independent of the order: no key holds two slots
    and none is passed by a lane of its own, so exactly 32 keys sit in the
    table with both their shreds, and both shreds of each of the other 8
    represent themselves: lanes == 32 + 16 > distinct == 40."""
    base, keys = _same_r(np.random.default_rng(34))
    arena, recs = pss.pack(base + [bytearray(base[-1]) for _ in range(40)], keys)
    codes, roots, rep, lanes, distinct = run(engine, oracle, arena, recs, exact=False)
    assert distinct == 40 and len(recs) == 80
    arena, recs = pss.pack(base + [bytearray(b) for b in base], keys)
    codes, roots, rep, lanes, distinct = run(engine, oracle, arena, recs, exact=False)
    assert distinct == 40 and len(recs) == 80
    assert distinct < lanes <= len(recs)         # the overflow path ran
    assert lanes == 48
    assert (codes[:40] == codes[40:]).all()


def test_two_slots_and_key_cache(engine, oracle, known, stream):
    a1, r1 = known
    a2, r2 = stream
    w1 = pss.model(a1, r1, VERSION, oracle.verify)
    w2 = pss.model(a2, r2, VERSION, oracle.verify)
    kc = VerifyEngine(0, max_txn=1 << 10, max_sig=1 << 10, max_arena=1 << 20, key_cache=True)
    try:
        for eng in (engine, kc):
            t1 = eng.submit_shred_sets(a1, r1, VERSION)
            t2 = eng.submit_shred_sets(a2, r2, VERSION)
            c2, o2, p2, l2 = eng.poll_shred_sets(t2)
            c1, o1, p1, l1 = eng.poll_shred_sets(t1)
            assert c1.tolist() == w1[0].tolist() and (o1 == w1[1]).all()
            assert c2.tolist() == w2[0].tolist() and (o2 == w2[1]).all()
            assert pss.check_reps(p1, l1, w1[2], len(r1)) == l1
            assert pss.check_reps(p2, l2, w2[2], len(r2)) == l2
    finally:
        kc.close()


def test_argument_errors(engine, mixed):
    arena, recs = mixed

    def bad(r, a=arena):
        with pytest.raises(RuntimeError, match=r"\(-10\)"):            # FDGPU_ERR_INVAL
            engine.submit_shred_sets(a, r, VERSION)

    r = recs[:8].copy(); r["known_off"][3] = len(arena) - 31
    bad(r)
    r = recs[:8].copy(); r["off"][3] = len(arena) - 100
    bad(r)
    r = recs[:8].copy(); r["pub_off"][0] = len(arena) - 31
    bad(r)
    r = np.zeros(1, dtype=SET_SHRED_DTYPE); r["sz"] = 1233; r["known_off"] = pss.NO_ROOT
    bad(r, np.zeros(4096, dtype=np.uint8))
    bad(np.zeros((1 << 17) + 1, dtype=SET_SHRED_DTYPE))                # n > max_txn
    # nothing was launched and no slot was taken: the ring still takes its two batches; rep and lanes may be NULL
    t1 = engine.submit_shred_sets(arena, recs[:4], VERSION)
    t2 = engine.submit_shred_sets(arena, recs[4:8], VERSION)
    c2, o2, p2, l2 = engine.poll_shred_sets(t2, want_rep=False)
    c1, o1, p1, l1 = engine.poll_shred_sets(t1)
    assert p2 is None and l2 is None and (c2 == 0).all() and (c1 == 0).all() and o2.any(axis=1).all() and l1 >= 1


def test_submit_shreds_unchanged(engine, mixed):
    arena, recs = mixed
    plain = pss.drop_known(recs)
    c0, r0 = engine.verify_shreds(arena, plain, VERSION)
    for _ in range(2):                           # both slots of the ring have carried a set batch
        engine.verify_shred_sets(arena, recs, VERSION)
    c1, r1 = engine.verify_shreds(arena, plain, VERSION)
    assert c0.tobytes() == c1.tobytes() and r0.tobytes() == r1.tobytes()
