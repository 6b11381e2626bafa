"""The PoH check on the GPU (include/fd_poh_gpu.h): leaves, roots, chains,
mixin and comparison against the hashlib model, bit for bit in hashes and
codes; the refill path, the cap, the ring's slot semantics and the block
caller over the engine."""
import numpy as np
import pytest

import pyref_poh as pp
from conftest import load_json
from firedancer_amd import VerifyEngine, tile, workload
from firedancer_amd.ed25519 import (CODE_POH_MISMATCH, CODE_POH_TOO_LONG, POH_DTYPE, POH_HASH_CNT_MAX, POH_NO_MIX,
                                    poh_chunk)

pytestmark = pytest.mark.gpu

CAP = 1 << 16


def same(got, want):
    codes, hashes = got
    want_codes, want_hashes = want
    assert codes.tolist() == want_codes.tolist()
    assert (hashes == want_hashes).all()


@pytest.fixture(scope="module")
def mixed1000():
    """1,000 entries of lengths 1..5,000 and what the model says of them"""
    arena, entries, sig_offs = pp.mixed(1000, np.random.default_rng(31)).arrays()
    return arena, entries, sig_offs, pp.evaluate(arena, entries, sig_offs, CAP)


def test_matrix(engine):
    chunk = poh_chunk()
    arena, entries, sig_offs = pp.matrix(chunk, np.random.default_rng(3)).arrays()
    assert len(entries) == 8 * (2 + len(pp.SIG_CNTS))
    assert sorted(set(entries["hash_cnt"].tolist())) == sorted({0, 1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1})
    assert {int(o) % 16 for o in sig_offs} == set(range(16))
    assert (entries["prev_off"] % 2 == 1).all() and (entries["hash_off"] % 2 == 1).all()
    want = pp.evaluate(arena, entries, sig_offs, CAP)
    assert not want[0].any()
    same(engine.verify_poh(arena, entries, sig_offs, CAP), want)
    same(engine.debug_poh(arena, entries, sig_offs, CAP), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_entry_counts(engine, mixed1000, n):
    arena, entries, sig_offs, (want_codes, want_hashes) = mixed1000
    assert not want_codes.any()
    same(engine.verify_poh(arena, entries[:n], sig_offs, CAP), (want_codes[:n], want_hashes[:n]))


def test_refill_with_one_and_two_waves(engine, mixed1000):
    """300 entries on 64 and on 128 lanes: every lane takes several entries from the queue"""
    arena, entries, sig_offs, (want_codes, want_hashes) = mixed1000
    en = entries[100:400]
    want = want_codes[100:400], want_hashes[100:400]
    full = engine.debug_poh(arena, en, sig_offs, CAP)
    same(full, want)
    for waves in (1, 2):
        same(engine.debug_poh(arena, en, sig_offs, CAP, grid_waves=waves), full)


def test_mismatches(engine):
    """256 entries of one length, so the queue (a stable sort, longest first) keeps the entries' order and each
    wave's first pull takes 64 consecutive entries at lanes 0..63: spoiled entries in every odd lane of the second
    64 and in single lanes of the others.  hash_cnt + 1 goes to entry 0 and hash_cnt - 1 to entry 255, which keep
    their places in the order."""
    rng = np.random.default_rng(41)
    arena, entries, sig_offs = pp.mixed(256, rng, lo=150, hi=150).arrays()
    bad = {i: ("hash", "sig", "prev")[k % 3] for k, i in enumerate(list(range(65, 128, 2)) + [63, 130, 200])}
    bad.update({0: "cnt+", 255: "cnt-"})
    for i, how in bad.items():
        if how == "sig" and not entries["sig_cnt"][i]:
            how = "hash"
        pp.corrupt(arena, entries, sig_offs, i, how, rng)
    assert np.argsort(-entries["hash_cnt"].astype(np.int64), kind="stable").tolist() == list(range(256))
    want_codes, want_hashes = pp.evaluate(arena, entries, sig_offs, CAP)
    assert np.flatnonzero(want_codes).tolist() == sorted(bad) and set(want_codes[sorted(bad)].tolist()) == {CODE_POH_MISMATCH}
    codes, hashes = engine.verify_poh(arena, entries, sig_offs, CAP)
    assert np.flatnonzero(codes == CODE_POH_MISMATCH).tolist() == sorted(bad)
    same((codes, hashes), (want_codes, want_hashes))              # the returned hash is still the model's


def test_cap(engine):
    rng = np.random.default_rng(43)
    arena, entries, sig_offs = pp.mixed(200, rng, lo=1, hi=200).arrays()
    cap = 100
    entries["hash_cnt"][17] = 2**63
    entries["hash_cnt"][64] = cap + 1
    entries["hash_cnt"][65] = cap
    over = entries["hash_cnt"] > cap
    assert 50 < over.sum() < 150
    want_codes, want_hashes = pp.evaluate(arena, entries, sig_offs, cap)
    assert (want_codes[over] == CODE_POH_TOO_LONG).all() and not want_hashes[over].any()
    # the neighbours are unaffected: whatever is within the cap and was not touched still passes
    touched = np.zeros(len(entries), dtype=bool); touched[[17, 64, 65]] = True
    assert not want_codes[~over & ~touched].any()
    same(engine.verify_poh(arena, entries, sig_offs, cap), (want_codes, want_hashes))
    same(engine.debug_poh(arena, entries, sig_offs, cap, grid_waves=1), (want_codes, want_hashes))


def test_mainnet_block_1(engine):
    vec = load_json("poh_vectors.json")["vectors"][1]
    b, last = pp.golden_entries(vec)
    arena, entries, sig_offs = b.arrays()
    assert entries["hash_cnt"].tolist() == [14613, 210348, 428776, 146263] and last.hex() == vec["post"]
    codes, hashes = engine.verify_poh(arena, entries, sig_offs, POH_HASH_CNT_MAX)
    assert codes.tolist() == [0, 0, 0, 0]
    assert hashes[3].tobytes().hex() == vec["post"]
    assert all(hashes[i].tobytes() == arena[int(entries["prev_off"][i + 1]):][:32].tobytes() for i in range(3))


def test_ring(mixed1000, oracle):
    arena, entries, sig_offs, (want_codes, want_hashes) = mixed1000
    e = VerifyEngine(0, max_txn=1 << 10, max_sig=1 << 11, max_arena=1 << 20, ring_depth=2)
    try:
        t1 = e.submit_poh(arena, entries[:300], sig_offs, CAP)
        t2 = e.submit_poh(arena, entries[300:500], sig_offs, CAP)
        with pytest.raises(RuntimeError, match=r"\(-12\)"):          # FDGPU_ERR_FULL
            e.submit_poh(arena, entries[:4], sig_offs, CAP)
        same(e.poll_poh(t2), (want_codes[300:500], want_hashes[300:500]))
        same(e.poll_poh(t1), (want_codes[:300], want_hashes[:300]))
        codes, hashes = e.verify_poh(arena, entries[:0], sig_offs[:0], CAP)   # an empty batch
        assert len(codes) == 0 and hashes.shape == (0, 32)
        # a PoH batch, a shred batch and a signature batch interleaved on one engine
        import pyref_shred as ps
        sh_arena, sh_recs, sh_codes, sh_roots = ps.verify_batch(0x1234, np.random.default_rng(21), workload.sign, oracle.verify)
        sh_recs, sh_codes, sh_roots = sh_recs[:200], sh_codes[:200], sh_roots[:200]
        tx_arena, txns, _ = workload.cfg1(256, seed=9)
        tx_want = oracle.verify_txns(tx_arena, txns)
        for _ in range(2):
            tp = e.submit_poh(arena, entries[500:700], sig_offs, CAP)
            ts = e.submit_shreds(sh_arena, sh_recs, 0x1234)
            same(e.poll_poh(tp), (want_codes[500:700], want_hashes[500:700]))
            tt = e.submit(tx_arena, txns)
            c, r = e.poll_shreds(ts)
            assert c.tolist() == sh_codes.tolist() and (r == sh_roots).all()
            tp = e.submit_poh(arena, entries[700:], sig_offs, CAP)
            assert e.poll(tt).tolist() == tx_want.tolist()
            same(e.poll_poh(tp), (want_codes[700:], want_hashes[700:]))
    finally:
        e.close()


def test_argument_errors(engine, mixed1000):
    arena, entries, sig_offs, _ = mixed1000
    en = entries[:12]

    def bad(e=en, so=sig_offs, cap=CAP, a=arena):
        with pytest.raises(RuntimeError, match=r"\(-10\)"):            # FDGPU_ERR_INVAL
            engine.submit_poh(a, e, so, cap)

    for f in ("prev_off", "hash_off"):
        e = en.copy(); e[f][4] = len(arena) - 31
        bad(e)
    k = int(np.flatnonzero(en["mix_off"] != POH_NO_MIX)[0])
    e = en.copy(); e["mix_off"][k] = len(arena) - 31
    bad(e)
    e = en.copy(); e["sig_cnt"][k] = 1
    bad(e)                                                            # mix_off together with sig_cnt
    e = en.copy(); e["sig_first"][2] = len(sig_offs)
    assert e["sig_cnt"][2]
    bad(e)                                                            # signatures outside sig_offs
    i, j = np.flatnonzero(en["sig_cnt"])[:2]
    e = en.copy(); e["sig_first"][j] = e["sig_first"][i] + e["sig_cnt"][i] - 1
    bad(e)                                                            # two ranges share a signature
    e["sig_first"][j], e["sig_cnt"][j] = e["sig_first"][i], e["sig_cnt"][i]
    bad(e)                                                            # the same range twice
    e = en.copy(); e["sig_first"][i], e["sig_first"][j] = en["sig_first"][j], en["sig_first"][i]
    e["sig_cnt"][i] = e["sig_cnt"][j] = 1
    bad(e)                                                            # disjoint, but not ascending
    so = sig_offs.copy(); so[-1] = len(arena) - 63
    bad(so=so)
    bad(cap=0)
    bad(cap=POH_HASH_CNT_MAX + 1)
    bad(np.zeros((1 << 17) + 1, dtype=POH_DTYPE))                     # n > max_txn
    bad(so=np.zeros((1 << 18) + 1, dtype=np.uint32))                  # sig_total > max_sig
    bad(a=np.zeros((1 << 26) + 1, dtype=np.uint8))                    # the arena does not fit max_arena
    # nothing was launched and no slot was taken: the ring still takes its two batches
    t1 = engine.submit_poh(arena, en, sig_offs, CAP)
    t2 = engine.submit_poh(arena, en, sig_offs, CAP)
    engine.poll_poh(t2); engine.poll_poh(t1)


def test_an_entry_given_twice(engine):
    """Signature ranges are folded in place on the device, so a batch whose entries share one is rejected; the same
    microblocks twice in a batch, their offsets repeated in sig_offs, get the model's answers for both copies."""
    b = pp.Batch(np.random.default_rng(9))
    for ns in (5, 33, 2, 129):
        b.add(30, n_sig=ns)
    arena, entries, sig_offs = b.arrays()
    twice = np.concatenate([entries, entries])
    with pytest.raises(RuntimeError, match=r"\(-10\)"):
        engine.submit_poh(arena, twice, sig_offs, CAP)
    twice["sig_first"][4:] += len(sig_offs)
    twice["hash_cnt"][5] += 1
    so = np.concatenate([sig_offs, sig_offs])
    want = pp.evaluate(arena, twice, so, CAP)
    assert want[0].tolist() == [0, 0, 0, 0, 0, CODE_POH_MISMATCH, 0, 0]
    same(engine.verify_poh(arena, twice, so, CAP), want)
    same(tile.poh_verify_host(arena, twice, so, CAP), want)


def test_block_caller_equals_the_host_path(engine):
    def sigs_of(payload):
        fp, raw = tile.txn_parse(payload)
        h = tile.txn_decode(raw)
        return [payload[h["signature_off"] + 64 * k: h["signature_off"] + 64 * k + 64] for k in range(h["signature_cnt"])]

    arena, txns, _ = workload.cfg3(64, seed=77)
    s = pp.stream(np.random.default_rng(5), workload.payloads(arena, txns), sigs_of)
    m = len(s["hash_cnt"])
    hc = list(s["hash_cnt"]); hc[3] += 1; hc[10] = CAP + 1
    k = next(i for i, c in enumerate(s["txn_cnt"]) if c >= 2)
    ps = list(s["payloads"]); ps[sum(s["txn_cnt"][:k]) + 1] = b"\x00" * 40
    want = [0] * m
    want[3], want[10], want[k] = CODE_POH_MISMATCH, CODE_POH_TOO_LONG, tile.REPLAY_PARSE_FAIL
    for eng, bem in ((None, 5), (engine, 5), (engine, 65536)):
        got = tile.block_poh_verify(eng, s["in_hash"], hc, s["entry_hash"], s["txn_cnt"], ps, CAP, batch_entry_max=bem)
        assert got.tolist() == want, (eng is None, bem)
